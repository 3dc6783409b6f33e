// ga_dev_post.h -- what follows the ladder: the walk over the finished jobs' moves where they lie in the trace pool, coding them as runs
// of operations (GA_F_OPS, ga_ops.h), spelling out the graph's bases along them (GA_F_PATHSEQ, ga_pathseq.h) or adding them to a pileup
// (GA_F_PILEUP, ga_pileup.h, ga_edges.h); a pileup's site queries (ga_sites.h); and the records and moves on their way back to the host (fetch).
// Not a header for others: a part of ga_device.hip's translation unit (ga_dev.h).
#ifndef GA_DEVICE_PARTS
#error "ga_dev_post.h is a part of ga_device.hip"
#endif

namespace {

struct DevBatch final : BatchLadder
{
	using BatchLadder::BatchLadder;
	// (the first destructor of the batch's layers to run: the device is set for all of them)
	~DevBatch() override { hipSetDevice(g->device); fetchDone(); }
	struct Ops
	{
		Events<4> ev;                   // around count, around write
		uint64_t* dOffsets = nullptr;   // device copies, until fetch has brought them down
		uint32_t* dRuns = nullptr;
		uint64_t total = 0, jobs = 0, moves = 0;
		float countMs = 0, writeMs = 0;
		std::vector<uint64_t> offsetsHost;
		std::unique_ptr<uint32_t[]> runsHost;
	} ops;
	struct PathSeq
	{
		Events<4> ev;                   // around count, around write
		uint64_t* dOffsets = nullptr;   // device copies, until fetch has brought them down
		uint8_t* dBases = nullptr;
		uint64_t total = 0, jobs = 0, moves = 0;
		float countMs = 0, writeMs = 0;
		std::vector<uint64_t> offsetsHost;
		std::unique_ptr<uint8_t[]> basesHost;
	} pathSeq;
	struct PileupAdd { Events<2> ev; } pileupAdd;
	struct HostTraces
	{
		uint8_t* at = nullptr;          // the graph's pinned buffer (fromPool) or a private one
		bool fromPool = false;
		std::unique_ptr<uint8_t[]> own;
		size_t ownBytes = 0;
	} host;

	int run() override
	{
		int rc = runLadder();
		if (rc) return rc;
		if (cfg.emit_ops)
		{
			releaseOps();
			ops.total = ops.jobs = ops.moves = 0; ops.countMs = ops.writeMs = 0;
			ops.offsetsHost.clear(); ops.runsHost.reset();
			if (jobs.empty()) { ops.offsetsHost.assign(1, 0); ops.runsHost.reset(new uint32_t[1]); }
			else if (int s = runOps()) return s;
		}
		if (cfg.emit_pathseq)
		{
			releasePathSeq();
			pathSeq.total = pathSeq.jobs = pathSeq.moves = 0; pathSeq.countMs = pathSeq.writeMs = 0;
			pathSeq.offsetsHost.clear(); pathSeq.basesHost.reset();
			if (jobs.empty()) { pathSeq.offsetsHost.assign(1, 0); pathSeq.basesHost.reset(new uint8_t[1]); }
			else if (int s = runPathSeq()) return s;
		}
		return 0;
	}

	// ---- the walk (ga_ops.h: run_wave and its callers): one wave per job at a time, over `n` jobs ------------------------------------
	const uint32_t* twinTable() { std::lock_guard<std::mutex> guard(g->twinLock); return g->dTwin ? g->dTwin : g->dOpsTwin; }
	uint32_t walkWaves(size_t n) const
	{
		const uint32_t waves = (uint32_t)std::min<size_t>(n, (size_t)g->cus * 16);
		return knobs.waveSlots ? std::min(waves, knobs.waveSlots) : waves;
	}
	// what the walk reads: the jobs, their records and moves, the reads as the prepare left them, the row codes and the graph's twin table
	gao::OpsLaunch walkLaunch(const uint8_t* dLut, const uint32_t* twin) const
	{
		gao::OpsLaunch O;
		memset(&O, 0, sizeof(O));
		O.graph = L.graph; O.jobs = L.jobs; O.outs = L.outs; O.fills = res.fills;
		O.traces = L.traces; O.trace_bytes = L.trace_pool_cap;
		O.seq = res.seq; O.seq_bytes = res.seqBytes; O.row_code = dLut;
		O.twin = twin;
		O.n_jobs = (uint32_t)jobs.size();
		return O;
	}

	// ---- GA_F_OPS (ga_ops.h): after the last pass, every finished job's moves coded as runs where they lie -------------------------
	void releaseOps()
	{
		if (ops.dOffsets) blocks.release(ops.dOffsets);
		if (ops.dRuns) blocks.release(ops.dRuns);
		ops.dOffsets = nullptr; ops.dRuns = nullptr;
	}
	int runOps()
	{
		if (!res.seq || !res.fills) return GA_E_INVALID;
		const size_t n = jobs.size();
		uint64_t* dCounts; uint8_t *dLut, *dTmp;
		if (alloc(&dCounts, n + 1) || alloc(&ops.dOffsets, n + 1) || alloc(&dLut, 256)) return GA_E_DEVICE;
		Scan<uint64_t> place{dCounts, ops.dOffsets, n + 1};
		if (int s = place.size(stream)) return s;
		if (alloc(&dTmp, place.tmpBytes + 16)) return GA_E_DEVICE;
		if (int s = ops.ev.create()) return s;
		HIP_OK(hipMemcpyAsync(dLut, res.lut, 256, hipMemcpyHostToDevice, stream));
		HIP_OK(hipMemsetAsync(dCounts, 0, (n + 1) * 8, stream));
		if (uploadList(orderHost)) return GA_E_DEVICE;           // longest first, dealt statically: wave w takes entries w, w + waves, ...
		gao::OpsLaunch O = walkLaunch(dLut, twinTable());
		if (!O.twin) return GA_E_INVALID;
		O.job_list = dList;
		O.counts = dCounts; O.offsets = ops.dOffsets;
		const uint32_t waves = walkWaves(n);
		HIP_OK(hipEventRecord(ops.ev[0], stream));
		hipLaunchKernelGGL(ga_ops_count_kernel, dim3(waves), dim3(64), 0, stream, O);
		HIP_OK(hipGetLastError());
		HIP_OK(hipEventRecord(ops.ev[1], stream));
		if (int s = place.run(dTmp, stream)) return s;
		HIP_OK(hipMemcpyAsync(&ops.total, ops.dOffsets + n, 8, hipMemcpyDeviceToHost, stream));
		HIP_OK(hipStreamSynchronize(stream));
		if (alloc(&ops.dRuns, ops.total + 1)) return GA_E_DEVICE;
		O.runs = ops.dRuns;
		HIP_OK(hipEventRecord(ops.ev[2], stream));
		hipLaunchKernelGGL(ga_ops_write_kernel, dim3(waves), dim3(64), 0, stream, O);
		HIP_OK(hipGetLastError());
		HIP_OK(hipEventRecord(ops.ev[3], stream));
		HIP_OK(hipStreamSynchronize(stream));
		if (ops.ev.elapsed(0, 1, ops.countMs) || ops.ev.elapsed(2, 3, ops.writeMs)) return GA_E_DEVICE;
		blocks.release(dCounts); blocks.release(dTmp); blocks.release(dLut);
		ops.jobs = ops.moves = 0;
		for (const GaJobOut& o : outs) if (movesCount(o)) { ops.jobs++; ops.moves += o.trace_len; }
		if (knobs.debugPasses) fprintf(stderr, "graphaligner_amd: operations: %llu jobs, %llu moves, %llu runs on %u waves, count %.2f ms, write %.2f ms\n",
		                               (unsigned long long)ops.jobs, (unsigned long long)ops.moves, (unsigned long long)ops.total, waves, ops.countMs, ops.writeMs);
		return 0;
	}
	int fetchOps(GaOpsOut& out) override
	{
		if (!cfg.emit_ops) return GA_E_INVALID;
		out.runs = ops.runsHost.get(); out.offsets = ops.offsetsHost.empty() ? nullptr : ops.offsetsHost.data();
		out.n_runs = ops.total; out.count_ms = ops.countMs; out.write_ms = ops.writeMs; out.jobs = ops.jobs; out.moves = ops.moves;
		return 0;
	}

	// ---- GA_F_PATHSEQ (ga_pathseq.h): after the last pass (and the operations), every finished job's bases along its moves ----------
	void releasePathSeq()
	{
		if (pathSeq.dOffsets) blocks.release(pathSeq.dOffsets);
		if (pathSeq.dBases) blocks.release(pathSeq.dBases);
		pathSeq.dOffsets = nullptr; pathSeq.dBases = nullptr;
	}
	int runPathSeq()
	{
		if (!res.fills) return GA_E_INVALID;
		const size_t n = jobs.size();
		uint64_t* dCounts; uint8_t* dTmp;
		if (alloc(&dCounts, n + 1) || alloc(&pathSeq.dOffsets, n + 1)) return GA_E_DEVICE;
		Scan<uint64_t> place{dCounts, pathSeq.dOffsets, n + 1};
		if (int s = place.size(stream)) return s;
		if (alloc(&dTmp, place.tmpBytes + 16)) return GA_E_DEVICE;
		if (int s = pathSeq.ev.create()) return s;
		HIP_OK(hipMemsetAsync(dCounts, 0, (n + 1) * 8, stream));
		if (uploadList(orderHost)) return GA_E_DEVICE;           // longest first, dealt statically, as the operations are
		gaps::PathLaunch P;
		memset(&P, 0, sizeof(P));
		P.walk = walkLaunch(nullptr, twinTable());               // (no read character is looked at: no row codes)
		if (!P.walk.twin) return GA_E_INVALID;
		P.walk.job_list = dList;
		P.walk.counts = dCounts; P.walk.offsets = pathSeq.dOffsets;
		const uint32_t waves = walkWaves(n);
		HIP_OK(hipEventRecord(pathSeq.ev[0], stream));
		hipLaunchKernelGGL(ga_pathseq_count_kernel, dim3(waves), dim3(64), 0, stream, P);
		HIP_OK(hipGetLastError());
		HIP_OK(hipEventRecord(pathSeq.ev[1], stream));
		if (int s = place.run(dTmp, stream)) return s;
		HIP_OK(hipMemcpyAsync(&pathSeq.total, pathSeq.dOffsets + n, 8, hipMemcpyDeviceToHost, stream));
		HIP_OK(hipStreamSynchronize(stream));
		if (alloc(&pathSeq.dBases, pathSeq.total + 1)) return GA_E_DEVICE;
		P.bases = pathSeq.dBases;
		HIP_OK(hipEventRecord(pathSeq.ev[2], stream));
		hipLaunchKernelGGL(ga_pathseq_write_kernel, dim3(waves), dim3(64), 0, stream, P);
		HIP_OK(hipGetLastError());
		HIP_OK(hipEventRecord(pathSeq.ev[3], stream));
		HIP_OK(hipStreamSynchronize(stream));
		if (pathSeq.ev.elapsed(0, 1, pathSeq.countMs) || pathSeq.ev.elapsed(2, 3, pathSeq.writeMs)) return GA_E_DEVICE;
		blocks.release(dCounts); blocks.release(dTmp);
		pathSeq.jobs = pathSeq.moves = 0;
		for (const GaJobOut& o : outs) if (movesCount(o)) { pathSeq.jobs++; pathSeq.moves += o.trace_len; }
		if (knobs.debugPasses) fprintf(stderr, "graphaligner_amd: path sequences: %llu jobs, %llu moves, %llu bases on %u waves, count %.2f ms, write %.2f ms\n",
		                               (unsigned long long)pathSeq.jobs, (unsigned long long)pathSeq.moves, (unsigned long long)pathSeq.total, waves, pathSeq.countMs, pathSeq.writeMs);
		return 0;
	}
	int fetchPathSeq(GaPathSeqOut& out) override
	{
		if (!cfg.emit_pathseq) return GA_E_INVALID;
		out.bases = pathSeq.basesHost.get(); out.offsets = pathSeq.offsetsHost.empty() ? nullptr : pathSeq.offsetsHost.data();
		out.n_bases = pathSeq.total; out.count_ms = pathSeq.countMs; out.write_ms = pathSeq.writeMs; out.jobs = pathSeq.jobs; out.moves = pathSeq.moves;
		return 0;
	}

	// ---- GA_F_PILEUP (ga_pileup.h): the winning jobs' moves, still in the trace pool after the collect, added to a pileup -----------
	int addToPileup(GaBackendPileup* to, const GaPileupAdd& add, GaPileupAddOut& out) override
	{
		DevPileup* p = static_cast<DevPileup*>(to);
		if (!cfg.emit_pileup || !p || p->device != g->device || p->entries != ga_pileup_entries((int)p->kind, g->totalBp, g->edgeSlots)) return GA_E_INVALID;
		out = GaPileupAddOut();
		const bool edges = p->kind == (uint32_t)GA_KIND_EDGES;
		if (!add.nList && !(edges ? add.nSlots : add.nPairs)) return 0;
		// everything that can refuse the add is looked at before a block is taken or anything is put on the stream
		const uint32_t* twin = nullptr;
		if (add.nList)
		{
			if (!res.seq || !res.fills) return GA_E_INVALID;
			twin = twinTable();
			if (!twin) return GA_E_INVALID;
		}
		HIP_OK(hipSetDevice(g->device));
		if (int s = pileupAdd.ev.create()) return s;
		// the add's blocks go back to the graph's list whether or not it went through: the lease ends here, with the stream idle
		// (addWith has waited for it, or end() does)
		BlockLease held(g, true);
		return held.end(addWith(p, add, twin, out, held), stream);
	}
	int addWith(DevPileup* p, const GaPileupAdd& add, const uint32_t* twin, GaPileupAddOut& out, BlockLease& held)
	{
		const Events<2>& ev = pileupAdd.ev;
		uint32_t *dJobList = nullptr, *dSlots = nullptr; uint64_t* dPairs = nullptr; uint8_t* dLut = nullptr; unsigned long long* dAdded = nullptr;
		// the EDGES kind takes the host's crossings (slot indices) where the other kinds take its items (plane, column)
		const bool edges = p->kind == (uint32_t)GA_KIND_EDGES;
		const size_t nPairs = edges ? 0 : add.nPairs, nSlots = edges ? add.nSlots : 0;
		if (held.take(&dAdded, 1)) return GA_E_DEVICE;
		HIP_OK(hipMemsetAsync(dAdded, 0, 8, stream));
		if (add.nList)
		{
			if (held.take(&dJobList, add.nList) || held.take(&dLut, 256)) return GA_E_DEVICE;
			HIP_OK(hipMemcpyAsync(dJobList, add.list, add.nList * 4, hipMemcpyHostToDevice, stream));
			HIP_OK(hipMemcpyAsync(dLut, res.lut, 256, hipMemcpyHostToDevice, stream));
		}
		if (nPairs)
		{
			if (held.take(&dPairs, nPairs)) return GA_E_DEVICE;
			HIP_OK(hipMemcpyAsync(dPairs, add.pairs, nPairs * 8, hipMemcpyHostToDevice, stream));
		}
		if (nSlots)
		{
			if (held.take(&dSlots, nSlots)) return GA_E_DEVICE;
			HIP_OK(hipMemcpyAsync(dSlots, add.slots, nSlots * 4, hipMemcpyHostToDevice, stream));
		}
		HIP_OK(hipEventRecord(ev[0], stream));
		const uint32_t waves = walkWaves(add.nList);
		if (add.nList && edges)
		{
			gaed::EdgesLaunch P;
			memset(&P, 0, sizeof(P));
			P.walk = walkLaunch(dLut, twin);
			P.counts = p->planes; P.mirror = p->mirror; P.entries = p->entries;
			P.list = dJobList; P.n_list = (uint32_t)add.nList; P.added = dAdded;
			hipLaunchKernelGGL(ga_pileup_edges_kernel, dim3(waves), dim3(64), 0, stream, P);
			HIP_OK(hipGetLastError());
		}
		else if (add.nList)
		{
			gapl::PileupLaunch P;
			memset(&P, 0, sizeof(P));
			P.walk = walkLaunch(dLut, twin);
			P.planes = p->planes; P.columns = p->entries; P.kind = p->kind;
			P.list = dJobList; P.n_list = (uint32_t)add.nList; P.added = dAdded;
			if (p->kind == gapl::KIND_BASES) hipLaunchKernelGGL(ga_pileup_bases_kernel, dim3(waves), dim3(64), 0, stream, P);
			else hipLaunchKernelGGL(ga_pileup_depth_kernel, dim3(waves), dim3(64), 0, stream, P);
			HIP_OK(hipGetLastError());
		}
		if (nPairs)
		{
			hipLaunchKernelGGL(ga_pileup_pairs_kernel, dim3((uint32_t)((nPairs + 255) / 256)), dim3(256), 0, stream, dPairs, (uint64_t)nPairs, p->planes, p->entries, p->kind);
			HIP_OK(hipGetLastError());
		}
		if (nSlots)
		{
			hipLaunchKernelGGL(ga_pileup_slots_kernel, dim3((uint32_t)((nSlots + 255) / 256)), dim3(256), 0, stream, dSlots, (uint64_t)nSlots, p->planes, p->entries);
			HIP_OK(hipGetLastError());
		}
		HIP_OK(hipEventRecord(ev[1], stream));
		unsigned long long added = 0;
		HIP_OK(hipMemcpyAsync(&added, dAdded, 8, hipMemcpyDeviceToHost, stream));
		HIP_OK(hipStreamSynchronize(stream));
		float ms = 0;
		if (int s = ev.elapsed(0, 1, ms)) return s;
		out.kernel_ms = ms; out.items = added;
		for (size_t k = 0; k < add.nList; k++)
		{
			const uint32_t job = add.list[k] & ~gapl::kCounts;
			if (!(add.list[k] & gapl::kCounts) || job >= outs.size()) continue;
			if (movesCount(outs[job])) { out.jobs++; out.moves += outs[job].trace_len; }
		}
		for (size_t k = 0; k < nPairs; k++)
			if (ga_pileup_plane_in_kind(p->kind, (uint32_t)(add.pairs[k] >> 56)) < p->nPlanes && (add.pairs[k] & 0x00ffffffffffffffull) < p->entries) out.items++;
		for (size_t k = 0; k < nSlots; k++) if (add.slots[k] < p->entries) out.items++;
		if (knobs.debugPasses) fprintf(stderr, "graphaligner_amd: pileup: %llu jobs, %llu moves, %llu items (%zu from the host), %.2f ms\n",
		                               (unsigned long long)out.jobs, (unsigned long long)out.moves, (unsigned long long)out.items, nPairs + nSlots, ms);
		return 0;
	}

	// ---- the way back: the records, the moves (into the graph's pinned buffer or a private one) and the operations ------------------
	int fetch(std::vector<GaJobOut>& o, const uint8_t** traces, uint64_t* nBytes) override
	{
		HIP_OK(hipSetDevice(g->device));
		fetchDone();
		o = outs;
		for (size_t i = 0; i < o.size(); i++) o[i].reserved2 = passOf[i];      // 0 = finished by the first pass
		uint64_t top = 0;
		// (on the batch's own stream: the null stream would make this wait for whatever kernel another batch is running)
		HIP_OK(hipMemcpyAsync(&top, L.trace_top, 8, hipMemcpyDeviceToHost, stream));
		HIP_OK(hipStreamSynchronize(stream));
		top = std::min<uint64_t>(top, L.trace_pool_cap);
		host.at = g->takeHost(top + 64);
		host.fromPool = host.at != nullptr;
		if (!host.at)
		{
			// another batch of this graph is being assembled from the pinned buffer: pageable memory, not initialised first
			if (host.ownBytes < top + 64) { host.own.reset(new uint8_t[top + 64]); host.ownBytes = top + 64; }
			host.at = host.own.get();
		}
		if (top)
		{
			HIP_OK(hipMemcpyAsync(host.at, L.traces, top, hipMemcpyDeviceToHost, stream));
			HIP_OK(hipStreamSynchronize(stream));
		}
		*traces = host.at;
		*nBytes = top;
		if (cfg.emit_ops && ops.dOffsets)
		{
			// the runs and their places come down with the records; their buffers go back to the graph's block list
			ops.offsetsHost.resize(jobs.size() + 1);
			ops.runsHost.reset(new uint32_t[ops.total + 1]);
			HIP_OK(hipMemcpyAsync(ops.offsetsHost.data(), ops.dOffsets, ops.offsetsHost.size() * 8, hipMemcpyDeviceToHost, stream));
			if (ops.total) HIP_OK(hipMemcpyAsync(ops.runsHost.get(), ops.dRuns, ops.total * 4, hipMemcpyDeviceToHost, stream));
			HIP_OK(hipStreamSynchronize(stream));
			releaseOps();
		}
		if (cfg.emit_pathseq && pathSeq.dOffsets)
		{
			// ... and so do the bases and theirs
			pathSeq.offsetsHost.resize(jobs.size() + 1);
			pathSeq.basesHost.reset(new uint8_t[pathSeq.total + 1]);
			HIP_OK(hipMemcpyAsync(pathSeq.offsetsHost.data(), pathSeq.dOffsets, pathSeq.offsetsHost.size() * 8, hipMemcpyDeviceToHost, stream));
			if (pathSeq.total) HIP_OK(hipMemcpyAsync(pathSeq.basesHost.get(), pathSeq.dBases, pathSeq.total, hipMemcpyDeviceToHost, stream));
			HIP_OK(hipStreamSynchronize(stream));
			releasePathSeq();
		}
		return 0;
	}
	void fetchDone() override
	{
		if (host.fromPool) g->giveHost();
		host.fromPool = false;
		host.at = nullptr;
	}
};

// ---- site queries (ga_sites.h) -----------------------------------------------------------------------------------------------------
int DevPileup::sites(const GaSiteQuery& q, GaSitesOut& out)
{
	out = GaSitesOut();
	const bool edges = kind == (uint32_t)GA_KIND_EDGES, foldNodes = q.fold && !edges;
	if (!g || q.first > entries || q.n > entries - q.first || q.alt_den == 0) return GA_E_INVALID;
	if (foldNodes && (!q.foldTable || q.nNodes != g->g.n_nodes)) return GA_E_INVALID;
	if (q.fold && edges && !mirror) return GA_E_INVALID;
	if (q.n == 0) return 0;
	std::lock_guard<std::mutex> one(g->sitesLock);
	HIP_OK(hipSetDevice(device));
	if (int s = g->sitesStream.create()) return s;
	if (int s = g->evS.create()) return s;
	if (foldNodes && !g->dFold)
		if (int s = g->uploadOnce({{(void**)&g->dFold, q.foldTable, (size_t)q.nNodes * 4}}, g->sitesStream)) return s;
	// the query's blocks go back to the graph's list whether or not it went through: the lease ends here, with the stream idle
	// (sitesWith has waited for it, or end() does)
	BlockLease held(g, false);
	return held.end(sitesWith(q, out, held), g->sitesStream);
}

int DevPileup::sitesWith(const GaSiteQuery& q, GaSitesOut& out, BlockLease& held)
{
	hipStream_t stream = g->sitesStream;
	gast::SitesLaunch L;
	memset(&L, 0, sizeof(L));
	L.planes = planes; L.entries = entries; L.kind = kind; L.nPlanes = nPlanes;
	L.fold = q.fold ? 1u : 0u; L.n_nodes = g->g.n_nodes;
	L.node_start = g->g.node_start; L.fold_table = g->dFold; L.mirror = mirror;
	L.first = q.first; L.n = q.n;
	L.min_depth = q.min_depth; L.min_alt = q.min_alt; L.alt_num = q.alt_num; L.alt_den = q.alt_den;
	L.n_tiles = (q.n + gast::kTile - 1) / gast::kTile;
	const size_t nT = (size_t)L.n_tiles;
	uint64_t *dCounts, *dOffsets; uint8_t* dTmp;
	if (held.take(&dCounts, nT + 1) || held.take(&dOffsets, nT + 1) || held.take(&L.mask, nT * gast::kRounds)) return GA_E_DEVICE;
	L.counts = dCounts; L.offsets = dOffsets;
	Scan<uint64_t> place{dCounts, dOffsets, nT + 1};
	if (int s = place.size(stream)) return s;
	if (held.take(&dTmp, place.tmpBytes + 16)) return GA_E_DEVICE;
	HIP_OK(hipMemsetAsync(dCounts + nT, 0, 8, stream));
	// enough waves to keep the memory system busy: a wave has 8 (fold: 16) loads of 256 bytes in flight
	const uint32_t waves = (uint32_t)std::min<uint64_t>(L.n_tiles, (uint64_t)std::max(g->cus, 1) * 32);
	HIP_OK(hipEventRecord(g->evS[0], stream));
	hipLaunchKernelGGL(ga_pileup_sites_mark_kernel, dim3(waves), dim3(64), 0, stream, L);
	HIP_OK(hipGetLastError());
	if (int s = place.run(dTmp, stream)) return s;
	uint64_t total = 0;
	HIP_OK(hipMemcpyAsync(&total, dOffsets + nT, 8, hipMemcpyDeviceToHost, stream));
	HIP_OK(hipStreamSynchronize(stream));
	if (total > q.n) return GA_E_DEVICE;
	const uint64_t nRecs = q.max_sites ? std::min(total, q.max_sites) : total;
	if (nRecs)
	{
		if (held.take(&L.recs, (size_t)nRecs)) return GA_E_DEVICE;
		L.n_recs = nRecs;
		hipLaunchKernelGGL(ga_pileup_sites_write_kernel, dim3(waves), dim3(64), 0, stream, L);
		HIP_OK(hipGetLastError());
	}
	HIP_OK(hipEventRecord(g->evS[1], stream));
	out.recs.resize((size_t)nRecs);
	if (nRecs) HIP_OK(hipMemcpyAsync(out.recs.data(), L.recs, (size_t)nRecs * sizeof(GaSiteRec), hipMemcpyDeviceToHost, stream));
	HIP_OK(hipStreamSynchronize(stream));
	float ms = 0;
	if (int s = g->evS.elapsed(0, 1, ms)) return s;
	out.n_total = total; out.kernel_ms = ms;
	return 0;
}

}  // namespace
