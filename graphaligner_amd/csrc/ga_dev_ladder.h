// ga_dev_ladder.h -- the device batch's run: ga_ladder.h decides which variant runs over which jobs, in which order; here is how each
// one is run.  The scratch geometry of the lanes = reads and the wave-per-read variants, the frame every pass has (pass), the two kinds
// of pass, launch() -- the one place that names the kernels' template arguments -- and runLadder.
// Not a header for others: a part of ga_device.hip's translation unit (ga_dev.h).
#ifndef GA_DEVICE_PARTS
#error "ga_dev_ladder.h is a part of ga_device.hip"
#endif

namespace {

struct BatchLadder : BatchPrepared
{
	using BatchPrepared::BatchPrepared;
	~BatchLadder() override { if (privateScratch) hipFree(privateScratch); }
	std::vector<uint8_t> passOf;       // which pass of the last run finished each job (0 = the first)
	int passNo = 0;
	GaRunStats st;
	GaRunStats stats() const override { return st; }
	uint8_t* privateScratch = nullptr; // only when the graph's pool is taken by another batch
	size_t privateBytes = 0;

	int ensureRows()
	{
		if (L.rows) return 0;
		if (res.rows) { L.rows = res.rows; return 0; }                            // (written by the match-word kernel)
		const std::vector<uint8_t>& rows = rowsProvider();
		uint8_t* dRows;
		if (alloc(&dRows, rows.size())) return GA_E_DEVICE;
		HIP_OK(hipMemcpyAsync(dRows, rows.data(), rows.size(), hipMemcpyHostToDevice, stream));
		L.rows = dRows;
		return 0;
	}

	// scratch for one pass: the graph's pool, or a private allocation while another batch holds the pool
	uint8_t* takeScratch(size_t bytes, bool& fromPool)
	{
		uint8_t* p = g->takePool(bytes);
		fromPool = p != nullptr;
		if (p) return p;
		if (bytes > privateBytes)
		{
			if (privateScratch) hipFree(privateScratch);
			privateScratch = nullptr; privateBytes = 0;
			if (hipMalloc((void**)&privateScratch, bytes) != hipSuccess) { privateScratch = nullptr; return nullptr; }
			privateBytes = bytes;
		}
		return privateScratch;
	}
	size_t scratchBudget() const
	{
		size_t freeB = 0, totalB = 0;
		if (hipMemGetInfo(&freeB, &totalB) != hipSuccess) return 0;
		const size_t poolFree = g->poolBytesIfFree();
		return (size_t)((freeB + (poolFree ? poolFree : privateBytes)) * 0.85);
	}
	uint32_t longestJob(const std::vector<uint32_t>& list) const
	{
		uint32_t maxRows = 0;
		for (uint32_t i : list) maxRows = std::max(maxRows, jobs[i].n_rows);
		return maxRows;
	}
	int afterPass(float& ms)
	{
		HIP_OK(hipGetLastError());
		HIP_OK(hipEventRecord(evPass[1], stream));
		HIP_OK(hipMemcpyAsync(outs.data(), L.outs, outs.size() * sizeof(GaJobOut), hipMemcpyDeviceToHost, stream));
		HIP_OK(hipStreamSynchronize(stream));
		if (int s = evPass.elapsed(0, 1, ms)) return s;
		st.kernel_ms += ms;
		return 0;
	}

	// the frame of every pass: scratch of `scratchBytes` (from the pool, which goes back whatever happens, or private), the job list, the
	// queue counter cleared, what else the variant clears (`clear`: a status), then the first event, the kernel (`launch`) and afterPass.
	// Not run (and rc 0) when there is no memory for the scratch: the jobs keep their status and climb on.
	struct PassRun { int rc = 0; bool ran = false; float ms = 0; };
	template <typename Clear, typename Launch> PassRun pass(const std::vector<uint32_t>& list, size_t scratchBytes, Clear clear, Launch launch)
	{
		PassRun r;
		bool fromPool = false;
		uint8_t* scratch = takeScratch(scratchBytes, fromPool);
		if (!scratch) return r;
		r.rc = uploadList(list);
		if (!r.rc)
		{
			hipMemsetAsync(L.next_job, 0, 16, stream);
			r.rc = clear(scratch);
		}
		if (!r.rc)
		{
			hipEventRecord(evPass[0], stream);
			launch(scratch);
			r.rc = afterPass(r.ms);
			r.ran = true;
		}
		if (fromPool) g->givePool();
		return r;
	}

	// third diagnostic layout of the stamps build: when the waves of the pass in hand ran and for how long
	void reportWaveLives() const
	{
#if GA_STAMPS == 3
		uint64_t lo = ~0ull, hi = 0, n = 0; double life = 0, cyc = 0, lateStart = 0;
		for (auto& o : outs) if (o.stamps[1]) { lo = std::min(lo, o.stamps[0]); hi = std::max(hi, o.stamps[1]); }
		for (auto& o : outs) if (o.stamps[1]) { n++; life += (double)(o.stamps[1] - o.stamps[0]); cyc += (double)o.stamps[4]; lateStart = std::max(lateStart, (double)(o.stamps[0] - lo)); }
		{
			// the spread of the waves' lifetimes, and what goes with a long one (fill steps are not known per wave; traceback rounds are)
			std::vector<std::pair<double, uint64_t>> lives;
			for (auto& o : outs) if (o.stamps[1]) lives.push_back({(double)(o.stamps[1] - o.stamps[0]) / 1e5, o.stamps[7]});
			std::sort(lives.begin(), lives.end());
			auto at = [&](double q) { return lives[(size_t)(q * (lives.size() - 1))]; };
			if (!lives.empty()) fprintf(stderr, "graphaligner_amd: wave life ms p10 %.2f p50 %.2f p90 %.2f p99 %.2f max %.2f; traceback rounds of the p10 / p50 / p99 / max wave: %llu / %llu / %llu / %llu, fast iterations %llu / %llu / %llu / %llu\n",
				at(0.1).first, at(0.5).first, at(0.9).first, at(0.99).first, at(1.0).first,
				(unsigned long long)(at(0.1).second & 0xffffffffu), (unsigned long long)(at(0.5).second & 0xffffffffu), (unsigned long long)(at(0.99).second & 0xffffffffu), (unsigned long long)(at(1.0).second & 0xffffffffu),
				(unsigned long long)(at(0.1).second >> 32), (unsigned long long)(at(0.5).second >> 32), (unsigned long long)(at(0.99).second >> 32), (unsigned long long)(at(1.0).second >> 32));
		}
		if (n) fprintf(stderr, "graphaligner_amd: %llu waves: first start to last end %.3f ms, mean wave life %.3f ms = %.1f M shader cycles (%.2f GHz), latest start %.3f ms after the first\n",
		               (unsigned long long)n, (hi - lo) / 1e5, life / n / 1e5, cyc / n / 1e6, cyc / life / 10.0, lateStart / 1e5);
#endif
	}

	// lanes = reads variants <10,64>, <24,32>, <56,16>: arena rows per lane and slice -- the band's columns rounded up to blocks of 8 per
	// node, with room for the widest slices.  (10 / 24 / 56 band nodes per lane = 4 / 2 / 1 waves per CU next to the 12.8 KB block image.
	// The wider tables trade lanes for LDS per lane: 32 and 16 lanes per wave keep four waves on every CU -- the same number of reads in
	// flight as 64-lane waves that leave three SIMDs of four idle, in four times as many instruction streams.)
	static constexpr uint32_t kLanesRowsPerSlice[] = {288, 480, 768};

	// one launch of the lanes = reads kernel over `list` (job indices, longest first)
	template <int N, int LW> int lanesPass(const std::vector<uint32_t>& list, uint32_t rowsPerSlice, bool first)
	{
		gal::GaLanesLaunch P;
		memset(&P, 0, sizeof(P));
		P.graph = L.graph; P.hmm = L.hmm; P.eq = dEq; P.jobs = L.jobs; P.outs = L.outs;
		P.job_list = dList; P.n_jobs = (uint32_t)list.size();
		P.lanes_per_wave = LW;
		P.next_group = L.next_job;
		P.traces = L.traces; P.trace_top = L.trace_top; P.trace_pool_cap = L.trace_pool_cap;
		P.initial_bw = L.initial_bw; P.ramp_bw = L.ramp_bw;
		P.emit_runs = cfg.emit_runs;
		const uint32_t maxRows = longestJob(list);
		P.max_slices = std::max<uint32_t>(maxRows / 64, 1);
		P.cap_cols = std::min<uint32_t>(N * 256u, 0xff00u);
		// (node runs are five words each: the staging plane holds a run per ten rows -- six times what a path over 64-bp nodes makes; a
		// job that needs more reports GA_CAP_TRACE and climbs on)
		P.cap_moves = maxRows * 2 + 1024;
		const uint32_t ldsBytes = gal::Lay<N>::WORDS * LW * 4 + LW * gal::kStageWords64 * 8 + 512;
		const uint32_t wavesPerCu = std::max<uint32_t>(1, std::min<uint32_t>(8, 163840u / ldsBytes));
		// arena rows of a wave = the band columns of its lanes (in blocks of 8 per node), `rowsPerSlice` per lane and slice: sized for the
		// lanes a wave will really carry
		auto layoutFor = [&](uint32_t lanes) {
			P.cap_rows = (uint32_t)std::min<uint64_t>(((uint64_t)P.max_slices * rowsPerSlice * lanes + 64 + 7u) & ~7ull, 0x7ffffff0ull);
			return gal::wave_layout<N>(P.cap_cols, P.cap_rows, P.max_slices, P.cap_moves, LW);
		};
		gal::WaveLayout lay = layoutFor(LW);
		const uint64_t fit = scratchBudget() / std::max<uint64_t>(lay.bytes, 1);
		uint64_t slotsHere = std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)g->cus * wavesPerCu, std::max<uint64_t>(fit, 64)));
		if (knobs.waveSlots) slotsHere = std::min<uint64_t>(slotsHere, knobs.waveSlots);
		// a SMALL batch is spread over all wave slots: a wave's steps cost the same with fewer lanes, and fewer lanes wait for each
		// other less.  A batch that gives at least six of ten slots a full wave runs in full waves: round 3's kernel is more sensitive
		// to the waves it shares its CU's memory path with than to the lanes it waits for (50 000 reads: 782 full waves 28.5 ms,
		// 1 021 waves of 49 reads 30.2 ms on the same box, profiles/r3_ab_lanes_per_wave.txt; round 2's kernel: the other way round)
		uint32_t lanesPer = LW;
		if (knobs.spread > 1) lanesPer = (uint32_t)std::min<int>(LW, knobs.spread);
		else if (knobs.spread && list.size() * 10 < slotsHere * LW * 6)
			lanesPer = (uint32_t)std::min<uint64_t>(LW, std::max<uint64_t>(8, (list.size() + slotsHere - 1) / slotsHere));
		P.lanes_per_wave = lanesPer;
		lay = layoutFor(lanesPer);
		P.wave_bytes = lay.bytes;
		const uint64_t groups = (list.size() + lanesPer - 1) / lanesPer;
		const uint32_t waves = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(slotsHere, groups));
		const PassRun r = pass(list, (size_t)waves * lay.bytes, [](uint8_t*) { return 0; }, [&](uint8_t* scratch) {
			P.scratch = scratch;
			if (P.emit_runs) hipLaunchKernelGGL((ga_lanes_kernel<N, LW>), dim3(waves), dim3(64), 0, stream, P);
			else hipLaunchKernelGGL((ga_lanes_moves_kernel<N, LW>), dim3(waves), dim3(64), 0, stream, P);
		});
		if (!r.ran) return r.rc;
		if (first) { st.main_ms = r.ms; st.main_variant = N * 1000 + 80 + (LW == 64 ? 0 : 1); st.slots = waves; st.waves_per_cu = wavesPerCu; st.scratch_bytes = (uint64_t)waves * lay.bytes; }
		if (knobs.debugPasses) fprintf(stderr, "graphaligner_amd: lanes pass <%d,%d>: %zu jobs on %u waves of %u lanes (%.1f GB scratch), %.2f ms\n", N, LW, list.size(), waves, lanesPer, waves * (double)lay.bytes / 1e9, r.ms);
		reportWaveLives();
		return r.rc;
	}

	// the wave-per-read variants: the kernel behind each and what the host has to know about it.  The two with 4 096 band nodes keep
	// their WaveState in the wave's scratch slot in HBM (stateBytes); the two that carry the sparse method have generation-stamped
	// tables, sized for sparseNodes band nodes, that start from zero once per launch.
	struct WaveKernel
	{
		void (*kernel)(GaLaunch);
		int maxN;
		bool general;
		uint64_t stateBytes;
		int sparseNodes;          // 0: the variant does not carry the sparse method
		bool clearSlotBySlot;     // the sparse tables are some 160 MB of a 360 MB slot: cleared slot by slot, and without them cleared nothing is launched
	};
	// the slots of ga_wide_sparse_kernel are some 360 MB each (arena for 2^20-column slices, 2^23 queue entries): a fallback for a few
	// jobs, capped so that a batch of many such jobs does not claim the whole device for it
	static constexpr uint32_t kWideSparseSlots = 32;
	// the scratch slot of each wave-per-read rung, in the order of gald::kRungs
	struct WaveGeom
	{
		uint32_t capCols;
		uint64_t arenaWordsPerSlice;
		uint32_t traceMul, wavesPerCu;
		uint64_t arenaWordsExtra;
		uint32_t slotCap;         // 0: as many slots as fit
	};
	static constexpr WaveGeom kWaveGeom[] = {
		// <GA_FIRST_N,false>: the lean variant over everything (32 band nodes in LDS, 24 waves per CU)
		{4096, 3 * 64 + 5 * 800, 2, 24, 0, 0},
		// <64,false>: 64 band nodes in LDS
		{8192, 3 * 64 + 5 * 2048, 3, 12, 0, 0},
		// <64,true>, <256,true>: the general variants, which also carry the paths for bands with cycles and for ramp redos; 256 band
		// nodes with large buffers
		{8192, 3 * 64 + 5 * 4096, 4, 8, 0, 0},
		{65536, 3 * 256 + 5 * 8192, 6, 4, 0, 0},
		// <4096,true>: bit-vector bands of more than 256 nodes (tangles of short nodes, wide bubbles, fans): 4 096 band nodes with the
		// tables in HBM, one wave per CU.  A bit-vector band has at most 199 999 columns.  Arena per slice: the node table of 4 096 nodes
		// and 32 768 columns -- four times the figure of the pass before for sixteen times its nodes, because what overflows 256 band
		// nodes is short nodes (the passes before allow 32 columns per table node; 8 per node here), and few slices of a job are that
		// wide.  A job that needs more reports GA_CAP_ARENA and goes on to the next pass like every other capacity miss.
		{kCutoffCols, 3 * (uint64_t)kWideNodes + 5 * 32768, 8, 1, 0, 0},
		// <256,true,true>: bands of 200 000 cells and more (the reference's sparse method and backtrace override, ga_sparse.h), with room
		// for every column of every node such a slice touches: 2^20 columns
		{1u << 20, 3 * 256 + 5 * 20000, 8, 1, 48ull << 20, 0},
		// <4096,true,true>: such bands with more than 256 nodes (fans and tangles of hundreds to thousands of nodes): the same with
		// 4 096 band nodes, the state in HBM and tables sized for it.  Arena as above.  No such job, no launch.
		{1u << 20, 3 * (uint64_t)kWideNodes + 5 * 20000, 8, 1, 48ull << 20, kWideSparseSlots},
	};
	static_assert(sizeof(kWaveGeom) / sizeof(kWaveGeom[0]) == sizeof(gald::kRungs) / sizeof(gald::kRungs[0]), "one scratch geometry per wave-per-read rung");

	// one launch of a wave-per-read kernel over `again` (job indices, longest first)
	int wavePass(const WaveKernel& k, const WaveGeom& geo, const std::vector<uint32_t>& again)
	{
		if (ensureRows()) return GA_E_DEVICE;
		GaLaunch Rl = L;
		const uint32_t maxRows = longestJob(again);
		Rl.cap_cols = geo.capCols;
		Rl.trace_cap = maxRows * geo.traceMul + 4096;
		Rl.max_slices = std::max<uint32_t>(maxRows / 64, 1);
		Rl.arena_words = std::min<uint64_t>(64 + (uint64_t)(maxRows / 64) * (gak::kSliceHdrWords + geo.arenaWordsPerSlice) + geo.arenaWordsExtra, 0xfffffff0ull);
		Rl.sparse_bw = k.sparseNodes ? (uint32_t)std::max(std::max(L.initial_bw, L.ramp_bw), 1) : 0u;
		const SlotLayout lay = slotLayout(Rl.cap_cols, Rl.max_slices, Rl.arena_words, Rl.trace_cap, Rl.sparse_bw, k.stateBytes, k.maxN);
		const uint64_t sparseBytes = k.sparseNodes ? sparseTableBytes(k.sparseNodes, Rl.sparse_bw) : 0;
		Rl.slot_bytes = lay.bytes;
		const uint64_t fit = scratchBudget() / lay.bytes;
		uint32_t rslots = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>((uint64_t)g->cus * geo.wavesPerCu, fit), again.size()));
		if (geo.slotCap) rslots = std::min(rslots, geo.slotCap);
		if (knobs.waveSlots) rslots = std::min(rslots, knobs.waveSlots);
		Rl.job_list = dList;
		Rl.n_jobs = (uint32_t)again.size();
		const PassRun r = pass(again, (size_t)rslots * lay.bytes, [&](uint8_t* scratch) -> int {
			if (k.clearSlotBySlot)
			{
				for (uint32_t s = 0; s < rslots; s++)
					if (hipMemsetAsync(scratch + (uint64_t)s * lay.bytes + lay.sparse, 0, sparseBytes, stream) != hipSuccess) return GA_E_DEVICE;
			}
			else if (k.sparseNodes) hipMemset2DAsync(scratch + lay.sparse, lay.bytes, 0, sparseBytes, rslots, stream);
			return 0;
		}, [&](uint8_t* scratch) {
			Rl.scratch = scratch;
			hipLaunchKernelGGL(k.kernel, dim3(rslots), dim3(64), 0, stream, Rl);
		});
		if (!r.ran) return r.rc;
		if (passNo == 1) { st.slots = rslots; st.waves_per_cu = geo.wavesPerCu; st.scratch_bytes = (uint64_t)rslots * lay.bytes; }
		if (knobs.debugPasses)
		{
			size_t capNodes = 0;
			for (uint32_t i : again) if (outs[i].status == GA_CAP_NODES) capNodes++;
			fprintf(stderr, "graphaligner_amd: wave-per-read pass <%d,%d%s>: %zu jobs on %u slots, %.2f ms, %zu left with GA_CAP_NODES\n", k.maxN, (int)k.general, k.sparseNodes ? ",sparse" : "", again.size(), rslots, r.ms, capNodes);
		}
		return r.rc;
	}

	// gald::climb's back end: the one place that names the kernels' template arguments
#ifndef GA_FIRST_N
#define GA_FIRST_N 32
#endif
	int launch(gald::Variant v, const std::vector<uint32_t>& list, bool first)
	{
		constexpr uint64_t kWideState = sizeof(gak::WaveState<kWideNodes>);
		static_assert(gak::Limits<kWideNodes>::kStateInHbm && !gak::Limits<256>::kStateInHbm, "two variants keep their state in HBM: <4096,true> and <4096,true,true>");
		const WaveGeom& geo = kWaveGeom[gald::isLanes(v) ? 0 : v - gald::kLean32];
		switch (v)
		{
		case gald::kLanes10: return lanesPass<10, 64>(list, kLanesRowsPerSlice[0], first);
		case gald::kLanes24: return lanesPass<24, 32>(list, kLanesRowsPerSlice[1], first);
		case gald::kLanes56: return lanesPass<56, 16>(list, kLanesRowsPerSlice[2], first);
		case gald::kLean32:
		{
			if (int rc = wavePass({ga_extend_kernel<GA_FIRST_N, false>, GA_FIRST_N, false, 0, 0, false}, geo, list)) return rc;
			st.main_ms = st.kernel_ms;
			st.main_variant = -GA_FIRST_N;                 // (negative: the wave-per-read kernel with that many band nodes in LDS)
			return 0;
		}
		case gald::kLean64: return wavePass({ga_extend_kernel<64, false>, 64, false, 0, 0, false}, geo, list);
		case gald::kGeneral64: return wavePass({ga_extend_kernel<64, true>, 64, true, 0, 0, false}, geo, list);
		case gald::kGeneral256: return wavePass({ga_extend_kernel<256, true>, 256, true, 0, 0, false}, geo, list);
		case gald::kWide: return wavePass({ga_wide_kernel, kWideNodes, true, kWideState, 0, false}, geo, list);
		case gald::kSparse256: return wavePass({ga_extend_kernel<256, true, true>, 256, true, 0, 256, false}, geo, list);
		case gald::kWideSparse: return wavePass({ga_wide_sparse_kernel, kWideNodes, true, kWideState, kWideNodes, true}, geo, list);
		default: return GA_E_INVALID;
		}
	}

	int runLadder()
	{
		HIP_OK(hipSetDevice(g->device));
		st = GaRunStats();
		passOf.assign(jobs.size(), 0);
		passNo = 0;
		if (jobs.empty()) return 0;
		// (the records are initialised on the device and come back whole after every pass: nothing to upload here; the host copy's
		// statuses are what the passes select their jobs by, so a batch that is run again starts from "not run" here too)
		for (auto& o : outs) o.status = GA_NOT_RUN;
		hipLaunchKernelGGL(ga_outs_init_kernel, dim3((uint32_t)((jobs.size() + 255) / 256)), dim3(256), 0, stream, L.outs, (uint32_t)jobs.size());
		HIP_OK(hipGetLastError());
		HIP_OK(hipMemsetAsync(L.trace_top, 0, 16, stream));
		// ---- the passes (ga_ladder.h): first the lanes = reads kernel, one job per lane, where the graph's shape makes its lockstep pay
		// -- its LDS tables hold 10, 24 or 56 band nodes per lane, the starting size follows the graph's mean node length, and jobs a
		// size cannot hold move to the next -- or the lean wave-per-read kernel; what is left climbs the wave-per-read rungs.
		// GA_LANES=1 / 0 forces which kernel goes first. ----
		const double meanNode = g->g.n_nodes > 2 ? (double)g->totalBp / (double)(g->g.n_nodes - 2) : 64.0;
		const int rc = gald::climb(orderHost, outs, passOf, passNo, st.jobs_retried, gald::firstPassFor(meanNode, knobs.lanes),
		                           [&](gald::Variant v, const std::vector<uint32_t>& list, bool first) { return launch(v, list, first); });
		for (int k = 0; k < 8; k++) { st.stamps[k] = 0; for (auto& o : outs) st.stamps[k] += o.stamps[k]; }
		return rc;
	}
};

}  // namespace
