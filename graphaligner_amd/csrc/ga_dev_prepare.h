// ga_dev_prepare.h -- the device batch's prepare: the stream, the reads and the jobs into device memory and the match words built from
// them (init, for ga_batch_prepare), or all of that from one upload with the seeds found and the jobs planned on the device
// (beginSeeded / finishSeeded, ga_plan.h); finish() is what both end in.
// Not a header for others: a part of ga_device.hip's translation unit (ga_dev.h).
#ifndef GA_DEVICE_PARTS
#error "ga_dev_prepare.h is a part of ga_device.hip"
#endif

namespace {

struct BatchPrepared : BatchCore
{
	using BatchCore::BatchCore;
	// what the prepare leaves in device memory for the stages after it
	const uint64_t* dEq = nullptr;     // the match words
	struct Resident
	{
		const uint8_t* seq = nullptr;   // the batch's copy of the reads and, per job, where its rows come from in it
		size_t seqBytes = 0;
		const GaEqFill* fills = nullptr;
		uint8_t* rows = nullptr;        // the row codes, when the match-word kernel wrote them
		uint8_t lut[256];               // the row codes of the read characters
	} res;
	std::vector<uint8_t> badFills;     // per fill of the GaEqSource: a row outside IUPAC
	GaRowsProvider rowsProvider;       // row codes for the wave-per-read kernels, uploaded when the first of them is about to run
	struct Seeded
	{
		uint8_t lut[768];               // row codes, row codes of the complement, "has a complement": lives as long as its upload may run
		Events<4> ev;                   // around seeding, plan and match words; destroyed when the prepare is done
	} seeded;
	const std::vector<uint8_t>* invalidFills() const override { return &badFills; }
	bool emittingRuns() const override { return cfg.emit_runs != 0; }
	void runsOffOnBadFills() { for (uint8_t f : badFills) if (f) { cfg.emit_runs = 0; break; } }

	// the stream and the events, before anything else
	int open()
	{
		HIP_OK(hipSetDevice(g->device));
		if (int s = stream.create()) return s;
		if (int s = evPass.create()) return s;
		memset(&L, 0, sizeof(L));
		L.graph = g->g;
		L.hmm = g->hmm;
		return 0;
	}
	// what every pass shares of the jobs and the configuration
	void setJobs(const std::vector<GaJob>& jobsIn)
	{
		jobs = jobsIn;
		L.n_jobs = (uint32_t)jobs.size();
		L.initial_bw = cfg.initial_bw;
		L.ramp_bw = cfg.ramp_bw;
		L.max_slices = std::max<uint32_t>(cfg.max_slices, 1);
	}

	int init(const uint64_t* eq, const GaEqSource* src, size_t eqWords, const std::vector<GaJob>& jobsIn)
	{
		if (int s = open()) return s;
		setJobs(jobsIn);
		GaJob* dJobs; uint64_t* eqDev;
		if (alloc(&eqDev, eqWords)) return GA_E_DEVICE;
		if (alloc(&dJobs, jobs.size())) return GA_E_DEVICE;
		if (!src && !eq) return GA_E_INVALID;
		if (src)
		{
			// the reads go up as they are (one transfer from the batch's pinned copy) and a kernel turns them into the match words
			uint8_t *dSeq, *dLut, *dFlags, *dRows; GaEqFill* dFills;
			const size_t rowBytes = (eqWords / 5) * 64 + 64;                         // (+ slack so a 64-byte row load never leaves the buffer)
			if (alloc(&dSeq, src->seqBytes + 64) || alloc(&dFills, src->nFills) || alloc(&dLut, 512) || alloc(&dFlags, src->nFills) || alloc(&dRows, rowBytes)) return GA_E_DEVICE;
			HIP_OK(hipMemsetAsync(dRows + rowBytes - 128, 0, 128, stream));
			res.rows = dRows;
			res.seq = dSeq; res.seqBytes = src->seqBytes; res.fills = dFills;
			if ((cfg.emit_ops || cfg.emit_pileup || cfg.emit_pathseq) && src->twin)
			{
				// (the twin table alone: a seeded prepare's dTwin serves as well)
				std::lock_guard<std::mutex> guard(g->twinLock);
				if (!g->dTwin && !g->dOpsTwin)
					if (int s = g->uploadOnce({{(void**)&g->dOpsTwin, src->twin, (size_t)g->g.n_nodes * 4}}, stream)) return s;
			}
			memcpy(res.lut, src->rowCode, 256);
			uint8_t lut[512];
			memcpy(lut, src->rowCode, 256); memcpy(lut + 256, src->rowCodeRc, 256);
			HIP_OK(hipMemcpyAsync(dSeq, src->seq, src->seqBytes, hipMemcpyHostToDevice, stream));
			HIP_OK(hipMemcpyAsync(dFills, src->fills, src->nFills * sizeof(GaEqFill), hipMemcpyHostToDevice, stream));
			HIP_OK(hipMemcpyAsync(dLut, lut, 512, hipMemcpyHostToDevice, stream));
			HIP_OK(hipMemsetAsync(eqDev + (eqWords - 5), 0, 40, stream));             // (the slack slice behind the last job)
			badFills.assign(src->nFills, 0);
			if (src->nFills)
			{
				const uint32_t waves = (uint32_t)std::min<size_t>(src->nFills, (size_t)g->cus * 64);
				hipLaunchKernelGGL(ga_eq_words_kernel, dim3(waves), dim3(64), 0, stream, dSeq, dFills, (uint32_t)src->nFills, dLut, (uint32_t)src->padCode, eqDev, dFlags, dRows);
				HIP_OK(hipGetLastError());
				HIP_OK(hipMemcpyAsync(badFills.data(), dFlags, src->nFills, hipMemcpyDeviceToHost, stream));
			}
			HIP_OK(hipStreamSynchronize(stream));                                      // (lut is on this stack; the flags decide emit_runs below)
			runsOffOnBadFills();
		}
		else HIP_OK(hipMemcpyAsync(eqDev, eq, eqWords * 8, hipMemcpyHostToDevice, stream));
		HIP_OK(hipMemcpyAsync(dJobs, jobs.data(), jobs.size() * sizeof(GaJob), hipMemcpyHostToDevice, stream));
		L.rows = nullptr;
		L.jobs = dJobs;
		dEq = eqDev;
		return finish();
	}

	// the hand-out order, the output records and the trace pool, from the host's copy of the jobs
	int finish()
	{
		// the device queues hand jobs out longest first: the short ones fill the tail of a launch, and the 64 jobs a lanes = reads
		// wave carries together have similar lengths
		orderHost.resize(jobs.size());
		for (uint32_t i = 0; i < jobs.size(); i++) orderHost[i] = i;
		std::stable_sort(orderHost.begin(), orderHost.end(), [&](uint32_t a, uint32_t b) { return jobs[a].n_rows > jobs[b].n_rows; });
		if (alloc(&dList, std::max<size_t>(jobs.size(), 1))) return GA_E_DEVICE;
		if (alloc(&L.outs, jobs.size())) return GA_E_DEVICE;
		// (the host copy of the records is page-locked: they come back after every pass, 128 bytes per job)
		outs.assign(jobs.size(), GaJobOut{});
		for (auto& o : outs) o.status = GA_NOT_RUN;
		outsLocked = !outs.empty() && hipHostRegister(outs.data(), outs.size() * sizeof(GaJobOut), hipHostRegisterDefault) == hipSuccess;
		if (alloc(&L.next_job, 4)) return GA_E_DEVICE;
		if (alloc(&L.trace_top, 2)) return GA_E_DEVICE;
		uint64_t totalRows = 0;
		for (auto& j : jobs) totalRows += j.n_rows;
		// one byte per move (a path makes at most ~1.5 moves per row), or 20 bytes per node run: room for a node change every 5 rows
		// (a job that does not fit reports GA_CAP_TRACE and is rerun by the ladder, which writes moves)
		L.trace_pool_cap = ((totalRows * (cfg.emit_runs ? 4 : 1) + totalRows / 2 + 256ull * jobs.size() + 4096) + 3) & ~3ull;
		// (test hook: a deliberately small pool, so that the claims' overflow path runs -- tests/parity_cases.py)
		if (knobs.tracePoolBytes) L.trace_pool_cap = knobs.tracePoolBytes;
		if (alloc(&L.traces, L.trace_pool_cap)) return GA_E_DEVICE;
		HIP_OK(hipStreamSynchronize(stream));
		return 0;
	}

	// ---- seeded batch (ga_plan.h): everything from the one upload of the reads to the one download of seeds and plan ----------------
	int beginSeeded(const GaSeededRequest& req, GaSeededPlan& plan)
	{
		if (int s = open()) return s;
		gasd::DevSeedEngine* eng = g->seed.get();
		if (!eng || !eng->built()) return GA_E_INVALID;
		const size_t nReads = req.nReads, nSlots = nReads * req.p.max_seeds, nJobsCap = 2 * nSlots;
		if (nSlots >= ((size_t)1 << 30)) return GA_E_INVALID;                  // (slot and job numbers are 32-bit)
		Events<4>& ev = seeded.ev;
		if (int s = ev.create()) return s;
		auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
		// what comes back in the one download
		const size_t oOutN = 0, oOutSeed = oOutN + up(nReads * 12), oOutLocus = oOutSeed + up(nSlots * 12), oOutNLoci = oOutLocus + (req.byLocus ? up(nSlots * 12) : 0);
		const size_t oTotals = oOutNLoci + (req.byLocus ? up(nReads * 4) : 0), oSeeds = oTotals + 256, oJobs = oSeeds + up(nSlots * sizeof(GaPlanSeed));
		const size_t oFills = oJobs + up(nJobsCap * sizeof(GaJob)), oFillRead = oFills + up(nJobsCap * sizeof(GaEqFill)), oFlags = oFillRead + up(nJobsCap * 4);
		const size_t downBytes = oFlags + up(nJobsCap);
		// what stays: the reads' block, and the plan's work arrays
		const size_t oFirstBad = 0, oNBw = oFirstBad + up(nReads * 4), oNFw = oNBw + up((nSlots + 1) * 4), oSlotJobs = oNFw + up((nSlots + 1) * 4);
		const size_t oJobAt = oSlotJobs + up((nSlots + 1) * 4), oSlotRows = oJobAt + up((nSlots + 1) * 4), oRowsAt = oSlotRows + up((nSlots + 1) * 8);
		const size_t workBytes = oRowsAt + up((nSlots + 1) * 8);
		const size_t eqWords = (size_t)(req.rowsBound / 64 + 1) * 5, rowBytes = (size_t)req.rowsBound + 128;
		uint8_t *dIn, *dDown, *dWork, *dLut, *dRows; uint64_t* eqDev;
		if (alloc(&dIn, req.blockBytes + 64) || alloc(&dDown, downBytes) || alloc(&dWork, workBytes) || alloc(&dLut, 768) || alloc(&dRows, rowBytes) || alloc(&eqDev, eqWords)) return GA_E_DEVICE;
		{
			std::lock_guard<std::mutex> guard(g->twinLock);
			if (!g->dTwin)
				if (int s = g->uploadOnce({{(void**)&g->dTwin, req.twin, (size_t)g->g.n_nodes * 4}, {(void**)&g->dRev, req.rev, (size_t)g->g.n_nodes}}, stream)) return s;
		}
		memcpy(seeded.lut, req.rowCode, 256); memcpy(seeded.lut + 256, req.rowCodeRc, 256); memcpy(seeded.lut + 512, req.hasComplement, 256);
		// the one upload: reads, read records, hand-out order
		HIP_OK(hipMemcpyAsync(dIn, req.block, req.blockBytes, hipMemcpyHostToDevice, stream));
		HIP_OK(hipMemcpyAsync(dLut, seeded.lut, 768, hipMemcpyHostToDevice, stream));
		HIP_OK(hipMemsetAsync(dDown, 0, oTotals + 256, stream));                   // (the seeding kernel adds to cleared outputs)
		gap::PlanLaunch P;
		memset(&P, 0, sizeof(P));
		P.node_start = g->g.node_start; P.twin = g->dTwin; P.rev = g->dRev;
		P.n_nodes = g->g.n_nodes; P.n_reads = (uint32_t)nReads; P.max_seeds = req.p.max_seeds; P.overlap = req.overlap;
		P.seq = dIn; P.reads = (const gas::SeedRead*)(dIn + req.oRecs);
		P.out_n = (const uint32_t*)(dDown + oOutN); P.out_seed = (const uint32_t*)(dDown + oOutSeed);
		P.first_bad = (uint32_t*)(dWork + oFirstBad); P.n_bw = (uint32_t*)(dWork + oNBw); P.n_fw = (uint32_t*)(dWork + oNFw);
		P.slot_jobs = (uint32_t*)(dWork + oSlotJobs); P.job_at = (uint32_t*)(dWork + oJobAt); P.slot_rows = (uint64_t*)(dWork + oSlotRows); P.rows_at = (uint64_t*)(dWork + oRowsAt);
		P.seeds = (GaPlanSeed*)(dDown + oSeeds); P.jobs = (GaJob*)(dDown + oJobs); P.fills = (GaEqFill*)(dDown + oFills); P.fill_read = (uint32_t*)(dDown + oFillRead);
		P.totals = (uint64_t*)(dDown + oTotals); P.eq = eqDev; P.rows = dRows;
		Scan<uint32_t> jobAt{P.slot_jobs, P.job_at, nSlots + 1};
		Scan<uint64_t> rowsAt{P.slot_rows, P.rows_at, nSlots + 1};
		if (jobAt.size(stream) || rowsAt.size(stream)) return GA_E_DEVICE;
		uint8_t* dTmp;
		if (alloc(&dTmp, std::max(jobAt.tmpBytes, rowsAt.tmpBytes) + 16)) return GA_E_DEVICE;
		plan.keep = g->hostBlock(downBytes);
		if (!plan.keep) return GA_E_DEVICE;
		{
			// the engine's hit and label buffers are per graph: its lock is held until this stream has finished the seeding kernel
			std::lock_guard<std::mutex> guard(eng->lock);
			auto queue = [&]() -> int {
			HIP_OK(hipEventRecord(ev[0], stream));
			if (nReads)
			{
				if (int s = eng->launchResident(req.p, nReads, req.byLocus, dIn, P.reads, (const uint32_t*)(dIn + req.oOrder), (uint32_t*)(dDown + oOutN), (uint32_t*)(dDown + oOutSeed),
				                                (uint32_t*)(dDown + oOutLocus), (uint32_t*)(dDown + oOutNLoci), stream)) return s;
			}
			HIP_OK(hipEventRecord(ev[1], stream));
			if (nReads)
			{
				const uint32_t waves = (uint32_t)std::min<size_t>(nReads, (size_t)g->cus * 32);
				hipLaunchKernelGGL(ga_plan_first_bad_kernel, dim3(waves), dim3(64), 0, stream, P, (const uint8_t*)(dLut + 512));
			}
			const uint32_t slotBlocks = (uint32_t)((nSlots + 1 + 255) / 256);
			hipLaunchKernelGGL(ga_plan_slot_kernel, dim3(slotBlocks), dim3(256), 0, stream, P);
			if (jobAt.run(dTmp, stream) || rowsAt.run(dTmp, stream)) return GA_E_DEVICE;
			hipLaunchKernelGGL(ga_plan_write_kernel, dim3(slotBlocks), dim3(256), 0, stream, P);
			HIP_OK(hipEventRecord(ev[2], stream));
			// the match words from the fills as they lie in device memory
			if (nSlots)
			{
				const uint32_t waves = (uint32_t)std::min<size_t>(nJobsCap, (size_t)g->cus * 64);
				hipLaunchKernelGGL(ga_eq_words_planned_kernel, dim3(waves), dim3(64), 0, stream, (const uint8_t*)dIn, (const GaEqFill*)P.fills, (const uint64_t*)P.totals, (const uint8_t*)dLut,
				                   (uint32_t)req.padCode, eqDev, dDown + oFlags, dRows);
			}
			HIP_OK(hipGetLastError());
			HIP_OK(hipEventRecord(ev[3], stream));
			// the one download
			HIP_OK(hipMemcpyAsync(plan.keep.get(), dDown, downBytes, hipMemcpyDeviceToHost, stream));
			HIP_OK(hipEventSynchronize(ev[1]));
			return 0;
			};
			// (a failure after the first launch: nothing of this batch may still run when the lock goes and the caller frees the batch,
			// whose blocks and the graph's hit buffers the next prepare takes)
			if (int s = queue()) { hipStreamSynchronize(stream); return s; }
		}
		HIP_OK(hipStreamSynchronize(stream));
		// (the scans' arrays, their temporary storage and the tables serve the prepare only: back to the graph's block list now, and the
		// prepare's events with them)
		blocks.release(dWork); blocks.release(dTmp); blocks.release(dLut);
		float ms[3] = {0, 0, 0};
		for (int k = 0; k < 3; k++) if (int s = ev.elapsed(k, k + 1, ms[k])) return s;
		ev.destroy();
		const char* h = plan.keep.get();
		plan.outN = (const uint32_t*)(h + oOutN); plan.outSeed = (const uint32_t*)(h + oOutSeed);
		if (req.byLocus) { plan.outLocus = (const uint32_t*)(h + oOutLocus); plan.outNLoci = (const uint32_t*)(h + oOutNLoci); }
		plan.seeds = (const GaPlanSeed*)(h + oSeeds); plan.jobs = (const GaJob*)(h + oJobs); plan.fills = (const GaEqFill*)(h + oFills);
		plan.fillRead = (const uint32_t*)(h + oFillRead); plan.badFills = (const uint8_t*)(h + oFlags);
		const uint64_t* totals = (const uint64_t*)(h + oTotals);
		plan.nJobs = (size_t)totals[0]; plan.rowsTotal = totals[1];
		plan.seed_ms = ms[0]; plan.plan_ms = ms[1]; plan.eq_ms = ms[2];
		if (plan.nJobs > nJobsCap || plan.rowsTotal > req.rowsBound) return GA_E_DEVICE;
		badFills.assign(plan.badFills, plan.badFills + plan.nJobs);
		res.seq = dIn; res.seqBytes = req.blockBytes; res.fills = (const GaEqFill*)P.fills;
		memcpy(res.lut, req.rowCode, 256);
		res.rows = dRows;
		L.rows = nullptr;
		L.jobs = (const GaJob*)P.jobs;
		dEq = eqDev;
		return 0;
	}
	int finishSeeded(const std::vector<GaJob>& jobsIn, const GaRunConfig& c, GaRowsProvider rows, const uint64_t*, size_t) override
	{
		HIP_OK(hipSetDevice(g->device));
		cfg = c;
		rowsProvider = rows;
		setJobs(jobsIn);
		runsOffOnBadFills();
		return finish();
	}
};

}  // namespace
