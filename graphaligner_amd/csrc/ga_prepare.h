// ga_prepare.h -- reads into a batch of extension jobs: splitting reads at their seeds (GraphAligner.h:2969-3024), or taking over the
// plan the back end made for a seeded batch (ga_plan.h), the match words and row codes of the jobs' rows, and running the batch.
// Not a header for others: a part of ga_host.cpp's translation unit, included once at its end (as ga_device.hip includes the device
// programs), and a file of that name because the test build (tests/emul) compiles ga_host.cpp and tracks csrc/*.h.
#ifndef GA_HOST_PARTS
#error "ga_prepare.h is a part of ga_host.cpp"
#endif
#include <chrono>

#include "ga_host.h"

using namespace gahost;

typedef ga_batch::RowFill RowFill;

static uint64_t pad64(uint64_t n) { return (n + W - 1) / W * W; }
static double msBetween(std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }

// run `fn(fill, read sequence)` for every job's rows on the host threads
template <typename F> static void forEachFill(ga_batch* b, F fn)
{
	const auto& fills = b->fills;
	forChunks(fills.size(), 64, 64, evenPieces(fills.size()), [&](size_t lo, size_t hi, size_t) { for (size_t k = lo; k < hi; k++) fn(fills[k], b->seqs[fills[k].read]); });
}

// the row codes (one byte per padded read base: match set, exact-compare code, validity): only the wave-per-read kernels read them
static void buildRows(ga_batch* b)
{
	if (!b->rows.empty()) return;
	const CharTables& T = tables();
	b->rows.assign(b->rowsTotal + 64, 0);       // (+ slack so a 64-byte row load never leaves the buffer)
	forEachFill(b, [&](const RowFill& f, const ReadSeq& seq) {
		const uint8_t padCode = T.rowCode[(uint8_t)'N'];
		uint8_t* dst = b->rows.data() + f.off;
		if (f.backward) for (uint64_t r = 0; r < f.n; r++) dst[r] = T.rowCode[T.complement[(uint8_t)seq[f.n - 1 - r]]];
		else for (uint64_t r = 0; r < f.n; r++) dst[r] = T.rowCode[(uint8_t)seq[f.pos + r]];
		for (uint64_t r = f.n; r < f.padded; r++) dst[r] = padCode;
	});
}

static void noteInvalidFill(ga_batch* b, size_t read)
{
	b->anyInvalidRow.store(1, std::memory_order_relaxed);
	b->readInvalid[read].store(1, std::memory_order_relaxed);
}

// the match words built on the host, for a back end that wants them finished (the host emulations of tests/)
static void buildHostWords(ga_batch* b)
{
	const CharTables& T = tables();
	b->eq.reset(new uint64_t[b->eqWords]);
	for (int k = 0; k < 5; k++) b->eq[b->eqWords - 5 + k] = 0;              // (the slack slice behind the last job)
	forEachFill(b, [&](const RowFill& f, const ReadSeq& seq) {
		// 64 row codes at a time, straight into the slice's match words
		const uint8_t padCode = T.rowCode[(uint8_t)'N'];
		const uint8_t* fw = (const uint8_t*)seq.data() + f.pos;
		const uint8_t* bw = (const uint8_t*)seq.data() + f.n - 1;
		uint8_t buf[W];
		for (uint64_t r0 = 0; r0 < f.padded; r0 += W)
		{
			const uint64_t full = r0 + W <= f.n ? (uint64_t)W : r0 < f.n ? f.n - r0 : 0;
			if (f.backward) for (uint64_t k = 0; k < full; k++) buf[k] = T.rowCodeRc[*(bw - (r0 + k))];
			else for (uint64_t k = 0; k < full; k++) buf[k] = T.rowCode[fw[r0 + k]];
			for (uint64_t k = full; k < (uint64_t)W; k++) buf[k] = padCode;
			uint64_t* words = b->eq.get() + (f.off + r0) / W * 5;
			ga_build_eq_words(buf, W, words);
			if (words[4] & 8u) noteInvalidFill(b, f.read);
		}
	});
}

static void decideRuns(ga_batch* b)
{
	const ga_graph* g = b->g;
	// Node runs instead of moves from the traceback when no result of the batch needs a cell list: no TraceItem lists wanted, every
	// read with one seed at its first base (one forward job: no backward part to mirror, no later seed to test against the cells
	// of an earlier one, GraphAligner.h:423-429), no character whose TraceItem the reference would assert on
	// ... and a graph of long nodes (the shape the lanes = reads kernel is the first pass for): a path then changes node every few
	// dozen rows and its runs are a fraction of its moves; on graphs chopped into short nodes moves are the smaller output
	const double meanNode = g->nodeCount() > 2 ? (double)g->bases.size() / (double)(g->nodeCount() - 2) : 64.0;
	// (with the words built by the back end, whether a row is such a character is known when the batch has been created: the back
	// end clears the flag then)
	bool runs = (b->flags & (GA_F_TRACE | GA_F_OPS | GA_F_PILEUP | GA_F_PATHSEQ)) == 0 && b->anyInvalidRow.load() == 0 && meanNode >= 40 && !(getenv("GA_RUNS") && atoi(getenv("GA_RUNS")) == 0);
	for (size_t i = 0; i < b->reads.size() && runs; i++) if (b->reads[i].nSeeds > 1) runs = false;
	for (const SeedPlan& sp : b->seeds) if (sp.bwJob >= 0 || (sp.fwJob >= 0 && sp.pos != 0)) { runs = false; break; }
	b->cfg.emit_runs = runs ? 1u : 0u;
	b->cfg.emit_ops = (b->flags & GA_F_OPS) ? 1u : 0u;
	b->cfg.emit_pileup = (b->flags & GA_F_PILEUP) ? 1u : 0u;
	b->cfg.emit_pathseq = (b->flags & GA_F_PATHSEQ) ? 1u : 0u;
}

// ---- what the two prepares share ---------------------------------------------------------------
static int entryStatus(const ga_graph_t* g, const ga_read_t* reads, size_t nReads, ga_batch_t** out, uint32_t flags)
{
	if (!g || !out || (!reads && nReads)) return GA_E_INVALID;
	if (!g->finalized) return GA_E_NOT_FINALIZED;
	if (!g->device) return GA_E_NO_DEVICE;
	if ((flags & GA_F_OPS) && !g->device->codesOps()) return GA_E_INVALID;
	if ((flags & GA_F_PILEUP) && !g->device->codesPileup()) return GA_E_INVALID;
	if ((flags & GA_F_PATHSEQ) && !g->device->writesPathSeq()) return GA_E_INVALID;
	return GA_S_OK;
}

static std::unique_ptr<ga_batch> newBatch(const ga_graph_t* g, size_t nReads, int initialBandwidth, int rampBandwidth, uint32_t flags)
{
	std::unique_ptr<ga_batch> b(new ga_batch());
	b->g = g;
	b->flags = flags;
	b->cfg.initial_bw = initialBandwidth;
	b->cfg.ramp_bw = rampBandwidth;
	b->reads.resize(nReads);
	b->names.resize(nReads);
	b->seqs.resize(nReads);
	return b;
}

// The batch keeps its own copy of the reads (the caller's buffers may go away before ga_batch_collect): ONE buffer (from the back end:
// the product hands out pinned blocks of a pool, so that the upload of the reads is one DMA transfer), so that the copy is a few large
// first-touch faults (huge pages where the system gives them) instead of one allocation per read, filled on the host threads
static bool readBlock(ga_batch* b, size_t bytes)
{
	b->seqBufBytes = bytes;
	b->seqKeep = b->g->device->hostBlock(bytes);
	b->seqBuf = b->seqKeep.get();
	return b->seqBuf != nullptr;
}

// read i to seqBuf + offsetOf(i); with padTo, zeros behind it up to the next multiple of padTo and padTo more (the seeder's layout)
template <typename OffsetOf> static void copyReads(ga_batch* b, const ga_read_t* reads, size_t nReads, OffsetOf offsetOf, size_t padTo)
{
	forChunks(nReads, 16, 256, evenPieces(nReads), [&](size_t lo, size_t hi, size_t) {
		for (size_t i = lo; i < hi; i++)
		{
			char* at = b->seqBuf + offsetOf(i);
			const size_t len = reads[i].length;
			if (len) memcpy(at, reads[i].sequence, len);
			if (padTo) memset(at + len, 0, (len + padTo - 1) / padTo * padTo + padTo - len);
			b->seqs[i] = ReadSeq(at, len);
			b->names[i] = reads[i].name ? reads[i].name : "";
		}
	});
}

// one extension job over n rows of `read` (its first pos + n bases mirrored, or its bases from pos on) and where its rows come from
static inline int64_t addJob(ga_batch* b, uint64_t& rowsTotal, size_t read, uint64_t n, uint32_t seedNode, uint32_t traceRows, uint64_t pos, bool backward)
{
	GaJob job;
	job.rows_off = rowsTotal;
	job.n_rows = (uint32_t)pad64(n);
	job.seed_node = seedNode;
	job.trace_rows = traceRows; job.reserved = 0;
	rowsTotal += job.n_rows;
	b->fills.push_back(RowFill{read, job.rows_off, n, job.n_rows, pos, backward});
	b->jobs.push_back(job);
	return (int64_t)b->jobs.size() - 1;
}

static void noteBadFills(ga_batch* b, const uint8_t* bad, size_t n)
{
	for (size_t k = 0; k < n && k < b->fills.size(); k++) if (bad[k]) noteInvalidFill(b, b->fills[k].read);
}

// Once jobs and fills stand: the limits of the run, the flags for characters outside IUPAC -- from the back end's list of bad fills
// where it has built the match words and knows already, from the host's own words where the back end wants them finished -- and
// whether the traceback may emit node runs
static void finishPlan(ga_batch* b, const uint8_t* badFills, bool hostWords)
{
	for (const GaJob& j : b->jobs)
	{
		b->cfg.max_rows = std::max(b->cfg.max_rows, j.n_rows);
		b->cfg.max_slices = std::max(b->cfg.max_slices, j.n_rows / W);
	}
	b->eqWords = (b->rowsTotal / W + 1) * 5;       // match words per slice for the lanes = reads kernel
	const size_t nReads = b->reads.size();
	b->readInvalid.reset(new std::atomic<uint8_t>[nReads + 1]);
	for (size_t i = 0; i <= nReads; i++) b->readInvalid[i].store(0, std::memory_order_relaxed);
	if (badFills) noteBadFills(b, badFills, b->fills.size());
	if (hostWords) buildHostWords(b);
	decideRuns(b);
}

// ... and once the back end's batch exists: the bad fills it has found by then, and whether its traceback does emit node runs
static void finishPlanOnDevice(ga_batch* b, const std::vector<uint8_t>* badFills)
{
	if (badFills) noteBadFills(b, badFills->data(), badFills->size());
	b->cfg.emit_runs = b->dev->emittingRuns() ? 1u : 0u;
}

// getSplitAlignment (GraphAligner.h:2969-3024): a seed of read i into its backward and its forward job.  (Run once per seed of the
// batch on one thread: the plan is written in place, the running row total and the tables stay with the caller's loop.)
static inline void planSeed(ga_batch* b, const CharTables& T, uint64_t& rowsTotal, size_t i, const ga_seed_t& seed, SeedPlan& sp)
{
	const ga_graph* g = b->g;
	const ReadSeq& seq = b->seqs[i];
	sp.pos = seed.read_pos;
	auto plain = g->lookup.find(seed.node_id * 2);
	auto flipped = g->lookup.find(seed.node_id * 2 + 1);
	if (plain == g->lookup.end() || flipped == g->lookup.end()) { sp.early = GA_S_BAD_SEED; return; }
	sp.seedNodeIndex = plain->second;
	sp.early = GA_S_ASSERTION;                  // (until the checks are through)
	if (!(sp.pos < seq.size())) return;
	const uint32_t fwNode = seed.reverse ? flipped->second : plain->second;
	const uint32_t bwNode = seed.reverse ? plain->second : flipped->second;
	if (g->nodeLen(fwNode) != g->nodeLen(bwNode)) return;
	if (sp.pos > 0)
	{
		if (seq.size() < sp.pos + (uint64_t)g->dbgOverlap) return;
		const uint64_t n = sp.pos + g->dbgOverlap;
		// ReverseComplement asserts on anything outside its table, eagerly over the whole prefix (CommonUtils.cpp:60-136)
		for (uint64_t r = 0; r < n; r++) if (!T.complement[(uint8_t)seq[r]]) return;
		sp.bwJob = addJob(b, rowsTotal, i, n, bwNode, (uint32_t)(n - g->dbgOverlap), 0, true);                           // trace_rows = sp.pos (:3069)
	}
	if (sp.pos < seq.size() - 1)
	{
		const uint64_t n = seq.size() - sp.pos;
		sp.fwJob = addJob(b, rowsTotal, i, n, fwNode, n >= (uint64_t)g->dbgOverlap ? (uint32_t)(n - g->dbgOverlap) : 0u, sp.pos, false);   // (:3051)
	}
	sp.valid = true;
	sp.early = GA_S_OK;
}

extern "C" {

int ga_batch_prepare(const ga_graph_t* g, const ga_read_t* reads, size_t nReads, const ga_seed_t* seeds, const size_t* seedOffsets,
                     int initialBandwidth, int rampBandwidth, uint32_t flags, ga_batch_t** out)
{
	if (!seedOffsets) return GA_E_INVALID;
	if (int s = entryStatus(g, reads, nReads, out, flags)) return s;
	const CharTables& T = tables();
	std::unique_ptr<ga_batch> owner = newBatch(g, nReads, initialBandwidth, rampBandwidth, flags);
	ga_batch* const b = owner.get();
	const auto tp0 = std::chrono::steady_clock::now();
	{
		std::vector<uint64_t> at(nReads + 1, 0);
		for (size_t i = 0; i < nReads; i++) at[i + 1] = at[i] + reads[i].length;
		// (no block is GA_E_INVALID here and GA_E_DEVICE in ga_batch_prepare_seeded: callers have seen either, so both stay)
		if (!readBlock(b, (size_t)at[nReads] + 64)) return GA_E_INVALID;
		copyReads(b, reads, nReads, [&](size_t i) { return at[i]; }, 0);
	}
	const auto tpc = std::chrono::steady_clock::now();
	// the jobs are planned first (sizes and offsets only); their match words are written afterwards by all host threads
	const size_t nSeeds = seedOffsets[nReads] - seedOffsets[0];
	b->seeds.reserve(nSeeds);
	b->jobs.reserve(2 * nSeeds);
	b->fills.reserve(2 * nSeeds);
	uint64_t rowsTotal = 0;
	for (size_t i = 0; i < nReads; i++)
	{
		b->reads[i].firstSeed = b->seeds.size();
		b->reads[i].nSeeds = seedOffsets[i + 1] - seedOffsets[i];
		for (size_t k = seedOffsets[i]; k < seedOffsets[i + 1]; k++) { b->seeds.emplace_back(); planSeed(b, T, rowsTotal, i, seeds[k], b->seeds.back()); }
	}
	b->rowsTotal = rowsTotal;
	const auto tp1 = std::chrono::steady_clock::now();
	// The product's back end builds the match words itself, by a kernel over the uploaded reads (the words are 0.6 bytes per base of
	// table look-ups and bit gathering: 26 ms on 16 host threads for the benchmark batch, nothing on the device); the host builder
	// is what the host emulation of tests/emul gets its words from.
	const bool deviceWords = g->device->buildsMatchWords();
	std::vector<GaEqFill> eqFills;
	if (deviceWords)
	{
		eqFills.resize(b->fills.size());
		for (size_t k = 0; k < b->fills.size(); k++)
		{
			const RowFill& f = b->fills[k];
			eqFills[k] = GaEqFill{(uint64_t)(b->seqs[f.read].data() - b->seqBuf), f.off / W, (uint32_t)f.pos, (uint32_t)f.n, (uint32_t)f.padded, f.backward ? 1u : 0u};
		}
	}
	finishPlan(b, nullptr, !deviceWords);
	int status = GA_S_OK;
	const auto tp2 = std::chrono::steady_clock::now();
	GaEqSource src;
	src.seq = b->seqBuf; src.seqBytes = b->seqBufBytes;
	src.fills = eqFills.data(); src.nFills = eqFills.size();
	src.rowCode = T.rowCode; src.rowCodeRc = T.rowCodeRc; src.padCode = T.rowCode[(uint8_t)'N'];
	src.twin = g->twin.data();
	b->dev = ga_backend_create_batch(g->device, [b]() -> const std::vector<uint8_t>& { buildRows(b); return b->rows; }, b->eq.get(), deviceWords ? &src : nullptr, b->eqWords,
	                                 b->jobs, b->cfg, &status);
	if (!b->dev) return status ? status : GA_E_DEVICE;
	finishPlanOnDevice(b, b->dev->invalidFills());
	if (getenv("GA_DEBUG_COLLECT"))
		fprintf(stderr, "graphaligner_amd: prepare: read copies %.1f ms, job plan %.1f ms, match words %.1f ms, device batch (alloc + upload) %.1f ms\n",
		        msBetween(tp0, tpc), msBetween(tpc, tp1), msBetween(tp1, tp2), msBetween(tp2, std::chrono::steady_clock::now()));
	*out = owner.release();
	return GA_S_OK;
}

// Seeds found and jobs planned on the back end's side (ga_plan.h): the host lays the reads out once, in the seeder's layout, and builds
// its own records from what comes back in one download -- by copying, with no lookup and no pass over the characters.
int ga_batch_prepare_seeded(const ga_graph_t* g, const ga_read_t* reads, size_t nReads, const ga_seed_params_t* params, int byLocus,
                            int initialBandwidth, int rampBandwidth, uint32_t flags, ga_batch_t** out)
{
	if (int s = entryStatus(g, reads, nReads, out, flags)) return s;
	GaSeedEngine* eng = g->device->seedEngine();
	if (!eng || !eng->built()) return GA_E_INVALID;
	GaSeedParams p{15, 2, 8, 4096, 1024, 64, 2, 2};                             // (ga_seed_params_default)
	if (params) p = GaSeedParams{params->k, params->sample_shift, params->max_occ, params->max_hits, params->window, params->diag_tol, params->min_support, params->max_seeds};
	if (!(p.k >= 11 && p.k <= 31 && p.sample_shift <= 8 && p.max_hits >= 1 && p.max_hits <= 65536 && p.max_seeds >= 1 && p.max_seeds <= 64)) return GA_E_INVALID;
	if (eng->info().k != p.k || eng->info().sample_shift != p.sample_shift) return GA_E_INVALID;
	for (size_t i = 0; i < nReads; i++) if ((reads[i].length && !reads[i].sequence) || reads[i].length > 0xfffffff0ull) return GA_E_INVALID;
	const CharTables& T = tables();
	const auto t0 = std::chrono::steady_clock::now();
	std::unique_ptr<ga_batch> owner = newBatch(g, nReads, initialBandwidth, rampBandwidth, flags);
	ga_batch* const b = owner.get();
	b->seeded = true; b->byLocus = byLocus != 0; b->seedParams = p;
	// the block: every read at a multiple of 16 with 16 bytes of padding behind it, then the read records (offset, length) and the reads'
	// numbers longest first, which is the order the seeding kernel hands them out in
	struct Rec { uint64_t off; uint32_t len, reserved; };
	std::vector<Rec> recs(nReads);
	uint64_t seqBytes = 0, rowsBound = 0;
	for (size_t i = 0; i < nReads; i++)
	{
		recs[i] = Rec{seqBytes, (uint32_t)reads[i].length, 0};
		seqBytes += ((reads[i].length + 15) & ~(size_t)15) + 16;
		// (a seed's two jobs have pad64(p + overlap) + pad64(length - p) rows)
		rowsBound += (uint64_t)p.max_seeds * ((reads[i].length + (uint64_t)g->dbgOverlap + 128 + 63) / 64 * 64);
	}
	std::vector<uint32_t> order(nReads);
	for (size_t i = 0; i < nReads; i++) order[i] = (uint32_t)i;
	std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return reads[x].length > reads[y].length; });
	auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
	GaSeededRequest req;
	req.seqBytes = (size_t)seqBytes; req.oRecs = up((size_t)seqBytes); req.oOrder = req.oRecs + up(nReads * sizeof(Rec)); req.blockBytes = req.oOrder + up(nReads * 4);
	if (!readBlock(b, req.blockBytes + 64)) return GA_E_DEVICE;           // (no memory: not a refusal of the call; see ga_batch_prepare)
	copyReads(b, reads, nReads, [&](size_t i) { return recs[i].off; }, 16);
	memset(b->seqBuf + seqBytes, 0, req.blockBytes - (size_t)seqBytes);
	if (nReads) { memcpy(b->seqBuf + req.oRecs, recs.data(), nReads * sizeof(Rec)); memcpy(b->seqBuf + req.oOrder, order.data(), nReads * 4); }
	uint8_t hasComplement[256];
	for (int c = 0; c < 256; c++) hasComplement[c] = T.complement[c] ? 1 : 0;
	req.block = b->seqBuf; req.nReads = nReads; req.p = p; req.byLocus = byLocus != 0; req.overlap = (uint32_t)g->dbgOverlap;
	req.twin = g->twin.data(); req.rev = g->idOdd.data(); req.hasComplement = hasComplement;
	req.rowCode = T.rowCode; req.rowCodeRc = T.rowCodeRc; req.padCode = T.rowCode[(uint8_t)'N']; req.rowsBound = rowsBound;
	const auto t1 = std::chrono::steady_clock::now();
	GaSeededPlan plan;
	int status = GA_S_OK;
	b->dev = g->device->beginSeededBatch(req, plan, &status);
	if (!b->dev) return status ? status : GA_E_DEVICE;
	const auto t2 = std::chrono::steady_clock::now();
	// the host's records, copied from the download
	const size_t nSlots = nReads * p.max_seeds;
	b->seedOutN.assign(plan.outN, plan.outN + nReads * 3);
	b->seedOut.assign(plan.outSeed, plan.outSeed + nSlots * 3);
	if (byLocus) { b->seedOutLocus.assign(plan.outLocus, plan.outLocus + nSlots * 3); b->seedNLoci.assign(plan.outNLoci, plan.outNLoci + nReads); }
	size_t nSeeds = 0;
	for (size_t i = 0; i < nReads; i++)
	{
		const uint32_t n = std::min(plan.outN[i * 3], p.max_seeds);
		b->reads[i].firstSeed = nSeeds;
		b->reads[i].nSeeds = n;
		nSeeds += n;
	}
	b->seeds.resize(nSeeds);
	for (size_t i = 0; i < nReads; i++)
		for (size_t t = 0; t < b->reads[i].nSeeds; t++)
		{
			const GaPlanSeed& ps = plan.seeds[i * p.max_seeds + t];
			SeedPlan& sp = b->seeds[b->reads[i].firstSeed + t];
			sp.valid = ps.valid != 0; sp.early = ps.early; sp.seedNodeIndex = ps.seed_node_index; sp.fwJob = ps.fw_job; sp.bwJob = ps.bw_job; sp.pos = ps.pos;
		}
	b->jobs.assign(plan.jobs, plan.jobs + plan.nJobs);
	b->fills.resize(plan.nJobs);
	for (size_t k = 0; k < plan.nJobs; k++)
	{
		const GaEqFill& f = plan.fills[k];
		b->fills[k] = RowFill{plan.fillRead[k], b->jobs[k].rows_off, f.n, f.padded, f.pos, f.backward != 0};
	}
	b->rowsTotal = plan.rowsTotal;
	finishPlan(b, plan.badFills, !plan.badFills);
	b->seedMs = plan.seed_ms; b->planMs = plan.plan_ms; b->eqMs = plan.eq_ms;
	plan.keep.reset();
	const auto t3 = std::chrono::steady_clock::now();
	status = b->dev->finishSeeded(b->jobs, b->cfg, [b]() -> const std::vector<uint8_t>& { buildRows(b); return b->rows; }, b->eq.get(), b->eqWords);
	if (status) return status;
	finishPlanOnDevice(b, nullptr);
	const auto t4 = std::chrono::steady_clock::now();
	b->hostMs = msBetween(t0, t4) - (b->seedMs + b->planMs + b->eqMs);
	if (getenv("GA_DEBUG_COLLECT"))
		fprintf(stderr, "graphaligner_amd: seeded prepare: read copies %.1f ms, upload + seeds + plan + match words + download %.1f ms (kernels %.1f + %.1f + %.1f), host records %.1f ms, device batch %.1f ms\n",
		        msBetween(t0, t1), msBetween(t1, t2), b->seedMs, b->planMs, b->eqMs, msBetween(t2, t3), msBetween(t3, t4));
	*out = owner.release();
	return GA_S_OK;
}

int ga_batch_prepare_stats(const ga_batch_t* b, ga_batch_prepare_stats_t* out)
{
	if (!b || !out || !b->seeded) return GA_E_INVALID;
	memset(out, 0, sizeof(*out));
	out->seed_kernel_ms = b->seedMs; out->plan_kernel_ms = b->planMs; out->eq_kernel_ms = b->eqMs; out->host_ms = b->hostMs;
	out->n_seeds = b->seeds.size(); out->n_jobs = b->jobs.size();
	for (const ReadPlan& r : b->reads) if (r.nSeeds == 0) out->reads_without_seed++;
	return GA_S_OK;
}

int ga_batch_plan_copy(const ga_batch_t* b, uint64_t* job_rows_off, uint32_t* job_n_rows, uint32_t* job_seed_node, uint32_t* job_trace_rows, size_t job_capacity,
                       uint64_t* seed_pos, uint32_t* seed_node_index, int32_t* seed_early, uint8_t* seed_valid, int64_t* seed_bw_job, int64_t* seed_fw_job, size_t seed_capacity,
                       uint64_t* fill_read, uint64_t* fill_off, uint64_t* fill_n, uint64_t* fill_padded, uint64_t* fill_pos, uint8_t* fill_backward, size_t fill_capacity,
                       size_t* counts)
{
	if (!b) return GA_E_INVALID;
	if (counts) { counts[0] = b->jobs.size(); counts[1] = b->seeds.size(); counts[2] = b->fills.size(); }
	for (size_t k = 0; k < std::min(job_capacity, b->jobs.size()); k++)
	{
		const GaJob& j = b->jobs[k];
		if (job_rows_off) job_rows_off[k] = j.rows_off;
		if (job_n_rows) job_n_rows[k] = j.n_rows;
		if (job_seed_node) job_seed_node[k] = j.seed_node;
		if (job_trace_rows) job_trace_rows[k] = j.trace_rows;
	}
	for (size_t k = 0; k < std::min(seed_capacity, b->seeds.size()); k++)
	{
		const SeedPlan& sp = b->seeds[k];
		if (seed_pos) seed_pos[k] = sp.pos;
		if (seed_node_index) seed_node_index[k] = sp.seedNodeIndex;
		if (seed_early) seed_early[k] = sp.early;
		if (seed_valid) seed_valid[k] = sp.valid ? 1 : 0;
		if (seed_bw_job) seed_bw_job[k] = sp.bwJob;
		if (seed_fw_job) seed_fw_job[k] = sp.fwJob;
	}
	for (size_t k = 0; k < std::min(fill_capacity, b->fills.size()); k++)
	{
		const RowFill& f = b->fills[k];
		if (fill_read) fill_read[k] = f.read;
		if (fill_off) fill_off[k] = f.off;
		if (fill_n) fill_n[k] = f.n;
		if (fill_padded) fill_padded[k] = f.padded;
		if (fill_pos) fill_pos[k] = f.pos;
		if (fill_backward) fill_backward[k] = f.backward ? 1 : 0;
	}
	return GA_S_OK;
}

int ga_batch_run(ga_batch_t* b)
{
	if (!b || !b->dev) return GA_E_INVALID;
	b->collected = false;                      // (the move bytes of the last collect are about to be overwritten)
	int s = b->dev->run();
	b->ran = s == GA_S_OK;
	return s;
}

static int runAndCollect(ga_batch_t* b, ga_results_t** out)
{
	int s = ga_batch_run(b);
	if (!s) s = ga_batch_collect(b, out);
	ga_batch_free(b);
	return s;
}

int ga_align_batch(const ga_graph_t* g, const ga_read_t* reads, size_t nReads, const ga_seed_t* seeds, const size_t* seedOffsets,
                   int initialBandwidth, int rampBandwidth, uint32_t flags, ga_results_t** out)
{
	ga_batch_t* b = nullptr;
	int s = ga_batch_prepare(g, reads, nReads, seeds, seedOffsets, initialBandwidth, rampBandwidth, flags, &b);
	return s ? s : runAndCollect(b, out);
}

int ga_align_reads(const ga_graph_t* g, const ga_read_t* reads, size_t nReads, const ga_seed_params_t* params, int byLocus,
                   int initialBandwidth, int rampBandwidth, uint32_t flags, ga_results_t** out)
{
	ga_batch_t* b = nullptr;
	int s = ga_batch_prepare_seeded(g, reads, nReads, params, byLocus, initialBandwidth, rampBandwidth, flags, &b);
	return s ? s : runAndCollect(b, out);
}

}  // extern "C"
