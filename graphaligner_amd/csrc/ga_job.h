// ga_job.h -- the whole job of the per-read extension program: run_job, from the seed state over the first pass (getSqrtSlices,
// GraphAligner.h:2571-2856), the wrongly aligned tail and the replay of the reference's checkpoints to the traceback, with the pieces of it
// that need none of the job's state as functions of their own.  Included by ga_kernel.h (namespace gak) after ga_sparse.h.
#pragma once

namespace gak {

// ---- the whole job --------------------------------------------------------------------------------------------
// Slice records carry everything needed to continue from them: the narrow variant only ever continues from
// the slice it has just finished; the wide variants also go back to an earlier one (the ramp redo of
// getSqrtSlices, GraphAligner.h:2648-2719) and re-run windows from checkpoints (getSlicesFromTable, :2858-2943)
// when a redo has left the reference's checkpoint list inconsistent with the slices it finally kept.
constexpr uint32_t kSeedRecord = 0xffffffffu;      // "record" of the initial slice (the seed node at score 0, j = -64)

// ---- pieces of the traceback that need none of the job's state ----
// A window = up to 64 consecutive columns of one node in one slice, one column per lane, so a
// run of steps inside a node costs no memory round trips: every lane evaluates its column
// at the wanted row (WordSlice.h:223-229) and the few values a step needs are read back.
struct Window { VU vp, vn; VI before; uint32_t slice, node; int lo, n; bool valid, present; };
GA_FN void load_window(Window& w, const SliceRec& rec, const uint32_t* tn, const uint32_t* tb, uint32_t recNodes, uint32_t sliceIdx, uint32_t n, uint32_t hiOffset)
{
	w.slice = sliceIdx; w.node = n;
	w.lo = hiOffset >= (uint32_t)(LANES - 1) ? (int)(hiOffset - (LANES - 1)) : 0;
	w.n = (int)hiOffset - w.lo + 1;
	int sl = find_slot(tn, (int)recNodes, n);
	w.present = sl >= 0;
	w.valid = true;
	if (sl >= 0)
	{
		uint32_t at = tb[sl] + (uint32_t)w.lo;
		w.vp = load_lanes_u64(rec.vp + at, w.n);
		w.vn = load_lanes_u64(rec.vn + at, w.n);
		w.before = load_lanes(rec.before + at, w.n, 0);
	}
}

template <int MAXN, bool GENERAL, bool SPARSE = false>
GA_FN void run_job(const GaLaunch& L, WaveState<MAXN>& ws, const Slot& slotIn, uint32_t jobIndex)
{
	constexpr bool kWide = GENERAL;             // cycles and ramp redos: compiled into the general variants only
	constexpr bool kSparse = SPARSE && GENERAL; // bands of >= 200 000 cells (sparse method, backtrace override): the last two variants of the ladder only
	const GaDevGraph& g = L.graph;
	const GaJob job = L.jobs[jobIndex];
	const GaHmmTables& hmm = *L.hmm;
	const uint8_t* rows = L.rows + job.rows_off;
	Slot slot = slotIn;
	GaJobOut out;
	out.status = GA_OK; out.score = 0x7fffffff; out.n_valid = 0; out.n_run = 0; out.trace_len = 0; out.max_band_nodes = 0; out.n_columns = 0; out.trace_off = 0;
	out.start_node = 0; out.start_offset = 0; out.start_row = 0; out.reserved2 = 0; out.n_node_steps = 0; out.reserved3 = 0;
	for (int i = 0; i < 8; i++) out.stamps[i] = 0;
	uint64_t tA = stamp(), tB;
#define GA_LAP(i) do { tB = stamp(); out.stamps[i] += tB - tA; tA = tB; } while (0)
	const uint32_t numSlices = job.n_rows / W;
	int status = GA_OK;

	// ---- the state a slice is computed from: previous band tables in LDS, packed end scores in end_prev ----
	int pn = 0;
	int prevMin = 0;
	double logCorrect = hmm.init_correct, logWrong = hmm.init_wrong;
	const uint32_t seedLen = g_len(g, job.seed_node);
	auto loadSeedState = [&]() {
		// initial slice: the whole seed node at score 0 (GraphAligner.h:2945-2960)
		wave_sync();
		if (GA_LANE0)
		{
			ws.pn_node[0] = job.seed_node; ws.pn_min[0] = 0; ws.pn_lastEnd[0] = 0; ws.pn_lastEnd2[0] = 0; ws.pn_colBase[0] = 0;
			ws.pn_len[0] = seedLen;
			ws.pn_outDeg[0] = 255;          // the seed node's out-list is read from HBM once
		}
		for (uint32_t c = 0; c < seedLen; c += LANES) store_lanes(slot.end_prev + c, (int)(seedLen - c), VI(4));      // score 0, scoreEndExists
		pn = 1; prevMin = 0; logCorrect = hmm.init_correct; logWrong = hmm.init_wrong;
		wave_sync();
	};
	auto loadRecordState = [&](uint32_t off) {
		// continue from a stored slice: what the reference keeps of it is its frozen end scores (NodeSlice.h:353-376)
		wave_sync();
		const uint32_t nN = slot.arena[off], nC = slot.arena[off + 1];
		const SliceRec r = slice_at(slot.arena, off, nN, nC);
		for (uint32_t q = 0; q < nN; q++)
		{
			const uint32_t base = r.colBase[q];
			const uint32_t next = q + 1 < nN ? r.colBase[q + 1] : nC;
			const uint32_t idx = next - 1;
			const uint64_t vp = r.vp[idx], vn = r.vn[idx];
			const int e = r.before[idx] + __builtin_popcountll(vp) - __builtin_popcountll(vn);
			if (GA_LANE0)
			{
				ws.pn_node[q] = r.nodes[q]; ws.pn_colBase[q] = base; ws.pn_len[q] = next - base; ws.pn_min[q] = r.nodeMin[q];
				ws.pn_lastEnd[q] = e; ws.pn_lastEnd2[q] = e - (int)(vp >> 63) + (int)(vn >> 63);
				ws.pn_outDeg[q] = 255;      // out-lists come from HBM
			}
		}
		// scoreEndExists: every column of a bit-vector slice; of a sparse-method slice (hdr[11] bit 0) only the columns whose last row was
		// written -- its untouched and partially confirmed columns have none (:2536), the frozen form keeps that bit (NodeSlice.h:370) and
		// the record keeps it as one byte per column behind `before` (sparse_materialize)
		const bool sparseRec = (r.hdr[11] & 1u) != 0;
		const uint8_t* exists = (const uint8_t*)(r.before + nC);
		for (uint32_t c = 0; c < nC; c += LANES)
		{
			const int k = (int)(nC - c);
			const VU vpV = load_lanes_u64(r.vp + c, k), vnV = load_lanes_u64(r.vn + c, k);
			const VI endV = load_lanes(r.before + c, k, 0) + vpopc(vpV) - vpopc(vnV);
			const VI existsV = sparseRec ? (load_lanes(exists + c, k, 0) << 2) : VI(4);
			store_lanes(slot.end_prev + c, k, (endV << 3) | existsV | vpopc(vpV & VU(1ull << 63)) | (vpopc(vnV & VU(1ull << 63)) << 1));
		}
		pn = (int)nN; prevMin = (int)r.hdr[2];
		union { double d; uint32_t w[2]; } a, b;
		a.w[0] = r.hdr[6]; a.w[1] = r.hdr[7]; b.w[0] = r.hdr[8]; b.w[1] = r.hdr[9];
		logCorrect = a.d; logWrong = b.d;
		wave_sync();
	};

	// a seed node of >= 200 000 bp is the whole band of the second slice: the reference goes sparse there (GraphAligner.h:2483)
	// (with the sparse method compiled in: slice 0 of such a seed runs at the ramp width, :2612; without one that is a bandwidth of 0 and
	// undefined behaviour in the reference, reported as an assertion; with one, every column of the seed node is a cell of row 0 --
	// more than this program's tables hold, reported as a capacity miss)
	if (seedLen >= kCutoff) status = kSparse ? (L.ramp_bw < 1 ? GA_ASSERTION : GA_CAP_COLS) : GA_UNSUPPORTED_BAND;
	else if (seedLen > L.cap_cols) status = GA_CAP_COLS;
	if (status == GA_OK) loadSeedState();
	VI rowNext = load_lanes(rows, W, 0);
	uint32_t rowNextSlice = 0;
	int rowAboveKept = 0;                      // code of the last row of slice rowAboveFor - 1
	uint32_t rowAboveFor = 0;
	uint64_t arenaTop = 0;
	uint32_t nPushed = 0;          // bandwidthPerSlice.size()
	uint32_t nRun = 0;
	const bool rampPossible = L.ramp_bw > L.initial_bw;

	// ---- one slice from the loaded state: band, order, fill; the record is written at arenaTop (not yet claimed) ----
	int cn = 0, sliceMin = 0;
	uint64_t need = 0;
	// what the slice just computed was: its cells (DPSlice::numCells) and, for a slice of the sparse method, what its frozen forms could not hold
	uint32_t freshCells = 0;
	bool freshSparse = false, freshEndsTooFar = false, freshBeforeTooFar = false;
	auto runSlice = [&](uint32_t slice, int bandwidth) -> int {
		uint32_t totalCols = 0;
		cn = 0;
		freshSparse = false; freshEndsTooFar = false; freshBeforeTooFar = false;
		GA_LAP(0);
		int st = project_band(g, ws, pn, prevMin, bandwidth, cn, totalCols);
		GA_LAP(1);
		if constexpr (kSparse)
		{
			if (st == GA_UNSUPPORTED_BAND)
			{
				// ---- the band has 200 000 cells or more: the sparse method (pickMethodAndExtendFill, :2499-2520) ----
				wave_sync();
				if ((uint32_t)bandwidth > slot.sparse_max_bw) return GA_CAP_HEAP;
				const SparseMem sm = sparse_mem_at<MAXN>(slot.sparse, slot.sparse_max_bw);
				const SparseResult sr = sparse_fill(g, ws, slot, sm, rows + (uint64_t)slice * W, job.n_rows, slice * W, pn, prevMin, bandwidth, cn);
				rowNextSlice = 0xffffffffu;                                           // (the row codes were not taken from the prefetch)
				if (sr.status != GA_OK) return sr.status;
				if (sr.oddWord) return GA_CAP_COLS;                                   // (see SparseResult::oddWord: reported, never a different answer)
				if (sr.minScore < prevMin) return GA_ASSERTION;                      // :2508
				sliceMin = sr.minScore;
				freshSparse = true; freshEndsTooFar = sr.endsTooFar; freshBeforeTooFar = sr.beforeTooFar;
				freshCells = sr.numCells;
				out.n_columns += sr.numCells;
				out.max_band_nodes = out.max_band_nodes > (uint32_t)cn ? out.max_band_nodes : (uint32_t)cn;
				need = 0;
				if (sr.endsTooFar) return GA_OK;                                      // the slice cannot outlive this iteration (see the loop): no record
				if (sr.numCells > L.cap_cols) return GA_CAP_COLS;
				need = slice_words((uint32_t)cn, sr.numCells) + (sr.numCells + 3) / 4;
				if (arenaTop + need > L.arena_words || arenaTop + need >= 0xffffffffull) return GA_CAP_ARENA;
				SliceRec rec = slice_at(slot.arena, arenaTop, (uint32_t)cn, sr.numCells);
				sparse_materialize(g, ws, slot, sm, rec, (uint8_t*)(rec.before + sr.numCells), cn, sr.nWords, bandwidth);
				if (GA_LANE0)
				{
					rec.hdr[0] = (uint32_t)cn; rec.hdr[1] = sr.numCells; rec.hdr[2] = (uint32_t)sliceMin; rec.hdr[3] = (uint32_t)sr.minSlot; rec.hdr[4] = sr.minOffset; rec.hdr[5] = 0;
					rec.hdr[11] = 1u | (sr.beforeTooFar ? 2u : 0u);
				}
				return GA_OK;
			}
		}
		// (in the variants of the last two passes a projection heap that overflows is reported as what it is there, band tables too small
		// for the band: the pass with 4 096 band nodes takes GA_CAP_NODES and leaves GA_CAP_HEAP, which the sparse method's own tables report)
		if constexpr (kSparse) { if (st == GA_CAP_HEAP) st = GA_CAP_NODES; }
		if (st != GA_OK) return st;
		freshCells = totalCols;
		if (totalCols > L.cap_cols) return GA_CAP_COLS;
		ws_order<MAXN>();
		load_topology(g, ws, pn, cn);
		ws_order<MAXN>();
		// this slice's row codes normally arrived during the previous slice; request the next slice's now
		if (rowNextSlice != slice) rowNext = load_lanes(rows + (uint64_t)slice * W, W, 0);
		const VI rowCode = rowNext;
		const int rowAboveCode = rowAboveFor == slice ? rowAboveKept : (slice > 0 ? (int)rows[(uint64_t)slice * W - 1] : 0);
		rowAboveKept = read_lane(rowCode, W - 1);
		rowAboveFor = slice + 1;
		if (slice + 1 < numSlices) { rowNext = load_lanes(rows + (uint64_t)(slice + 1) * W, W, 0); rowNextSlice = slice + 1; }
		GA_LAP(2);
		st = processing_order(g, ws, cn);
		int nComps = 0;
		bool cyclicBand = false;
		if constexpr (kWide)
		{
			// a band with a cycle is filled by the confirmation-tracking path (wide kernel variants only; the
			// narrow variant reports GA_UNSUPPORTED_CYCLE and the job is rerun by a wide one)
			if (st == GA_UNSUPPORTED_CYCLE) { ws_order<MAXN>(); st = scc_order(g, ws, cn, nComps); cyclicBand = true; }
		}
		GA_LAP(3);
		if (st != GA_OK) return st;
		need = slice_words((uint32_t)cn, totalCols);
		if (arenaTop + need > L.arena_words) return GA_CAP_ARENA;
		if (arenaTop + need >= 0xffffffffull) return GA_CAP_ARENA;
		SliceRec rec = slice_at(slot.arena, arenaTop, (uint32_t)cn, totalCols);
		for (int c = 0; c < cn; c += LANES)
		{
			store_lanes(rec.nodes + c, cn - c, load_lanes(ws.cn_node + c, cn - c, 0));
			store_lanes(rec.colBase + c, cn - c, load_lanes(ws.cn_colBase + c, cn - c, 0));
		}
		ws_order<MAXN>();
		int minSlot;
		uint32_t minOffset;
		GA_LAP(0);
		if constexpr (kWide)
		{
			if (cyclicBand) st = fill_slice_general(g, ws, slot, rec, rowCode, rowAboveCode, job.n_rows, slice * W, prevMin, pn, cn, nComps, sliceMin, minSlot, minOffset);
			else st = fill_slice(g, ws, slot, rec, rowCode, rowAboveCode, job.n_rows, slice * W, pn, cn, sliceMin, minSlot, minOffset);
		}
		else st = fill_slice(g, ws, slot, rec, rowCode, rowAboveCode, job.n_rows, slice * W, pn, cn, sliceMin, minSlot, minOffset);
		GA_LAP(4);
		if (st != GA_OK) return st;
		if (sliceMin < prevMin) return GA_ASSERTION;                              // :2469
		ws_order<MAXN>();
		for (int c = 0; c < cn; c += LANES) store_lanes(rec.nodeMin + c, cn - c, load_lanes(ws.cn_min + c, cn - c, 0));
		if (GA_LANE0)
		{
			rec.hdr[0] = (uint32_t)cn; rec.hdr[1] = totalCols; rec.hdr[2] = (uint32_t)sliceMin; rec.hdr[3] = (uint32_t)minSlot; rec.hdr[4] = minOffset; rec.hdr[5] = 0;
			rec.hdr[11] = 0;
		}
		out.n_columns += totalCols;
		out.max_band_nodes = out.max_band_nodes > (uint32_t)cn ? out.max_band_nodes : (uint32_t)cn;
		return GA_OK;
	};
	// the slice just computed becomes the state
	auto adoptSlice = [&]() {
		ws_order<MAXN>();
		for (int c = 0; c < cn; c += LANES)
		{
			int k = cn - c;
			store_lanes(ws.pn_node + c, k, load_lanes(ws.cn_node + c, k, 0));
			store_lanes(ws.pn_min + c, k, load_lanes(ws.cn_min + c, k, 0));
			store_lanes(ws.pn_lastEnd + c, k, load_lanes(ws.cn_lastEnd + c, k, 0));
			store_lanes(ws.pn_lastEnd2 + c, k, load_lanes(ws.cn_lastEnd2 + c, k, 0));
			store_lanes(ws.pn_colBase + c, k, load_lanes(ws.cn_colBase + c, k, 0));
			store_lanes(ws.pn_len + c, k, load_lanes(ws.cn_len + c, k, 0));
			store_lanes(ws.pn_outDeg + c, k, load_lanes(ws.cn_outDeg + c, k, 0));
		}
		for (int c = 0; c < cn * kNbr; c += LANES) store_lanes(ws.pn_outNbr + c, cn * kNbr - c, load_lanes(ws.cn_outNbr + c, cn * kNbr - c, 0));
		pn = cn;
		prevMin = sliceMin;
		uint32_t* t = slot.end_prev; slot.end_prev = slot.end_cur; slot.end_cur = t;
		wave_sync();
	};

	// ---- first pass (getSqrtSlices, GraphAligner.h:2571-2856) ----
	// checkpoint bookkeeping of the reference, needed only to reproduce what a ramp redo does to it
	uint32_t sampling = 0;
	while ((sampling + 1) * (sampling + 1) <= numSlices) sampling++;            // (int)sqrt(len / 64) (:2962-2967)
	uint32_t lastRec = kSeedRecord, rampRec = kSeedRecord, storeRec = kSeedRecord;
	uint32_t storeMem = 28, rampUntil = 0, rampRedoIndex = 0xffffffffu, nCkpt = 0;
	bool redone = false;
	auto recSlice = [&](uint32_t recOff) -> uint32_t { return recOff == kSeedRecord ? 0xffffffffu : slot.arena[recOff + 10]; };   // slice index of a record (-1 for the seed)
	// DPSlice::j as the reference compares it: unsigned, the seed slice's -64 is the largest value there is
	auto recJ = [&](uint32_t recOff) -> uint64_t { return recOff == kSeedRecord ? ~0ull - 63 : (uint64_t)slot.arena[recOff + 10] * W; };
	// backtrace-override bookkeeping of getSqrtSlices (:2604-2606, 2721-2764, 2810-2825): the open window = slices ovFirst .. ovFirst + ovCount - 1
	uint32_t lastNumCells = 0, ovPreRec = kSeedRecord, ovFirst = 0, ovCount = 0, nOv = 0;
	bool overriding = false, anyOverride = false;
	(void)recJ; (void)ovPreRec; (void)ovFirst; (void)ovCount; (void)nOv; (void)overriding; (void)anyOverride; (void)lastNumCells;
	// what building the override of the open window checks (ga_sparse.h), then the window joins the list and the checkpoints inside it go
	auto closeWindow = [&]() -> int {
		if constexpr (kSparse)
		{
			if (ovCount == 0 || lastRec == kSeedRecord || recSlice(lastRec) != ovFirst + ovCount - 1) return GA_ASSERTION;   // assert(lastSlice.j == backtraceOverrideTemps.back().j)
			wave_sync();
			const SparseMem sm = sparse_mem_at<MAXN>(slot.sparse, slot.sparse_max_bw);
			const int st = explore_override(g, ws, slot, sm, slot.slice_off, ovFirst, ovCount, ovPreRec == kSeedRecord ? 0u : ovPreRec, ovPreRec == kSeedRecord,
			                                job.seed_node, rows, (int)job.n_rows);
			if (st != GA_OK) return st;
			if (GA_LANE0) { slot.ovr[2 * nOv] = ovFirst; slot.ovr[2 * nOv + 1] = ovFirst + ovCount - 1; }
			nOv++;
			anyOverride = true;
			overriding = false;
			const uint64_t startj = (uint64_t)ovFirst * W, endj = (uint64_t)(ovFirst + ovCount - 1) * W;
			while (nCkpt > 0 && recJ(slot.ckpt[nCkpt - 1]) >= startj && recJ(slot.ckpt[nCkpt - 1]) <= endj) nCkpt--;
			ovCount = 0;
			wave_sync();
		}
		return GA_OK;
	};
	for (uint32_t slice = 0; slice < numSlices && status == GA_OK; slice++)
	{
		// slice 0 always runs at the ramp width because rampUntil(0) >= slice(0) (:2603,2612)
		const bool useRamp = rampUntil >= slice;
		const int bandwidth = useRamp ? L.ramp_bw : L.initial_bw;
		status = runSlice(slice, bandwidth);
		if (status != GA_OK) break;
		const uint32_t thisRec = (uint32_t)arenaTop;
		nRun++;
		// ---- HMM step (AlignmentCorrectnessEstimation.cpp:71-89): additions and comparisons only ----
		int mism = sliceMin - prevMin;
		if (mism > 64) { status = GA_ASSERTION; break; }
		double cc = logCorrect + hmm.c2c, fc = logWrong + hmm.f2c, cf = logCorrect + hmm.c2f, ff = logWrong + hmm.f2f;
		bool correctFromCorrect = cc >= fc;
		bool falseFromCorrect = cf >= ff;
		const double newCorrect = (cc > fc ? cc : fc) + hmm.correct_mult[mism];
		const double newWrong = (cf > ff ? cf : ff) + hmm.wrong_mult[mism];
		bool currentlyCorrect = newCorrect > newWrong;
		if constexpr (kSparse) { if (rampUntil == slice && freshCells >= kCutoff) rampUntil++; }      // :2626-2629
		if constexpr (kWide)
		{
			if (rampPossible && ((slice > 0 && rampUntil == slice - 1) || (rampUntil < slice && currentlyCorrect && falseFromCorrect)) && (!kSparse || lastNumCells < kCutoff))
			{
				rampRec = lastRec;                                               // :2630-2634
				rampRedoIndex = slice - 1;
			}
		}
		if (!correctFromCorrect) break;                                          // :2640-2647 (this slice is not kept)
		if (!currentlyCorrect && rampUntil < slice && rampPossible)
		{
			if constexpr (!kWide) { status = GA_UNSUPPORTED_RAMP; break; }       // rerun by a wide variant
			else
			{
				// ---- go back to the remembered slice and come forward again at the ramp width (:2648-2719) ----
				rampUntil = slice;
				const uint32_t back = rampRedoIndex;
				rampRedoIndex = slice;
				const uint32_t backRec = rampRec;
				rampRec = lastRec;
				lastRec = backRec;
				if (backRec == kSeedRecord) loadSeedState(); else loadRecordState(backRec);
				nPushed = back + 1;                                              // bandwidthPerSlice / correctness shrink to back + 1 entries
				while (nCkpt > 1 && slot.ckpt[nCkpt - 1] != kSeedRecord && recSlice(slot.ckpt[nCkpt - 1]) > back) nCkpt--;
				if constexpr (kSparse)
				{
					lastNumCells = backRec == kSeedRecord ? 0u : slot.arena[backRec + 1];
					if (overriding)                                              // :2673-2700
					{
						if (recJ(ovPreRec) > recJ(lastRec)) { overriding = false; ovCount = 0; }
						// "shorten": the reference swaps an empty slice (j = SIZE_MAX) into the back of its list, does not pop it and tests the
						// back's j again -- once entered, that loop never ends (:2690-2694).  Reported as an assertion.
						else if (ovCount > 0 && (uint64_t)(ovFirst + ovCount - 1) * W > recJ(lastRec)) { status = GA_ASSERTION; break; }
					}
					while (nOv > 0 && (uint64_t)slot.ovr[2 * (nOv - 1) + 1] * W > recJ(lastRec)) nOv--;
				}
				redone = true;
				slice = back;                                                    // the loop increment makes it back + 1
				continue;
			}
		}
		const uint32_t thisMem = freshCells * 4 + (uint32_t)cn * 28;             // estimatedMemory (:136-139)
		bool closedWindow = false;
		if constexpr (kSparse)
		{
			// ---- the slice is kept: what the reference now freezes of it, and the override window it opens, extends or closes (:2721-2764) ----
			bool pushTemps = false, closing = false;
			if (!overriding && freshCells >= kCutoff && lastNumCells < kCutoff) { ovPreRec = lastRec; overriding = true; ovFirst = slice; ovCount = 0; pushTemps = true; }
			else if (overriding) { if (freshCells < kCutoff) closing = true; else pushTemps = true; }
			// lastSlice = newSlice.getFrozenSqrtEndScores() always follows (:2805), getFrozenScores for a window's list (:2729, 2762): both assert
			// that the slice's scores lie within 16 bits of their minimum (NodeSlice.h:344, 372) -- which a long node's untouched columns break
			if (freshSparse && (freshEndsTooFar || (pushTemps && freshBeforeTooFar))) { status = GA_ASSERTION; break; }
			if (closing)
			{
				status = closeWindow();
				if (status != GA_OK) break;
				if (GA_LANE0) slot.ckpt[nCkpt] = lastRec;                        // result.slices.push_back(lastSlice) (:2752)
				nCkpt++;
				closedWindow = true;
				ws_order<MAXN>();
			}
			if (pushTemps) ovCount++;
		}
		if (GA_LANE0)
		{
			uint32_t* hdr = slot.arena + arenaTop;
			union { double d; uint32_t w[2]; } a, b;
			a.d = newCorrect; b.d = newWrong;
			hdr[5] = (uint32_t)((currentlyCorrect ? 1 : 0) | (falseFromCorrect ? 2 : 0) | (useRamp ? 4 : 0));
			hdr[6] = a.w[0]; hdr[7] = a.w[1]; hdr[8] = b.w[0]; hdr[9] = b.w[1]; hdr[10] = slice;
			slot.slice_off[slice] = thisRec;
			slot.slice_flags[slice] = (uint8_t)((currentlyCorrect ? 1 : 0) | (falseFromCorrect ? 2 : 0) | (useRamp ? 4 : 0) | ((freshSparse && freshBeforeTooFar) ? 16 : 0));
		}
		if (nPushed != slice) { status = GA_ASSERTION; break; }                  // :2768
		nPushed++;
		arenaTop += need;
		logCorrect = newCorrect; logWrong = newWrong;
		if (closedWindow) { storeRec = thisRec; storeMem = thisMem; }            // storeSlice = newSlice.getFrozenSqrtEndScores() (:2756)
		if constexpr (kWide)
		{
			if (rampPossible || kSparse)
			{
				// checkpoint = cheapest slice of each sqrt window (:2772-2786)
				if (slice % sampling == 0)
				{
					if (nCkpt == 0 || recSlice(storeRec) != recSlice(slot.ckpt[nCkpt - 1]))
					{
						if (GA_LANE0) slot.ckpt[nCkpt] = storeRec;
						nCkpt++;
						storeRec = thisRec; storeMem = thisMem;
					}
				}
				if (thisMem < storeMem) { storeRec = thisRec; storeMem = thisMem; }
				ws_order<MAXN>();
			}
		}
		lastRec = thisRec;
		lastNumCells = freshCells;
		adoptSlice();
	}
	if constexpr (kSparse)
	{
		// a window still open when the slices end (:2810-2825); its checkpoints go, nothing is pushed
		if (status == GA_OK && overriding) status = closeWindow();
	}
	out.n_run = nRun;
	GA_LAP(0);

	// ---- drop the wrongly aligned tail (removeWronglyAlignedEnd, :2554-2569) ----
	uint32_t kept = nPushed;
	if (status == GA_OK && kept > 0)
	{
		wave_sync();
		bool ok = slot.slice_flags[kept - 1] & 1;
		while (!ok)
		{
			kept--;
			if (kept == 0) break;
			ok = (slot.slice_flags[kept - 1] & 2) != 0;
		}
	}
	out.n_valid = status == GA_OK ? kept : 0;

	// ---- after a ramp redo the slices the traceback sees are those the reference would recompute from its
	// checkpoints (getSlicesFromTable :2858-2943); a checkpoint taken before the redo can disagree with the slices kept ----
	const uint32_t* inTab = slot.slice_off;       // record traced through, per slice
	const uint32_t* belowTab = slot.slice_off;    // record standing for the slice above a slice boundary
	uint32_t startRec = kept > 0 ? slot.slice_off[kept - 1] : 0;
	if constexpr (kWide)
	{
		const bool tableTouched = redone || (kSparse && anyOverride);             // (otherwise the checkpoint list is in order by construction)
		if (status == GA_OK && tableTouched)
		{
			// the checks at the end of getSqrtSlices (:2833-2854) look at the whole checkpoint list, before the wrongly aligned tail
			// is trimmed (removeWronglyAlignedEnd is the caller's next step, :3002,3018) and whether or not anything is kept
			wave_sync();
			if (nCkpt == 0) status = GA_ASSERTION;                                // :2834
			for (uint32_t i = 1; i < nCkpt && status == GA_OK; i++)
			{
				const uint32_t a = slot.ckpt[i - 1], b = slot.ckpt[i];
				if (i >= 2 && !(recJ(b) > recJ(a))) status = GA_ASSERTION;                           // :2835-2838
				const int ma = a == kSeedRecord ? 0 : (int)slot.arena[a + 2], mb = b == kSeedRecord ? 0 : (int)slot.arena[b + 2];
				if (mb < ma) status = GA_ASSERTION;                                                // :2839-2842
			}
			if constexpr (kSparse)
			{
				for (uint32_t i = 1; i < nOv && status == GA_OK; i++) if (!(slot.ovr[2 * i] > slot.ovr[2 * (i - 1) + 1])) status = GA_ASSERTION;   // :2850-2853
			}
			if (status != GA_OK) out.n_valid = 0;
		}
		if (status == GA_OK && tableTouched && kept > 0 && numSlices >= 4)
		{
			wave_sync();
			const auto firstPassColumns = out.n_columns;                          // the column-update count is the first pass's (cellsProcessed)
			const auto firstPassNodes = out.max_band_nodes;
			// trimmed checkpoints (:2566-2568; the overrides are not trimmed)
			while (status == GA_OK && nCkpt > 1 && recJ(slot.ckpt[nCkpt - 1]) >= (uint64_t)kept * W) nCkpt--;
			for (uint32_t sIdx = 0; sIdx < kept; sIdx++) if (GA_LANE0) slot.below_off[sIdx] = slot.slice_off[sIdx];
			wave_sync();
			// getTraceFromTable's walk over the checkpoints, last to first (:917-947): between two of them the reference recomputes the slices
			// (asserting what getSlicesFromTable asserts, freezing every recomputed slice), and where a checkpoint is the last slice of the
			// next override window it follows that window's links instead and recomputes nothing of it
			uint32_t usedLo = 0xffffffffu;                                        // lastBacktraceOverrideStartJ / 64
			int ovIdx = (int)nOv - 1;
			for (uint32_t i = nCkpt; i-- > 0 && status == GA_OK;)
			{
				const uint32_t ck = slot.ckpt[i];
				const uint32_t ckSlice = recSlice(ck);                               // 0xffffffff for the seed
				const uint32_t firstSlice = ckSlice + 1;                             // wraps to 0 for the seed
				uint32_t endSlice = i + 1 == nCkpt ? kept : recSlice(slot.ckpt[i + 1]) + 1;
				if (ck != kSeedRecord && GA_LANE0) slot.below_off[ckSlice] = ck;
				if (firstSlice == kept)
				{
					if (i + 1 != nCkpt) status = GA_ASSERTION;                       // :911
					continue;
				}
				if constexpr (kSparse)
				{
					if (!(usedLo > firstSlice)) { status = GA_ASSERTION; break; }     // assert(overrideLastJ > startSlice * 64) (:2862)
					if (endSlice >= usedLo) endSlice = usedLo;                       // :2865
				}
				if (!(endSlice > firstSlice) || endSlice > kept) { status = GA_ASSERTION; break; }   // :2866-2867
				if constexpr (kSparse)
				{
					// result.push_back(newSlice.getFrozenScores()) for every recomputed slice (:2908; NodeSlice.h:344)
					wave_sync();
					for (uint32_t sl = firstSlice; sl < endSlice; sl++) if (slot.slice_flags[sl] & 16) status = GA_ASSERTION;
					if (status != GA_OK) break;
				}
				const bool consistent = ck == kSeedRecord || ck == slot.slice_off[ckSlice];
				if (!consistent && redone)
				{
					// the recompute would NOT reproduce the kept slices: a checkpoint taken before a ramp redo
					loadRecordState(ck);
					for (uint32_t sl = firstSlice; sl < endSlice && status == GA_OK; sl++)
					{
						const int bandwidth = (slot.slice_flags[sl] & 4) ? L.ramp_bw : L.initial_bw;
						status = runSlice(sl, bandwidth);
						if (status != GA_OK) break;
						if (freshSparse && (freshEndsTooFar || freshBeforeTooFar)) { status = GA_ASSERTION; break; }
						if (GA_LANE0) { slot.arena[arenaTop + 10] = sl; slot.slice_off[sl] = (uint32_t)arenaTop; if (sl + 1 < endSlice || i + 1 == nCkpt) slot.below_off[sl] = (uint32_t)arenaTop; }
						arenaTop += need;
						adoptSlice();
					}
				}
				if constexpr (kSparse)
				{
					if (status == GA_OK && ck != kSeedRecord && ovIdx >= 0 && ckSlice == slot.ovr[2 * ovIdx + 1])
					{
						// GetBacktrace through the window (:939-946): its slices are the first pass's; flag them for the traceback's row-63 rule
						const uint32_t lo = slot.ovr[2 * ovIdx];
						if (GA_LANE0) for (uint32_t sl = lo; sl <= ckSlice; sl++) slot.slice_flags[sl] |= 8;
						usedLo = lo;
						ovIdx--;
					}
				}
			}
			wave_sync();
			if (status == GA_OK)
			{
				// the trace starts at the last checkpoint when that is the last kept slice itself (:908-916), else at the last slice of the last window
				const uint32_t lastCk = slot.ckpt[nCkpt - 1];
				startRec = (lastCk != kSeedRecord && recSlice(lastCk) + 1 == kept) ? lastCk : slot.slice_off[kept - 1];
			}
			belowTab = slot.below_off;
			out.n_columns = firstPassColumns;
			out.max_band_nodes = firstPassNodes;
		}
	}

	// ---- traceback (getTraceFromTable :894-957 with pickBacktracePredecessor :493-591) ----
	if (status == GA_OK && kept > 0)
	{
		if (numSlices < 4) status = GA_ASSERTION;                                // assert(slice.samplingFrequency > 1) (:906)
	}
	if (status == GA_OK && kept > 0)
	{
		uint8_t* tr = slot.trace;
		const int big = (int)job.n_rows;                                         // getValueOrMax default = sequence.size()
		uint32_t sIdx = kept - 1;
		uint32_t off = inTab[sIdx];
		uint32_t nN = slot.arena[off], nC = slot.arena[off + 1];
		SliceRec cur = slice_at(slot.arena, off, nN, nC);
		const SliceRec from = slice_at(slot.arena, startRec, slot.arena[startRec], slot.arena[startRec + 1]);   // = cur unless a ramp redo left a stale checkpoint
		out.score = (int32_t)from.hdr[2];
		uint32_t node = from.nodes[from.hdr[3]];
		uint32_t offset = from.hdr[4];
		uint32_t row = sIdx * W + (W - 1);
		uint32_t len = 0, nodeSteps = 0;
		out.start_node = node; out.start_offset = offset; out.start_row = row;
		SliceRec prv = cur;
		uint32_t pN = 0;
		// node lists (node id, first column in the record) of the slice traced through and of the one above it, in LDS
		uint32_t* curNodes = ws.cn_node; uint32_t* curBase = ws.cn_colBase;
		uint32_t* prvNodes = ws.pn_node; uint32_t* prvBase = ws.pn_colBase;
		auto loadTable = [&](uint32_t* tn, uint32_t* tb, const SliceRec& r, uint32_t n) {
			ws_order<MAXN>();
			for (uint32_t c = 0; c < n; c += LANES)
			{
				store_lanes(tn + c, (int)(n - c), load_lanes(r.nodes + c, (int)(n - c), 0));
				store_lanes(tb + c, (int)(n - c), load_lanes(r.colBase + c, (int)(n - c), 0));
			}
			ws_order<MAXN>();
		};
		auto loadPrev = [&]() {
			if (sIdx == 0) return;
			uint32_t o = belowTab[sIdx - 1];
			pN = slot.arena[o];
			prv = slice_at(slot.arena, o, pN, slot.arena[o + 1]);
			loadTable(prvNodes, prvBase, prv, pN);
		};
		wave_sync();
		loadTable(curNodes, curBase, cur, nN);
		loadPrev();
		auto valuePrevLastRow = [&](uint32_t n, uint32_t o2) -> int {
			// row 63 of the slice before; before slice 0 that is the all-zero seed slice
			if (sIdx == 0) return n == job.seed_node ? 0 : big;
			return stored_value(prv, prvNodes, prvBase, pN, n, o2, W - 1, big);
		};
		Window cw, pw;
		cw.valid = false; pw.valid = false;
		cw.vp = VU(0); cw.vn = VU(0); cw.before = VI(0); pw.vp = VU(0); pw.vn = VU(0); pw.before = VI(0);
		cw.slice = cw.node = pw.slice = pw.node = 0; cw.lo = cw.n = pw.lo = pw.n = 0; cw.present = pw.present = false;
		VI winBases = VI(0);
		VI rowv = load_lanes(rows + sIdx * W, W, 0);
		uint32_t rowvSlice = sIdx;
		const VI lane = lane_iota();
		VI winRec = VI(0);                         // graph record of the node the current window lies in
		uint32_t winRecNode = 0xffffffffu;
		while (true)
		{
			if (row == 0xffffffffu) break;                                       // reached the row before the first one
			if (len + LANES >= L.trace_cap) { status = GA_CAP_TRACE; break; }
			int r = (int)(row - sIdx * W);
			if (rowvSlice != sIdx) { rowv = load_lanes(rows + sIdx * W, W, 0); rowvSlice = sIdx; }
			if constexpr (kSparse)
			{
				// inside an override window the reference follows precomputed links, and a cell of a slice's last row without an end
				// score has none (BacktraceItem::end, :311-317; assert(!current.end) :211; the entry cell must be among them, :202-209)
				if (r == W - 1 && (slot.slice_flags[sIdx] & 8))
				{
					const int sx = find_slot(curNodes, (int)nN, node);
					if (sx < 0) { status = GA_ASSERTION; break; }
					const uint8_t* ex = (const uint8_t*)(cur.before + cur.hdr[1]);
					if (ex[curBase[sx] + offset] == 0) { status = GA_ASSERTION; break; }
				}
			}
			// ---- make the current window cover this column (and its left neighbour when there is one) ----
			bool covers = cw.valid && cw.slice == sIdx && cw.node == node && (int)offset >= cw.lo && (int)offset < cw.lo + cw.n && !((int)offset == cw.lo && offset > 0);
			if (!covers)
			{
				if (pw.valid && pw.slice == sIdx && pw.node == node && (int)offset >= pw.lo && (int)offset < pw.lo + pw.n && !((int)offset == pw.lo && offset > 0))
				{
					cw = pw;                                                   // the window fetched for the slice boundary becomes current
				}
				else
				{
					if (winRecNode != node) { winRec = g_record(g, node); winRecNode = node; }      // travels together with the window's words
					load_window(cw, cur, curNodes, curBase, nN, sIdx, node, offset);
					const uint64_t firstCol = (((uint64_t)(uint32_t)read_lane(winRec, 1) << 32) | (uint32_t)read_lane(winRec, 0)) + (uint32_t)cw.lo;
					VI at = lane + (int)(firstCol & 15);
					winBases = (gather(g.seq2 + (firstCol >> 4), at >> 4) >> ((at & 15) << 1)) & 3;
				}
				pw.valid = false;
			}
			if (winRecNode != node) { winRec = g_record(g, node); winRecNode = node; }
			if (!cw.present) { status = GA_ASSERTION; break; }                   // assert(slice.scores.hasNode(nodeIndex)) (:498)
			int rel = (int)offset - cw.lo;
			uint64_t maskR = r < 63 ? ~(~0ull << (r + 1)) : ~0ull;
			VI valR = cw.before + vpopc(maskR & cw.vp) - vpopc(maskR & cw.vn);
			int here = read_lane(valR, rel);
			if (row == 0 && node == job.seed_node && (here == 0 || here == 1)) { row = 0xffffffffu; continue; }   // free start (:500)
			// ---- a run of diagonal steps inside the window, all at once ----
			// Lane L looks at the diagonal cell (column L, row L + r - rel).  A step from column L+1
			// to L is diagonal iff the horizontal move is not taken (:541-546) and the diagonal cell
			// has the matching score (:556-571); the run is the stretch of such lanes below `rel`.
			if (rel >= 1 && r >= 1)
			{
				const VI rho = lane + (r - rel);
				const VU mA = mask_low_bits(rho + 1);
				const VI A = cw.before + vpopc(cw.vp & mA) - vpopc(cw.vn & mA);
				// one row further down: add that row's vertical delta
				const VI B = A + bit64_at(cw.vp, rho + 1) - bit64_at(cw.vn, rho + 1);
				const VI mOwn = (lane_gather(rowv, rho) >> winBases) & 1;
				const VI hereSrc = shl1(A, 0), mSrc = shl1(mOwn, 0);
				const uint64_t cond = ballot(B > hereSrc - 1) & ballot(A == hereSrc - 1 + mSrc) & ballot((lane < rel) && (rho > -1));
				const uint64_t broken = ~(cond << (64 - rel));
				int run = broken == 0 ? 64 : __builtin_clzll(broken);
				run = run < rel ? run : rel;
				if (run >= 2)
				{
					// the whole run is `run` diagonal moves inside the node
					store_lanes(tr + len, run, VI(GA_MOVE_DIAG));
					len += (uint32_t)run;
					offset -= (uint32_t)run;
					row -= (uint32_t)run;
					// the run ended because the next step is not a plain diagonal one: take that step right away from the new
					// cell (same window, same slice) unless the window has to move first
					rel -= run;
					r -= run;
					if (rel == 0 && offset > 0) continue;
					maskR = r < 63 ? ~(~0ull << (r + 1)) : ~0ull;
					valR = cw.before + vpopc(maskR & cw.vp) - vpopc(maskR & cw.vn);
					here = read_lane(valR, rel);
					if (row == 0 && node == job.seed_node && (here == 0 || here == 1)) { row = 0xffffffffu; continue; }
					if (len + LANES >= L.trace_cap) { status = GA_CAP_TRACE; break; }
				}
			}
			const int rowCode = read_lane(rowv, r);
			const int base = read_lane(winBases, rel);
			const bool match = (rowCode >> base) & 1;
			// values one row up: same window for r > 0, the slice above (its row 63) for r == 0
			VI valUp;
			bool upKnown = true;
			if (r > 0)
			{
				const uint64_t maskU = ~(~0ull << r);
				valUp = cw.before + vpopc(maskU & cw.vp) - vpopc(maskU & cw.vn);
			}
			else if (sIdx == 0)
			{
				valUp = VI(node == job.seed_node ? 0 : big);
			}
			else
			{
				if (!(pw.valid && pw.slice == sIdx - 1 && pw.node == node && pw.lo == cw.lo && pw.n == cw.n))
					load_window(pw, prv, prvNodes, prvBase, pN, sIdx - 1, node, (uint32_t)(cw.lo + cw.n - 1));
				if (pw.present) valUp = pw.before + vpopc(pw.vp) - vpopc(pw.vn);
				else valUp = VI(big);
			}
			(void)upKnown;
			int res = 0;
			int viaNeighbour = 0;                                                // ordinal of the in-neighbour a move enters (0 inside a node)
			const uint32_t curNode = node, curOffset = offset;
			auto decide = [&](int horizontal, int diagonal, uint32_t un, uint32_t uo) -> int {
				if (horizontal < here - 1) return -1;
				if (horizontal == here - 1) { node = un; offset = uo; return 1; }
				if (match)
				{
					if (diagonal < here) return -1;
					if (diagonal == here) { node = un; offset = uo; row = row - 1; return 2; }
				}
				else
				{
					if (diagonal < here - 1) return -1;
					if (diagonal == here - 1) { node = un; offset = uo; row = row - 1; return 2; }
				}
				return 0;
			};
			if (curOffset == 0)
			{
				const int inDeg = read_lane(winRec, 3) & 0xffff;
				if (inDeg <= kNbr)
				{
					// the last columns of all in-neighbours (this slice, and the slice above when at its first row) in one round trip:
					// lane k < inDeg looks at in-neighbour k; the record holds the neighbours and their lengths
					const VI nbr = lane_gather(winRec, vmin(lane, VI(kNbr - 1)) + 8);
					const VI nbrLast = lane_gather(winRec, vmin(lane, VI(kNbr - 1)) + 12) - 1;
					VI idxCur = VI(-1), idxPrv = VI(-1);
					for (int k = 0; k < inDeg; k++)
					{
						const uint32_t m = (uint32_t)read_lane(nbr, k);
						const int sc = find_slot(curNodes, (int)nN, m);
						if (sc >= 0) idxCur = select(lane == k, VI((int)curBase[sc]) + nbrLast, idxCur);
						if (r == 0 && sIdx > 0)
						{
							const int sp = find_slot(prvNodes, (int)pN, m);
							if (sp >= 0) idxPrv = select(lane == k, VI((int)prvBase[sp]) + nbrLast, idxPrv);
						}
					}
					const VB haveC = idxCur > -1;
					const VI safeC = select(haveC, idxCur, VI(0));
					const VU vpC = select(haveC, gather64(cur.vp, safeC), VU(0)), vnC = select(haveC, gather64(cur.vn, safeC), VU(0));
					const VI beC = gather(cur.before, safeC);
					const VI horV = select(haveC, beC + vpopc(vpC & VU(maskR)) - vpopc(vnC & VU(maskR)), VI(big));
					VI diaV;
					if (r > 0)
					{
						const uint64_t maskU = ~(~0ull << r);
						diaV = select(haveC, beC + vpopc(vpC & VU(maskU)) - vpopc(vnC & VU(maskU)), VI(big));
					}
					else if (sIdx == 0) diaV = select(nbr == (int)job.seed_node, VI(0), VI(big));
					else
					{
						const VB haveP = idxPrv > -1;
						const VI safeP = select(haveP, idxPrv, VI(0));
						diaV = select(haveP, gather(prv.before, safeP) + vpopc(gather64(prv.vp, safeP)) - vpopc(gather64(prv.vn, safeP)), VI(big));
					}
					for (int k = 0; k < inDeg && res == 0; k++)
					{
						viaNeighbour = k;
						res = decide(read_lane(horV, k), read_lane(diaV, k), (uint32_t)read_lane(nbr, k), (uint32_t)read_lane(nbrLast, k));
					}
				}
				else
				{
					for (uint32_t e = g.in_off[curNode]; e < g.in_off[curNode + 1] && res == 0; e++)
					{
						uint32_t m = g.in_nbr[e];
						uint32_t mo = g_len(g, m) - 1;
						viaNeighbour = (int)(e - g.in_off[curNode]);
						int horizontal = stored_value(cur, curNodes, curBase, nN, m, mo, r, big);
						int diagonal = 0;
						if (horizontal > here - 1) diagonal = r == 0 ? valuePrevLastRow(m, mo) : stored_value(cur, curNodes, curBase, nN, m, mo, r - 1, big);
						res = decide(horizontal, diagonal, m, mo);
					}
				}
			}
			else res = decide(read_lane(valR, rel - 1), read_lane(valUp, rel - 1), curNode, curOffset - 1);
			if (curOffset == 0 && (res == 1 || res == 2)) nodeSteps++;           // left the node through its first column
			if (res < 0) { status = GA_ASSERTION; break; }
			if (res == 0)
			{
				int up = read_lane(valUp, rel);
				if (up != here - 1) { status = GA_ASSERTION; break; }            // assert(false) (:588)
				row = row - 1;
				res = 3;
			}
			// put the move away (the step onto the row before the first one is not part of the trace, :949-950)
			if (row != 0xffffffffu)
			{
				if (viaNeighbour > 62) { status = GA_CAP_TRACE; break; }
				const int code = res == 1 ? GA_MOVE_LEFT : res == 2 ? GA_MOVE_DIAG : GA_MOVE_UP;
				if (GA_LANE0) tr[len] = (uint8_t)(code | (res == 3 ? 0 : (viaNeighbour << 2)));
				len++;
			}
			if (res >= 2 && r == 0 && row != 0xffffffffu)
			{
				// stepped into the slice above
				sIdx--;
				if (belowTab[sIdx] == inTab[sIdx])
				{
					cur = prv; nN = pN;
					uint32_t* t = curNodes; curNodes = prvNodes; prvNodes = t;
					t = curBase; curBase = prvBase; prvBase = t;
				}
				else
				{
					// the slice is traced through in another version than the one the boundary step looked at
					const uint32_t o = inTab[sIdx];
					nN = slot.arena[o];
					cur = slice_at(slot.arena, o, nN, slot.arena[o + 1]);
					loadTable(curNodes, curBase, cur, nN);
					pw.valid = false;
				}
				loadPrev();
			}
		}
		GA_LAP(5);
		// hand the steps over: claim exactly `len` entries of the pool and copy them, 64 at a time
		if (status == GA_OK)
		{
			wave_sync();
			const uint32_t words = (len + 3) / 4;
			const uint64_t at = wave_claim(L.trace_top, (uint64_t)words * 4, L.trace_pool_cap);      // (commits only when it fits)
			if (at == ~0ull) status = GA_CAP_TRACE;
			else
			{
				uint32_t* dst = (uint32_t*)(L.traces + at);
				const uint32_t* src = (const uint32_t*)tr;
				for (uint32_t c = 0; c < words; c += LANES) store_lanes(dst + c, (int)(words - c), load_lanes(src + c, (int)(words - c), 0));
				out.trace_off = at;
				out.trace_len = len;
				out.n_node_steps = nodeSteps;
			}
		}
	}
	GA_LAP(6);
#undef GA_LAP
	out.status = status;
	if (GA_LANE0) L.outs[jobIndex] = out;
}

}  // namespace gak
