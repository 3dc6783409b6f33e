// ga_ops.h -- per-base alignment operations, run-length coded on the device (include/graphaligner_amd.h states the rule under GA_F_OPS;
// DESIGN.md section 11 argues it).  After the last pass of the ladder every finished job's traceback lies in the trace pool as one byte
// per move (ga_types.h: GA_MOVE_*).  This program walks those bytes where they lie and leaves, per job, the types of the TraceItems
// the job contributes (getTraceInfoInner, GraphAligner.h:718-780; traceItemsInner of ga_host.cpp) cut into maximal runs of equal type.
//
// One wave (= one workgroup of 64 lanes) takes one job at a time and walks its moves 64 per round.  Written in PHASES like ga_seed.h:
// inside GAO_LANES(l) { ... } every lane runs the block for its own l; lanes exchange values only through the OpsLds block with a
// sync() between the phase that writes and the phase that reads, and through the two wave primitives below (scan, ballot).  Everything
// declared outside a lane block is the same in every lane, so the control flow around the blocks is uniform.  On gfx950 a lane block
// is straight-line code of the lane; in the host build of the tests (tests/emul) it is a loop over the 64 lanes.
//
// The same program runs twice: a counting launch leaves one run count per job, an exclusive scan turns the counts into places, and a
// writing launch stores the runs there -- a backward job's in stream order, a forward job's back to front, which is the final order
// of both (reverseTrace, GraphAligner.h:3026-3037).  Jobs are dealt statically (wave w takes entries w, w + waves, ... of the job
// list) and every loop ends by a known count.
//
// walk_job takes what it does with the items as a parameter (SINK_COUNT, SINK_WRITE, or SINK_ADD with a sink object): the pileups of
// ga_pileup.h are this walk with an add per item in place of the runs.
#pragma once
#include "ga_backend.h"

namespace gao {

#ifdef GA_EMULATE
#define GAO_FN inline
#define GAO_LANES(l) for (int l = 0; l < 64; l++)
inline void sync() {}
#else
#define GAO_FN __device__ __forceinline__
#define GAO_LANES(l) if (const int l = (int)threadIdx.x; true)
GAO_FN void sync() { __syncthreads(); }
#endif

enum { OP_MATCH = 1, OP_MISMATCH = 2, OP_INSERTION = 3, OP_DELETION = 4, OP_SPLIT = 5 };

struct OpsLaunch
{
	GaDevGraph graph;
	const GaJob* jobs;
	const GaJobOut* outs;
	const GaEqFill* fills;                 // per job: where its rows come from in `seq`
	const uint8_t* traces;                 // the trace pool
	uint64_t trace_bytes;                  // its size: a job whose moves would leave it is not walked
	const uint8_t* seq;                    // the batch's resident copy of the reads
	uint64_t seq_bytes;
	const uint8_t* row_code;               // 256 entries: bits 0-3 = which of A, C, G, T the character matches
	const uint32_t* twin;                  // [n_nodes] the node of the other strand (0xffffffff: none); nullptr: the strands are exact mirrors
	const uint32_t* job_list;              // optional hand-out order; nullptr = identity
	uint32_t n_jobs, reserved;
	uint64_t* counts;                      // [n_jobs + 1] counting launch: runs per job (entry n_jobs stays 0)
	const uint64_t* offsets;               // [n_jobs + 1] writing launch: the scanned counts
	uint32_t* runs;                        // writing launch: type | length << 3
};

struct OpsLds
{
	uint8_t code[256];
	uint32_t own[64];                      // the lane's move: row step | column step << 16
	uint32_t incl[64];                     // inclusive sums of own
	uint32_t colLane[64];                  // colLane[c] = the lane whose move is the round's c-th column step
	// per cell of the round (cell l = where move l starts; cell 64 = where the round ends): its node, the column steps of the round
	// after which that node's offset 0 is reached, the node's length and first column
	uint32_t cNode[65], cTop[65], cLen[65];
	uint64_t cCol0[65];
	uint8_t mv[64], type[64], flag[64];
};

// inclusive scan of lds.own over the lanes into lds.incl (the caller syncs before and after)
GAO_FN void scan_steps(OpsLds& lds)
{
#ifdef GA_EMULATE
	uint32_t run = 0;
	for (int l = 0; l < 64; l++) { run += lds.own[l]; lds.incl[l] = run; }
#else
	const int l = (int)threadIdx.x;
	uint32_t v = lds.own[l];
	for (int d = 1; d < 64; d <<= 1) { const uint32_t o = (uint32_t)__shfl_up((int)v, d, 64); if (l >= d) v += o; }
	lds.incl[l] = v;
#endif
}

// bit l = lane l's byte is not zero (the caller syncs before)
GAO_FN uint64_t ballot(const uint8_t* flag)
{
#ifdef GA_EMULATE
	uint64_t m = 0;
	for (int l = 0; l < 64; l++) if (flag[l]) m |= 1ull << l;
	return m;
#else
	return __ballot(flag[threadIdx.x] != 0);
#endif
}

GAO_FN uint32_t popc(uint64_t x) { return (uint32_t)__builtin_popcountll(x); }
GAO_FN uint32_t ctz(uint64_t x) { return (uint32_t)__builtin_ctzll(x); }

// a node of length 1 that has itself as out-neighbour: a step up in its column is a diagonal to the reference (GraphAligner.h:742)
GAO_FN bool self_loop(const GaDevGraph& g, uint32_t node)
{
	const uint32_t lo = g.out_off[node], hi = g.out_off[node + 1];
	bool found = false;
	for (uint32_t e = lo; e < hi; e++) found = found || g.out_nbr[e] == node;
	return found;
}

// what a walk does with the items it finds: count the runs of their types, write those runs at the job's scanned place, or hand every
// item with its column to `sink` (ga_pileup.h), which then sees the left moves' cells too and no runs are formed
// SINK_EDGES (ga_edges.h): the items themselves are not looked at; every node crossing whose two cells both have an item is handed to
// `sink` as the slot of the edge it takes (position in the in-neighbour lists laid end to end).  Its code is compiled into no other walk
// SINK_PATH (ga_pathseq.h): no item is formed and no read character looked at; every round, with its cells, is handed to `sink`, which
// counts or writes the cells' bases, and so is the stream's last cell behind the loop (a job without moves still has that cell).  Its
// code is compiled into no other walk either
enum { SINK_COUNT = 0, SINK_WRITE = 1, SINK_ADD = 2, SINK_EDGES = 3, SINK_PATH = 4 };
struct NoSink { GAO_FN void item(uint32_t, uint64_t, uint32_t) {} };

// the runs of one job: returns their number (SINK_ADD: 0)
template <int SINK, class Sink> GAO_FN uint32_t walk_job(const OpsLaunch& L, OpsLds& lds, uint32_t job, Sink& sink)
{
	constexpr bool WRITE = SINK == SINK_WRITE;
	const GaDevGraph& G = L.graph;
	const GaJobOut* o = L.outs + job;
	const uint32_t nMoves = o->trace_len;
	if (o->status != GA_OK || o->n_valid == 0 || o->reserved3 == 1 || (nMoves == 0 && SINK != SINK_PATH)) return 0;
	const uint64_t traceOff = o->trace_off;
	if (traceOff + nMoves > L.trace_bytes || o->start_node >= G.n_nodes) return 0;
	const uint8_t* mv = L.traces + traceOff;
	const uint32_t traceRows = L.jobs[job].trace_rows;
	const GaEqFill f = L.fills[job];
	const bool backward = f.backward != 0;
	if (SINK == SINK_ADD && backward && !L.twin) return 0;    // (an item's column on the other strand needs the table)
	const uint64_t totalBp = G.node_start[G.n_nodes];
	// the walk's state at the round's first move: the node, the column steps after which its offset 0 is reached (= the offset), the row
	uint32_t node = o->start_node, top = o->start_offset, row0 = o->start_row;
	const uint32_t* rec = G.node_rec + (uint64_t)node * GA_NODE_REC_WORDS;
	uint32_t len = rec[2];
	uint64_t col0 = (uint64_t)rec[0] | ((uint64_t)rec[1] << 32);
	if (top >= len) return 0;
	uint64_t base = 0, cnt = 0;
	if (WRITE) { base = L.offsets[job]; cnt = L.offsets[job + 1] - base; }
	uint32_t opened = 0, carryType = 0, carryLen = 0;       // runs opened so far; the open run
	[[maybe_unused]] uint32_t prevRow = 0xffffffffu;        // SINK_EDGES: the row the round before's last move starts in (none yet: no row)
	bool bad = false;
	for (uint32_t m0 = 0; m0 < nMoves && !bad; m0 += 64)
	{
		const uint32_t nValid = nMoves - m0 < 64 ? nMoves - m0 : 64;
		sync();                                                // (the round before is no longer read)
		GAO_LANES(l)
		{
			uint32_t s = 0;
			uint8_t b = 0;
			if ((uint32_t)l < nValid)
			{
				b = mv[m0 + (uint32_t)l];
				const uint32_t code = b & 3u;
				s = (code != GA_MOVE_LEFT ? 1u : 0u) | (code != GA_MOVE_UP ? 0x10000u : 0u);
			}
			lds.mv[l] = b;
			lds.own[l] = s;
		}
		sync();
		scan_steps(lds);
		sync();
		const uint32_t totalRows = lds.incl[63] & 0xffffu, totalCols = lds.incl[63] >> 16;
		GAO_LANES(l)
		{
			const uint32_t cb = (lds.incl[l] - lds.own[l]) >> 16;
			if (lds.own[l] >> 16) lds.colLane[cb] = (uint32_t)l;
			lds.cNode[l] = node; lds.cTop[l] = top; lds.cLen[l] = len; lds.cCol0[l] = col0;
		}
		sync();
		// node crossings inside the round: the column step number `top` leaves offset 0 through the in-neighbour its move names; the
		// cells behind it re-base on that neighbour.  Each crossing consumes a column step: at most 64 per round
		for (uint32_t k = 0; k < 64 && top < totalCols; k++)
		{
			const uint32_t via = (uint32_t)lds.mv[lds.colLane[top]] >> 2;
			const uint32_t inLo = G.in_off[node], inHi = G.in_off[node + 1];
			if (via >= inHi - inLo) { bad = true; break; }
			const uint32_t next = via < 4 ? rec[8 + via] : G.in_nbr[inLo + via];
			if (next >= G.n_nodes) { bad = true; break; }
			node = next;
			rec = G.node_rec + (uint64_t)node * GA_NODE_REC_WORDS;
			len = rec[2];
			col0 = (uint64_t)rec[0] | ((uint64_t)rec[1] << 32);
			const uint32_t from = top + 1;
			top += len;
			GAO_LANES(l)
			{
				const uint32_t cb = (lds.incl[l] - lds.own[l]) >> 16;
				if (cb >= from) { lds.cNode[l] = node; lds.cTop[l] = top; lds.cLen[l] = len; lds.cCol0[l] = col0; }
			}
		}
		if (bad || top < totalCols) { bad = true; break; }     // (a node of length 0, or a move that names no in-neighbour: nothing the kernels write)
		GAO_LANES(l) { if (l == 0) { lds.cNode[64] = node; lds.cTop[64] = top; lds.cLen[64] = len; lds.cCol0[64] = col0; } }
		sync();
		if constexpr (SINK == SINK_EDGES)
		{
			// the lane whose move is the column step numbered cTop of its cell crosses from `to`, the cell's node, into `from`, the next
			// cell's: the edge from -> to, named by its place in to's in-list.  It counts when both cells have an item -- forward: the
			// cells moves m and m + 1 start in (the stream's last cell has none); backward: the cells moves m - 1 and m lead to, where
			// move m - 1 may be the round before's last (prevRow) --, neither lies on a dummy node and the two are not one column
			GAO_LANES(l)
			{
				const uint32_t excl = lds.incl[l] - lds.own[l];
				if ((uint32_t)l < nValid && (lds.own[l] >> 16) != 0 && (excl >> 16) == lds.cTop[l])
				{
					const uint32_t m = m0 + (uint32_t)l;
					const uint32_t rowA = row0 - (excl & 0xffffu), rowB = rowA - (lds.own[l] & 0xffffu);
					const uint32_t rowBefore = l == 0 ? prevRow : rowA + (lds.own[l > 0 ? l - 1 : 0] & 0xffffu);
					const bool both = backward ? m > 0 && rowBefore < traceRows && rowA < traceRows : rowA < traceRows && rowB < traceRows && m + 1 < nMoves;
					const uint32_t to = lds.cNode[l], from = lds.cNode[l + 1], last = G.n_nodes - 1;
					if (both && to != 0 && to != last && from != 0 && from != last && !(to == from && lds.cLen[l] == 1))
						sink.crossing(G.in_off[to] + ((uint32_t)lds.mv[l] >> 2), backward);
				}
			}
			prevRow = row0 - ((lds.incl[63] - lds.own[63]) & 0xffffu);
			top -= totalCols; row0 -= totalRows;
			continue;
		}
		if constexpr (SINK == SINK_PATH)
		{
			sink.round(L, lds, nValid, row0, traceRows, totalBp);
			top -= totalCols; row0 -= totalRows;
			continue;
		}
		GAO_LANES(l)
		{
			uint32_t t = 0;
			const uint32_t excl = lds.incl[l] - lds.own[l];
			const uint32_t rowA = row0 - (excl & 0xffffu);
			if ((uint32_t)l < nValid && rowA < traceRows)        // cells at rows >= trace_rows are dropped: the first moves of the stream
			{
				const uint32_t code = lds.mv[l] & 3u;
				if (SINK != SINK_ADD && code == GA_MOVE_LEFT) t = OP_DELETION;
				else
				{
					// forward: the item describes the cell the move starts in; backward: the cell it leads to
					const int ci = backward ? l + 1 : l;
					const uint32_t cb = backward ? lds.incl[l] >> 16 : excl >> 16;
					uint32_t cn = lds.cNode[ci], cl = lds.cLen[ci];
					uint64_t col = lds.cCol0[ci] + (lds.cTop[ci] - cb);
					bool flip = false;
					if (backward)
					{
						// the final trace holds the mirror cell (reverseTrace): the other strand's node, the offset counted from its end.  On a
						// graph with overlaps that node is not the exact reverse complement, so its own base is read
						if (!L.twin) flip = true;
						else
						{
							const uint32_t other = L.twin[cn];
							if (other >= G.n_nodes) cn = 0;                // (no mirror: the read ends in the assertion and has no runs)
							else
							{
								const uint32_t* orec = G.node_rec + (uint64_t)other * GA_NODE_REC_WORDS;
								const uint32_t off = lds.cTop[ci] - cb;
								col = ((uint64_t)orec[0] | ((uint64_t)orec[1] << 32)) + (orec[2] - 1 - off);
								cl = orec[2];
								cn = off < orec[2] ? other : 0;
							}
						}
					}
					uint32_t readByte = 256;
					bool diagonal = code == GA_MOVE_DIAG;
					if (SINK == SINK_ADD && code == GA_MOVE_LEFT) t = OP_DELETION;
					else if (!diagonal) { if (cl == 1 && self_loop(G, cn)) diagonal = true; else t = OP_INSERTION; }
					if (diagonal)
					{
						const uint32_t row = backward ? rowA - 1 : rowA;
						const uint64_t at = f.seq_off + (backward ? (uint64_t)traceRows - 1 - row : (uint64_t)f.pos + row);
						bool match = false;
						if (cn != 0 && cn != G.n_nodes - 1 && at < L.seq_bytes && col < totalBp)      // (a cell on a dummy node matches nothing)
						{
							uint32_t b = (G.seq2[col >> 4] >> ((col & 15) * 2)) & 3u;
							if (flip) b = 3u - b;
							readByte = L.seq[at];
							match = ((lds.code[readByte] >> b) & 1u) != 0;
						}
						t = match ? OP_MATCH : OP_MISMATCH;
					}
					// (an item on a dummy node is not counted, nor one whose mirror cell does not exist)
					if (SINK == SINK_ADD && cn != 0 && cn != G.n_nodes - 1 && col < totalBp) sink.item(t, col, readByte);
				}
			}
			if (SINK != SINK_ADD) lds.type[l] = (uint8_t)t;
		}
		if (SINK == SINK_ADD) { top -= totalCols; row0 -= totalRows; continue; }
		sync();
		GAO_LANES(l)
		{
			const uint32_t t = lds.type[l], prev = l == 0 ? carryType : lds.type[l - 1];
			lds.flag[l] = t != 0 && t != prev ? 1 : 0;
		}
		sync();
		const uint64_t starts = ballot(lds.flag), active = ballot(lds.type);
		const uint32_t nActive = popc(active);
		if (!starts) carryLen += nActive;
		else
		{
			// every start but the round's last opens a run that also ends in this round; the first one ends the run carried in
			const uint32_t first = ctz(starts), last = 63u - (uint32_t)__builtin_clzll(starts), firstActive = ctz(active);
			if (WRITE)
			{
				GAO_LANES(l)
				{
					if (l == 0 && carryType)
					{
						const uint64_t idx = opened - 1;
						if (idx < cnt) L.runs[base + (backward ? idx : cnt - 1 - idx)] = carryType | ((carryLen + first - firstActive) << 3);
					}
					if (((starts >> l) & 1) && (uint32_t)l != last)
					{
						const uint64_t rest = starts & ~((2ull << l) - 1);
						const uint64_t idx = opened + popc(starts & ((1ull << l) - 1));
						if (idx < cnt) L.runs[base + (backward ? idx : cnt - 1 - idx)] = lds.type[l] | ((ctz(rest) - (uint32_t)l) << 3);
					}
				}
			}
			carryType = lds.type[last];
			carryLen = firstActive + nActive - last;
			opened += popc(starts);
		}
		top -= totalCols;
		row0 -= totalRows;
	}
	if (bad) return 0;
	if constexpr (SINK == SINK_PATH) return sink.end(L, node, len, col0, top, row0, traceRows, totalBp);
	if (WRITE && carryType)
	{
		GAO_LANES(l)
		{
			const uint64_t idx = opened - 1;
			if (l == 0 && idx < cnt) L.runs[base + (backward ? idx : cnt - 1 - idx)] = carryType | (carryLen << 3);
		}
	}
	return opened;
}

// one wave's share of a launch: entries wave, wave + nWaves, ... of the job list
template <bool WRITE> GAO_FN void run_wave(const OpsLaunch& L, OpsLds& lds, uint32_t wave, uint32_t nWaves)
{
	GAO_LANES(l) { for (uint32_t i = (uint32_t)l; i < 256; i += 64) lds.code[i] = L.row_code[i]; }
	sync();
	const uint32_t per = nWaves ? (L.n_jobs + nWaves - 1) / nWaves : 0;
	for (uint32_t k = 0; k < per; k++)
	{
		const uint32_t at = wave + k * nWaves;
		if (at >= L.n_jobs) break;
		const uint32_t job = L.job_list ? L.job_list[at] : at;
		if (job >= L.n_jobs) continue;
		NoSink none;
		const uint32_t n = walk_job<WRITE ? SINK_WRITE : SINK_COUNT>(L, lds, job, none);
		if (!WRITE) { GAO_LANES(l) { if (l == 0) L.counts[job] = n; } }
		sync();
	}
}

}  // namespace gao
