// ga_pathseq.h -- path sequences: the graph's bases along each alignment, written on the device (include/graphaligner_amd.h states the
// rule under GA_F_PATHSEQ; DESIGN.md section 15 argues it).  The program is the walk of ga_ops.h once more with SINK_PATH: the walk
// forms the round's cells and hands the round to the sink below, which looks at no read character and forms no runs.  Per job the
// sequence is the base of c_0, the first cell of the job's part in read order, and then one base per kept move that takes a column
// step (a diagonal or a move left) or goes up inside a one-base node with itself as out-neighbour; a cell on a dummy node gives none.
//
// The same program runs twice, as the operations do: a counting launch leaves one count per job (it loads no base), the 64-bit scan
// turns the counts into places, and a writing launch stores one ASCII byte per base there -- a backward job's in stream order, a
// forward job's back to front.  Within a round a base's place is the bases before the round plus the emitting lanes below its lane
// (one ballot): there is no run to carry from round to round.  c_0 is one more byte: a backward job's comes first (the first cell of
// the stream at a row < trace_rows), a forward job's last (the stream's last cell).  Every store is a byte store of one lane at
// base + idx with idx < the job's count.
#pragma once
#include "ga_ops.h"

namespace gaps {

struct PathLaunch
{
	gao::OpsLaunch walk;                   // (seq, row_code, fills' rows and runs are not used; counts and offsets are the bases' per job)
	uint8_t* bases;                        // writing launch: offsets[n_jobs] bytes
};

// a cell of the final trace: a forward job's own cell, a backward job's mirror cell (ga_ops.h: the other strand's node at the offset
// counted from its end, through the twin table; without a table the cell itself with its base complemented).  node 0: the cell gives nothing
struct PathCell { uint32_t node, len; uint64_t col; bool flip; };
GAO_FN PathCell path_cell(const gao::OpsLaunch& L, bool backward, uint32_t node, uint32_t len, uint64_t col0, uint32_t off)
{
	const GaDevGraph& G = L.graph;
	PathCell c{node, len, col0 + off, false};
	if (!backward) return c;
	if (!L.twin) { c.flip = true; return c; }
	const uint32_t other = L.twin[node];
	if (other >= G.n_nodes) { c.node = 0; return c; }       // (no mirror: the read ends in the assertion and has no sequence)
	const uint32_t* orec = G.node_rec + (uint64_t)other * GA_NODE_REC_WORDS;
	c.col = ((uint64_t)orec[0] | ((uint64_t)orec[1] << 32)) + (orec[2] - 1 - off);
	c.len = orec[2];
	c.node = off < orec[2] ? other : 0;
	return c;
}
// whether the cell has a base: not on a dummy node, inside the graph's columns
GAO_FN bool path_cell_counts(const GaDevGraph& G, const PathCell& c, uint64_t totalBp) { return c.node != 0 && c.node != G.n_nodes - 1 && c.col < totalBp; }
GAO_FN uint8_t path_cell_base(const GaDevGraph& G, const PathCell& c)
{
	uint32_t b = (G.seq2[c.col >> 4] >> ((c.col & 15) * 2)) & 3u;
	if (c.flip) b = 3u - b;
	return (uint8_t)(0x54474341u >> (b * 8));                // "ACGT"[b]
}

// the sink of gao::walk_job<SINK_PATH>: everything in it is the same in every lane
template <bool WRITE_> struct PathSink
{
	static constexpr bool WRITE = WRITE_;
	uint8_t* bytes;                        // the job's place (writing launch)
	uint64_t cnt;                          // ... and its count: no store at or behind it
	uint32_t emitted;                      // bases so far, in stream order
	bool backward, first;                  // first: a backward job whose c_0 is still to come
	GAO_FN void item(uint32_t, uint64_t, uint32_t) {}      // (the walk's item code is not reached with SINK_PATH; it still has to compile)

	GAO_FN void begin(const gao::OpsLaunch& L, uint8_t* all, uint32_t job, bool isBackward)
	{
		bytes = nullptr; cnt = 0; emitted = 0; backward = isBackward; first = isBackward;
		if (WRITE) { bytes = all + L.offsets[job]; cnt = L.offsets[job + 1] - L.offsets[job]; }
	}
	// one byte by one lane, at the place of the base numbered idx in stream order
	GAO_FN void put(uint64_t idx, uint8_t ch) const { if (idx < cnt) bytes[backward ? idx : cnt - 1 - idx] = ch; }

	// a cell that is the same in every lane (c_0): its base, if it has one, is the next in stream order
	GAO_FN void whole_cell(const gao::OpsLaunch& L, uint32_t node, uint32_t len, uint64_t col0, uint32_t off, uint64_t totalBp)
	{
		const PathCell c = path_cell(L, backward, node, len, col0, off);
		if (!path_cell_counts(L.graph, c, totalBp)) return;
		if (WRITE) { GAO_LANES(l) { if (l == 0) put(emitted, path_cell_base(L.graph, c)); } }
		emitted++;
	}

	// one round of the walk (the cells are formed, lds.cNode .. lds.cCol0 of cells 0 .. 64; the caller has synced)
	GAO_FN void round(const gao::OpsLaunch& L, gao::OpsLds& lds, uint32_t nValid, uint32_t row0, uint32_t traceRows, uint64_t totalBp)
	{
		const GaDevGraph& G = L.graph;
		if (first)
		{
			// c_0 of a backward job: the cell the first kept move starts in.  Rows only fall along the stream, so that is the lowest lane at a row < trace_rows
			GAO_LANES(l) { lds.flag[l] = (uint32_t)l < nValid && row0 - ((lds.incl[l] - lds.own[l]) & 0xffffu) < traceRows ? 1 : 0; }
			gao::sync();
			const uint64_t kept = gao::ballot(lds.flag);
			gao::sync();
			if (kept)
			{
				const uint32_t l0 = gao::ctz(kept);
				whole_cell(L, lds.cNode[l0], lds.cLen[l0], lds.cCol0[l0], lds.cTop[l0] - ((lds.incl[l0] - lds.own[l0]) >> 16), totalBp);
				first = false;
			}
		}
		GAO_LANES(l)
		{
			uint8_t ch = 0;
			const uint32_t excl = lds.incl[l] - lds.own[l];
			const uint32_t rowA = row0 - (excl & 0xffffu);
			if ((uint32_t)l < nValid && rowA < traceRows)        // cells at rows >= trace_rows are dropped: the first moves of the stream
			{
				// forward: the item describes the cell the move starts in; backward: the cell it leads to
				const int ci = backward ? l + 1 : l;
				const uint32_t cb = backward ? lds.incl[l] >> 16 : excl >> 16;
				const PathCell c = path_cell(L, backward, lds.cNode[ci], lds.cLen[ci], lds.cCol0[ci], lds.cTop[ci] - cb);
				// a column step has a base; a step up has one only where the reference counts it as a diagonal (:742)
				const bool emits = (lds.mv[l] & 3u) != GA_MOVE_UP || (c.len == 1 && gao::self_loop(G, c.node));
				if (emits && path_cell_counts(G, c, totalBp)) ch = WRITE ? path_cell_base(G, c) : 1;
			}
			lds.flag[l] = ch;
		}
		gao::sync();
		const uint64_t emitting = gao::ballot(lds.flag);
		if (WRITE) { GAO_LANES(l) { if ((emitting >> l) & 1) put((uint64_t)emitted + gao::popc(emitting & ((1ull << l) - 1)), lds.flag[l]); } }
		emitted += gao::popc(emitting);
	}

	// behind the last round: the stream's last cell (the only one of a job without moves) is c_0 of a forward job, and of a backward
	// job that kept no move.  Returns the job's count
	GAO_FN uint32_t end(const gao::OpsLaunch& L, uint32_t node, uint32_t len, uint64_t col0, uint32_t off, uint32_t row, uint32_t traceRows, uint64_t totalBp)
	{
		if (row < traceRows && (!backward || first)) whole_cell(L, node, len, col0, off, totalBp);
		return emitted;
	}
};

// one wave's share of a launch: entries wave, wave + nWaves, ... of the job list
template <bool WRITE> GAO_FN void run_wave(const PathLaunch& P, gao::OpsLds& lds, uint32_t wave, uint32_t nWaves)
{
	const gao::OpsLaunch& L = P.walk;
	const uint32_t per = nWaves ? (L.n_jobs + nWaves - 1) / nWaves : 0;
	for (uint32_t k = 0; k < per; k++)
	{
		const uint32_t at = wave + k * nWaves;
		if (at >= L.n_jobs) break;
		const uint32_t job = L.job_list ? L.job_list[at] : at;
		if (job >= L.n_jobs) continue;
		PathSink<WRITE> sink;
		sink.begin(L, P.bases, job, L.fills[job].backward != 0);
		const uint32_t n = gao::walk_job<gao::SINK_PATH>(L, lds, job, sink);
		if (!WRITE) { GAO_LANES(l) { if (l == 0) L.counts[job] = n; } }
		gao::sync();
	}
}

}  // namespace gaps
