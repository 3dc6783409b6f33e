// ga_emul_edges.cpp -- TEST-ONLY: the edge-support program of graphaligner_amd/csrc/ga_edges.h compiled for the host with GA_EMULATE,
// wave by wave, with plain adds where the device has atomics, behind component hooks for tests/test_edge_pileup.py.  A small library of
// its own (tests/emul/edges.mk -> tests/_build/libga_edges_emul.so), like ga_emul_pileup.cpp: the host emulation of the back end has no
// pileups.  The counters are the caller's buffer itself -- filled with a poison value, then the pileup's own reset of its entries -- so
// that a store past the entries lands in the words the caller put behind them.  The OpsLds block is filled with 0xA5 once per launch
// and then kept across its jobs, as LDS is.  Never shipped, never loaded by graphaligner_amd/.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../graphaligner_amd/csrc/ga_edges.h"

namespace {

// a graph from in-lists: node k has nodeLen[k] bases (all A), in-neighbours inNbr[inOff[k] .. inOff[k + 1]); the out-lists follow
bool flatFromInLists(uint32_t n, const uint32_t* nodeLen, const uint32_t* inOff, const uint32_t* inNbr, GaFlatGraph& f)
{
	if (n < 2 || inOff[0] != 0) return false;
	f.node_start.assign(n + 1, 0);
	for (uint32_t k = 0; k < n; k++) { if (!nodeLen[k] || inOff[k + 1] < inOff[k]) return false; f.node_start[k + 1] = f.node_start[k] + nodeLen[k]; }
	f.seq2.assign((f.node_start[n] + 15) / 16 + 8, 0);
	f.in_off.assign(inOff, inOff + n + 1);
	f.in_nbr.assign(inNbr, inNbr + inOff[n]);
	for (uint32_t m : f.in_nbr) if (m >= n) return false;
	f.out_off.assign(n + 1, 0);
	for (uint32_t m : f.in_nbr) f.out_off[m + 1]++;
	for (uint32_t k = 0; k < n; k++) f.out_off[k + 1] += f.out_off[k];
	f.out_nbr.assign(inOff[n], 0);
	std::vector<uint32_t> at(f.out_off.begin(), f.out_off.end() - 1);
	for (uint32_t to = 0; to < n; to++) for (uint32_t e = inOff[to]; e < inOff[to + 1]; e++) f.out_nbr[at[inNbr[e]]++] = to;
	f.in_nbr.push_back(0); f.out_nbr.push_back(0);            // (slack, as the product's lists have)
	return true;
}

}  // namespace

// the mirror-slot table the host library builds for a pileup of the EDGES kind (ga_backend.h: ga_edge_mirror_slots), over a graph given
// as in-lists.  mirror: inOff[n] words.  Returns the slot count, or -1.
extern "C" long ga_emul_edges_mirror(uint32_t n, const uint32_t* nodeLen, const uint32_t* inOff, const uint32_t* inNbr, const uint32_t* twin, uint32_t* mirror)
{
	GaFlatGraph f;
	if (!flatFromInLists(n, nodeLen, inOff, inNbr, f)) return -1;
	f.in_nbr.pop_back();
	const std::vector<uint32_t> m = ga_edge_mirror_slots(f, std::vector<uint32_t>(twin, twin + n));
	if (m.size() != inOff[n] || ga_edge_slot_count(f) != inOff[n]) return -1;
	std::copy(m.begin(), m.end(), mirror);
	return (long)m.size();
}

// component hook (tests/test_edge_pileup.py): the program over a fabricated move stream and a small graph given as in-lists (n nodes,
// the two dummy nodes 0 and n - 1 included; twin[k] = the node of the other strand or 0xffffffff).  The job starts in (startNode,
// startOffset) at row startRow and walks `moves` back.  counts: the pileup's own words, `entries` of them = inOff[n], which the caller
// may follow with guard words.  Returns the crossings added, or -1.
extern "C" long ga_emul_edges_stream(const uint8_t* moves, uint32_t nMoves, uint32_t n, const uint32_t* nodeLen, const uint32_t* inOff, const uint32_t* inNbr,
                                     const uint32_t* twin, uint32_t startNode, uint32_t startOffset, uint32_t startRow, uint32_t traceRows, int backward,
                                     uint32_t* counts, uint64_t entries)
{
	GaFlatGraph f;
	if (!flatFromInLists(n, nodeLen, inOff, inNbr, f) || entries != inOff[n] || startNode >= n) return -1;
	std::vector<uint32_t> rec = ga_build_node_records(f);
	f.in_nbr.pop_back();
	std::vector<uint32_t> mirror = ga_edge_mirror_slots(f, std::vector<uint32_t>(twin, twin + n));
	f.in_nbr.push_back(0);
	mirror.push_back(0xffffffffu);
	GaDevGraph dev;
	dev.n_nodes = n; dev.reserved = 0;
	dev.node_start = f.node_start.data(); dev.seq2 = f.seq2.data(); dev.in_off = f.in_off.data(); dev.in_nbr = f.in_nbr.data();
	dev.out_off = f.out_off.data(); dev.out_nbr = f.out_nbr.data(); dev.node_rec = rec.data();
	GaJob job{0, (traceRows + 63) / 64 * 64, startNode, traceRows, 0};
	GaJobOut o;
	memset(&o, 0, sizeof(o));
	o.status = GA_OK; o.n_valid = 1; o.trace_len = nMoves; o.trace_off = 0;
	o.start_node = startNode; o.start_offset = startOffset; o.start_row = startRow;
	GaEqFill fill{0, 0, 0, traceRows, (traceRows + 63) / 64 * 64, backward ? 1u : 0u};
	std::fill(counts, counts + entries, 0xA5A5A5A5u);
	std::fill(counts, counts + entries, 0u);                  // (the pileup's reset: its entries and nothing else)
	const uint32_t list[1] = {0u | gapl::kCounts};
	gaed::EdgesLaunch P;
	memset(&P, 0, sizeof(P));
	gao::OpsLaunch& L = P.walk;
	L.graph = dev; L.jobs = &job; L.outs = &o; L.fills = &fill; L.n_jobs = 1;
	L.traces = moves; L.trace_bytes = nMoves;                 // (the caller's bytes themselves, nothing behind them)
	P.counts = counts; P.mirror = mirror.data(); P.entries = entries; P.list = list; P.n_list = 1;
	unsigned long long added = 0;
	P.added = &added;
	gao::OpsLds lds;
	memset(&lds, 0xA5, sizeof(lds));
	gaed::run_wave(P, lds, 0, 1);
	return (long)added;
}
