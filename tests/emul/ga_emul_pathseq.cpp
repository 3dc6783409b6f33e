// ga_emul_pathseq.cpp -- TEST-ONLY: the path-sequence program of graphaligner_amd/csrc/ga_pathseq.h compiled for the host with GA_EMULATE,
// launch by launch, behind a component hook for tests/test_pathseq.py.  A small library of its own (tests/emul/pathseq.mk ->
// tests/_build/libga_pathseq_emul.so), like ga_emul_edges.cpp: the host emulation of the back end writes no path sequences.  The bytes are
// the caller's buffer itself, so that a store outside a job's place lands in the guard bytes the caller put around it.  The OpsLds
// block is filled with 0xA5 once and then kept across both launches, as LDS is.  Never shipped, never loaded by graphaligner_amd/.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../graphaligner_amd/csrc/ga_pathseq.h"

// component hook: the program over a fabricated move stream.  The graph is the chain of ga_emul_ops_stream (tests/emul/ga_emul_ops.cpp):
// nNodes nodes of nodeLen bases each, node k+1's only in-neighbour node k, base i of the chain "ACGT"[i % 4], between the two dummy
// nodes; the job starts in the chain's last base at row startRow and walks `moves` (GA_MOVE_* codes, via 0) back.  No twin table, as
// there: a backward job's bases are the cells' own, complemented.  out: `cap` bytes, which the caller pre-fills and surrounds with guard
// bytes; the counting launch, a running sum and the writing launch run, and the job's bytes are written at out[0 ..).  Returns their
// number, -1 when it exceeds cap (nothing is written then).
extern "C" long ga_emul_pathseq_stream(const uint8_t* moves, uint32_t nMoves, uint32_t nNodes, uint32_t nodeLen, uint32_t startRow, uint32_t traceRows, int backward,
                                       uint8_t* out, size_t cap)
{
	GaFlatGraph f;
	const uint32_t n = nNodes + 2;
	f.node_start.resize(n + 1);
	f.node_start[0] = 0; f.node_start[1] = 1;
	for (uint32_t k = 0; k < nNodes; k++) f.node_start[k + 2] = f.node_start[k + 1] + nodeLen;
	f.node_start[n] = f.node_start[n - 1] + 1;
	const uint64_t bp = f.node_start[n];
	f.seq2.assign((bp + 15) / 16 + 8, 0);
	for (uint64_t i = 1; i + 1 < bp; i++) f.seq2[i >> 4] |= (uint32_t)((i - 1) & 3) << ((i & 15) * 2);
	f.in_off.assign(n + 1, 0); f.out_off.assign(n + 1, 0);
	for (uint32_t k = 0; k < n; k++)
	{
		// (the chain's first node takes the start dummy as in-neighbour, so that a stream may walk off the chain's front)
		const bool hasIn = k >= 1 && k + 1 < n, hasOut = k + 2 < n;
		f.in_off[k + 1] = f.in_off[k] + (hasIn ? 1 : 0);
		if (hasIn) f.in_nbr.push_back(k - 1);
		f.out_off[k + 1] = f.out_off[k] + (hasOut ? 1 : 0);
		if (hasOut) f.out_nbr.push_back(k + 1);
	}
	f.in_nbr.push_back(0); f.out_nbr.push_back(0);
	std::vector<uint32_t> rec = ga_build_node_records(f);
	GaDevGraph dev;
	dev.n_nodes = n; dev.reserved = 0;
	dev.node_start = f.node_start.data(); dev.seq2 = f.seq2.data(); dev.in_off = f.in_off.data(); dev.in_nbr = f.in_nbr.data();
	dev.out_off = f.out_off.data(); dev.out_nbr = f.out_nbr.data(); dev.node_rec = rec.data();
	GaJob job{0, (traceRows + 63) / 64 * 64, nNodes, traceRows, 0};
	GaJobOut o;
	memset(&o, 0, sizeof(o));
	o.status = GA_OK; o.n_valid = 1; o.trace_len = nMoves; o.trace_off = 0;
	o.start_node = nNodes; o.start_offset = nodeLen - 1; o.start_row = startRow;
	GaEqFill fill{0, 0, 0, traceRows, (traceRows + 63) / 64 * 64, backward ? 1u : 0u};
	gaps::PathLaunch P;
	memset(&P, 0, sizeof(P));
	gao::OpsLaunch& L = P.walk;
	L.graph = dev; L.jobs = &job; L.outs = &o; L.fills = &fill; L.n_jobs = 1;
	L.traces = moves; L.trace_bytes = nMoves;                 // (the caller's bytes themselves, nothing behind them; no reads, no row codes)
	gao::OpsLds lds;
	memset(&lds, 0xA5, sizeof(lds));
	uint64_t counts[2] = {0, 0}, offsets[2] = {0, 0};
	L.counts = counts;
	gaps::run_wave<false>(P, lds, 0, 1);
	offsets[1] = counts[0];
	if (counts[0] > cap) return -1;
	L.offsets = offsets; P.bases = out;
	gaps::run_wave<true>(P, lds, 0, 1);
	return (long)counts[0];
}
