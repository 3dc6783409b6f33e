// ga_emul_ops.cpp -- TEST-ONLY (ga_emul.h): GA_F_OPS.  Behind the last pass of a run the operations program of
// graphaligner_amd/csrc/ga_ops.h runs on the host launch by launch: the counting launch for every wave in turn, the exclusive scan as a
// running sum (what replaces the device library's scan here), the writing launch for every wave.  It reads what a batch that built
// its own match words holds: the reads and one GaEqFill per job.  The OpsLds block is filled with 0xA5 once and then kept across all
// jobs of a run, as LDS is.
#include <chrono>
#include <cstdlib>
#include <cstring>

#include "ga_emul.h"
#include "../../graphaligner_amd/csrc/ga_ops.h"

using namespace gae;

namespace {

uint32_t opsWaves()
{
	// (GA_TEST_WAVE_SLOTS as in the product: no launch starts more waves than that)
	const char* e = getenv("GA_TEST_WAVE_SLOTS");
	return e && atoi(e) > 0 ? (uint32_t)atoi(e) : 7u;
}

// the two launches and the scan between them over one set of job records and move bytes
void codeRuns(gao::OpsLaunch L, uint32_t waves, std::vector<uint64_t>& offsets, std::vector<uint32_t>& runs)
{
	gao::OpsLds lds;
	memset(&lds, 0xA5, sizeof(lds));
	std::vector<uint64_t> counts((size_t)L.n_jobs + 1, 0);
	offsets.assign((size_t)L.n_jobs + 1, 0);
	L.counts = counts.data();
	for (uint32_t w = 0; w < waves; w++) gao::run_wave<false>(L, lds, w, waves);
	uint64_t run = 0;
	for (size_t j = 0; j <= L.n_jobs; j++) { offsets[j] = run; run += counts[j]; }
	runs.assign((size_t)run + 1, 0xA5A5A5A5u);
	L.offsets = offsets.data(); L.runs = runs.data();
	for (uint32_t w = 0; w < waves; w++) gao::run_wave<true>(L, lds, w, waves);
}

}  // namespace

void EmulBatch::codeOps()
{
	gao::OpsLaunch L;
	memset(&L, 0, sizeof(L));
	L.graph = g->dev; L.jobs = jobs.data(); L.outs = outs.data(); L.fills = fills.data();
	L.traces = pool.data(); L.trace_bytes = poolTop;
	L.seq = (const uint8_t*)seq; L.seq_bytes = seqBytes; L.row_code = rowCode; L.twin = twin;
	L.n_jobs = (uint32_t)jobs.size();
	const auto t0 = std::chrono::steady_clock::now();
	codeRuns(L, opsWaves(), opsOffsets, opsRuns);
	opsMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	opsJobs = opsMoves = 0;
	for (const GaJobOut& o : outs) if (o.status == GA_OK && o.n_valid > 0 && o.reserved3 != 1) { opsJobs++; opsMoves += o.trace_len; }
}

int EmulBatch::fetchOps(GaOpsOut& out)
{
	if (!cfg.emit_ops) return GaBackendBatch::fetchOps(out);
	out.runs = opsRuns.data(); out.offsets = opsOffsets.data(); out.n_runs = opsOffsets.empty() ? 0 : opsOffsets.back();
	out.count_ms = out.write_ms = opsMs / 2; out.jobs = opsJobs; out.moves = opsMoves;
	return 0;
}

// component hook (tests/test_ops.py): the operations program over a fabricated move stream.  The graph is a chain of nNodes nodes of
// nodeLen bases each (node k+1's only in-neighbour is node k; base i of the chain is "ACGT"[i % 4]) between the two dummy nodes; the
// job starts in the chain's last base at row startRow and walks `moves` (GA_MOVE_* codes, via 0) back.  read: the characters the rows
// are taken from (forward: row r is read[r]; backward: row r is read[traceRows - 1 - r]).  Returns the number of runs written to out
// (capacity cap), or -1.
extern "C" long ga_emul_ops_stream(const uint8_t* moves, uint32_t nMoves, uint32_t nNodes, uint32_t nodeLen, uint32_t startRow, uint32_t traceRows, int backward,
                                   const char* read, uint32_t readLen, uint32_t* out, size_t cap)
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
	GaEqFill fill{0, 0, 0, readLen, (readLen + 63) / 64 * 64, backward ? 1u : 0u};
	uint8_t rowCode[256];
	for (int c = 0; c < 256; c++) rowCode[c] = 0x80;
	rowCode[(uint8_t)'A'] = 1; rowCode[(uint8_t)'C'] = 2; rowCode[(uint8_t)'G'] = 4; rowCode[(uint8_t)'T'] = 8; rowCode[(uint8_t)'N'] = 15;
	std::vector<uint8_t> mv(moves, moves + nMoves);
	mv.resize((size_t)nMoves + 64, 0xA5);
	gao::OpsLaunch L;
	memset(&L, 0, sizeof(L));
	L.graph = dev; L.jobs = &job; L.outs = &o; L.fills = &fill; L.traces = mv.data(); L.trace_bytes = nMoves;
	L.seq = (const uint8_t*)read; L.seq_bytes = readLen; L.row_code = rowCode; L.n_jobs = 1;
	std::vector<uint64_t> offsets;
	std::vector<uint32_t> runs;
	codeRuns(L, 1, offsets, runs);
	const uint64_t nRuns = offsets[1];
	if (nRuns > cap) return -1;
	for (uint64_t i = 0; i < nRuns; i++) out[i] = runs[i];
	return (long)nRuns;
}
