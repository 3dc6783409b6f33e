// ga_backend_ops_emul.cpp -- TEST-ONLY back end for GA_F_OPS: the newest alignment emulation (tests/emul_wide_sparse, compiled into this
// file as it is) and behind its run() the operations program of graphaligner_amd/csrc/ga_ops.h run on the host launch by launch: the
// counting launch for every wave in turn, the exclusive scan as a running sum (what replaces the device library's scan here), the
// writing launch for every wave.  Like the product it builds the match words itself from the batch's copy of the reads
// (GaBackendGraph::buildsMatchWords), so that it holds what the operations program reads: the reads and one GaEqFill per job.  The
// OpsLds block is filled with 0xA5 once and then kept across all jobs of a run, as LDS is.  The older host builds stay as they are
// and refuse a prepare with GA_F_OPS; this one has no seeding (ga_batch_prepare_seeded is refused).
// Linked only into tests/_build/libga_ops_emul.so, next to the product's host code (ga_host.cpp, ga_vgio.cpp).
#include <chrono>

#include "../../graphaligner_amd/csrc/ga_backend.h"

#define ga_backend_upload_graph ga_align_part_upload_graph
#define ga_backend_create_batch ga_align_part_create_batch
#include "../emul_wide_sparse/ga_backend_wide_sparse_emul.cpp"
#undef ga_backend_upload_graph
#undef ga_backend_create_batch

#include "../../graphaligner_amd/csrc/ga_ops.h"

GaBackendGraph* ga_backend_upload_graph(const GaFlatGraph& g, const GaHmmTables& hmm, int device, int* status);
GaBackendBatch* ga_backend_create_batch(GaBackendGraph* g, GaRowsProvider rows, const uint64_t* eq, const GaEqSource* src, size_t eqWords, const std::vector<GaJob>& jobs,
                                        const GaRunConfig& cfg, int* status);

namespace {

uint32_t opsWaves()
{
	// (GA_TEST_WAVE_SLOTS as in the product: no launch starts more waves than that)
	const char* e = getenv("GA_TEST_WAVE_SLOTS");
	return e && atoi(e) > 0 ? (uint32_t)atoi(e) : 7u;
}

// the two launches and the scan between them over one set of job records and move bytes
struct OpsRun
{
	std::vector<uint64_t> counts, offsets;
	std::vector<uint32_t> runs;
	gao::OpsLds lds;
	OpsRun() { memset(&lds, 0xA5, sizeof(lds)); }
	void go(gao::OpsLaunch L, uint32_t waves)
	{
		counts.assign((size_t)L.n_jobs + 1, 0);
		offsets.assign((size_t)L.n_jobs + 1, 0);
		L.counts = counts.data();
		for (uint32_t w = 0; w < waves; w++) gao::run_wave<false>(L, lds, w, waves);
		uint64_t run = 0;
		for (size_t j = 0; j <= L.n_jobs; j++) { offsets[j] = run; run += counts[j]; }
		runs.assign((size_t)run + 1, 0xA5A5A5A5u);
		L.offsets = offsets.data(); L.runs = runs.data();
		for (uint32_t w = 0; w < waves; w++) gao::run_wave<true>(L, lds, w, waves);
	}
};

struct OpsGraph : GaBackendGraph
{
	GaFlatGraph flat;
	std::vector<uint32_t> nodeRec;
	GaDevGraph dev;
	std::unique_ptr<GaBackendGraph> inner;
	bool buildsMatchWords() const override { return true; }
	bool codesOps() const override { return true; }
};

struct OpsBatch : GaBackendBatch
{
	OpsGraph* g = nullptr;
	std::unique_ptr<GaBackendBatch> inner;
	GaRunConfig cfg;
	std::vector<GaJob> jobs;
	std::vector<GaEqFill> fills;
	std::vector<uint64_t> eq;
	std::vector<uint8_t> bad;
	const char* seq = nullptr; size_t seqBytes = 0;
	const uint32_t* twin = nullptr;
	uint8_t rowCode[256];
	bool ownWords = false;
	OpsRun ops;
	uint64_t opsJobs = 0, opsMoves = 0;
	double countMs = 0, writeMs = 0;

	const std::vector<uint8_t>* invalidFills() const override { return ownWords ? &bad : nullptr; }
	bool emittingRuns() const override { return inner->emittingRuns(); }
	int run() override
	{
		int s = inner->run();
		if (s || !cfg.emit_ops) return s;
		std::vector<GaJobOut> outs;
		const uint8_t* traces = nullptr; uint64_t nBytes = 0;
		if ((s = inner->fetch(outs, &traces, &nBytes))) return s;
		gao::OpsLaunch L;
		memset(&L, 0, sizeof(L));
		L.graph = g->dev; L.jobs = jobs.data(); L.outs = outs.data(); L.fills = fills.data();
		L.traces = traces; L.trace_bytes = nBytes;
		L.seq = (const uint8_t*)seq; L.seq_bytes = seqBytes; L.row_code = rowCode; L.twin = twin;
		L.n_jobs = (uint32_t)jobs.size();
		const auto t0 = std::chrono::steady_clock::now();
		ops.go(L, opsWaves());
		countMs = writeMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / 2;
		opsJobs = opsMoves = 0;
		for (const GaJobOut& o : outs) if (o.status == GA_OK && o.n_valid > 0 && o.reserved3 != 1) { opsJobs++; opsMoves += o.trace_len; }
		inner->fetchDone();
		return 0;
	}
	int fetch(std::vector<GaJobOut>& outs, const uint8_t** traceBytes, uint64_t* nBytes) override { return inner->fetch(outs, traceBytes, nBytes); }
	int fetchOps(GaOpsOut& out) override
	{
		if (!cfg.emit_ops) return 100;
		out.runs = ops.runs.data(); out.offsets = ops.offsets.data(); out.n_runs = ops.offsets.empty() ? 0 : ops.offsets.back();
		out.count_ms = countMs; out.write_ms = writeMs; out.jobs = opsJobs; out.moves = opsMoves;
		return 0;
	}
	void fetchDone() override { inner->fetchDone(); }
	GaRunStats stats() const override { return inner->stats(); }
};

}  // namespace

GaBackendGraph* ga_backend_upload_graph(const GaFlatGraph& flat, const GaHmmTables& hmm, int device, int* status)
{
	OpsGraph* g = new OpsGraph();
	g->flat = flat;
	g->inner.reset(ga_align_part_upload_graph(flat, hmm, device, status));
	if (!g->inner) { delete g; if (!*status) *status = 102; return nullptr; }
	g->dev.n_nodes = (uint32_t)(flat.node_start.size() - 1);
	g->dev.reserved = 0;
	g->dev.node_start = g->flat.node_start.data(); g->dev.seq2 = g->flat.seq2.data();
	g->dev.in_off = g->flat.in_off.data(); g->dev.in_nbr = g->flat.in_nbr.data();
	g->dev.out_off = g->flat.out_off.data(); g->dev.out_nbr = g->flat.out_nbr.data();
	g->nodeRec = ga_build_node_records(g->flat);
	g->dev.node_rec = g->nodeRec.data();
	*status = 0;
	return g;
}

GaBackendBatch* ga_backend_create_batch(GaBackendGraph* graph, GaRowsProvider rows, const uint64_t* eq, const GaEqSource* src, size_t eqWords, const std::vector<GaJob>& jobs,
                                        const GaRunConfig& cfg, int* status)
{
	OpsGraph* g = static_cast<OpsGraph*>(graph);
	if (!src) { *status = 100; return nullptr; }
	std::unique_ptr<OpsBatch> b(new OpsBatch());
	b->g = g; b->cfg = cfg; b->jobs = jobs; b->ownWords = true;
	b->fills.assign(src->fills, src->fills + src->nFills);
	b->seq = src->seq; b->seqBytes = src->seqBytes; b->twin = src->twin;
	memcpy(b->rowCode, src->rowCode, 256);
	// the match words, as ga_eq_words_kernel builds them: 64 row codes at a time
	b->eq.assign(eqWords, 0);
	b->bad.assign(src->nFills, 0);
	for (size_t k = 0; k < src->nFills; k++)
	{
		const GaEqFill& f = src->fills[k];
		const uint8_t* s = (const uint8_t*)src->seq + f.seq_off;
		for (uint32_t r0 = 0; r0 < f.padded; r0 += 64)
		{
			uint8_t buf[64];
			for (uint32_t i = 0; i < 64; i++)
			{
				const uint32_t r = r0 + i;
				buf[i] = r < f.n ? (f.backward ? src->rowCodeRc[s[f.n - 1 - r]] : src->rowCode[s[f.pos + r]]) : src->padCode;
			}
			uint64_t* words = b->eq.data() + (f.eq_slice + r0 / 64) * 5;
			ga_build_eq_words(buf, 64, words);
			if (words[4] & 8u) b->bad[k] = 1;
		}
	}
	for (uint8_t f : b->bad) if (f) { b->cfg.emit_runs = 0; break; }
	b->inner.reset(ga_align_part_create_batch(g->inner.get(), rows, b->eq.data(), nullptr, eqWords, jobs, b->cfg, status));
	if (!b->inner) return nullptr;
	*status = 0;
	return b.release();
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
	OpsRun run;
	run.go(L, 1);
	const uint64_t nRuns = run.offsets[1];
	if (nRuns > cap) return -1;
	for (uint64_t i = 0; i < nRuns; i++) out[i] = run.runs[i];
	return (long)nRuns;
}
