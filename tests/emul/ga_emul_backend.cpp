// ga_emul_backend.cpp -- TEST-ONLY (ga_emul.h): the graph and the batch of the host emulation, the GA_EMUL_WITHOUT switch and the
// match words.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "ga_emul.h"

using namespace gae;

namespace {

// "words" implies "ops" (the operations program reads what a batch that builds its own words holds); "seeding" leaves no engine to
// withhold "walks", "loci" and "topology" from, and no seeds for "seeded"
bool parseWithout(const char* list, uint32_t& bits)
{
	static const struct { const char* name; uint32_t bits; } kNames[] = {
		{"wide", NO_WIDE}, {"wide_sparse", NO_WIDE_SPARSE}, {"words", NO_WORDS | NO_OPS}, {"ops", NO_OPS},
		{"seeding", NO_SEEDING | NO_WALKS | NO_LOCI | NO_TOPOLOGY | NO_SEEDED}, {"walks", NO_WALKS}, {"loci", NO_LOCI}, {"topology", NO_TOPOLOGY}, {"seeded", NO_SEEDED}};
	bits = 0;
	const std::string s = list ? list : "";
	for (size_t at = 0; at < s.size(); )
	{
		const size_t end = std::min(s.find(',', at), s.size());
		const std::string word = s.substr(at, end - at);
		bool known = word.empty();
		for (const auto& n : kNames) if (word == n.name) { bits |= n.bits; known = true; }
		if (!known) { fprintf(stderr, "emul: GA_EMUL_WITHOUT: no capability named '%s'\n", word.c_str()); return false; }
		at = end + 1;
	}
	return true;
}

// test hook (tests/test_alphabet.py): what the host's two builders made for the batch created last -- the match words of
// ga_batch_prepare and the row codes of buildRows -- kept only while the hook is switched on
bool keepTables = false;
std::vector<uint64_t> keptEq;
std::vector<uint8_t> keptRows;
std::vector<uint64_t> keptJobs;      // per job: rows_off, n_rows

}  // namespace

extern "C" void ga_emul_keep_tables(int on) { keepTables = on != 0; keptEq.clear(); keptRows.clear(); keptJobs.clear(); }
extern "C" void ga_emul_kept_sizes(uint64_t* out) { out[0] = keptEq.size(); out[1] = keptRows.size(); out[2] = keptJobs.size() / 2; }
extern "C" void ga_emul_kept_copy(uint64_t* eq, uint8_t* rows, uint64_t* jobs)
{
	std::copy(keptEq.begin(), keptEq.end(), eq);
	std::copy(keptRows.begin(), keptRows.end(), rows);
	std::copy(keptJobs.begin(), keptJobs.end(), jobs);
}

void EmulBatch::buildWords(const GaEqSource& src, size_t eqWords)
{
	ownWords = true;
	fills.assign(src.fills, src.fills + src.nFills);
	seq = src.seq; seqBytes = src.seqBytes; twin = src.twin;
	memcpy(rowCode, src.rowCode, 256);
	eq.assign(eqWords, 0);
	bad.assign(src.nFills, 0);
	for (size_t k = 0; k < src.nFills; k++)
	{
		const GaEqFill& f = src.fills[k];
		const uint8_t* s = (const uint8_t*)src.seq + f.seq_off;
		for (uint32_t r0 = 0; r0 < f.padded; r0 += 64)
		{
			uint8_t buf[64];
			for (uint32_t i = 0; i < 64; i++)
			{
				const uint32_t r = r0 + i;
				buf[i] = r < f.n ? (f.backward ? src.rowCodeRc[s[f.n - 1 - r]] : src.rowCode[s[f.pos + r]]) : src.padCode;
			}
			uint64_t* words = eq.data() + (f.eq_slice + r0 / 64) * 5;
			ga_build_eq_words(buf, 64, words);
			if (words[4] & 8u) bad[k] = 1;
		}
	}
}

int EmulBatch::finishSeeded(const std::vector<GaJob>& jobsIn, const GaRunConfig& c, GaRowsProvider r, const uint64_t* eqIn, size_t eqWords)
{
	if (!seeded) return GaBackendBatch::finishSeeded(jobsIn, c, r, eqIn, eqWords);
	jobs = jobsIn;
	cfg = c;
	rowsProvider = r;
	if (!ownWords) eq.assign(eqIn, eqIn + eqWords);
	for (uint8_t f : bad) if (f) { cfg.emit_runs = 0; break; }
	return 0;
}

GaBackendGraph* ga_backend_upload_graph(const GaFlatGraph& flat, const GaHmmTables& hmm, int, int* status)
{
	uint32_t without = 0;
	if (!parseWithout(getenv("GA_EMUL_WITHOUT"), without)) { *status = 100; return nullptr; }
	EmulGraph* g = new EmulGraph();
	g->without = without;
	g->flat = flat;
	g->hmm = hmm;
	g->dev.n_nodes = (uint32_t)(flat.node_start.size() - 1);
	g->dev.reserved = 0;
	g->dev.node_start = g->flat.node_start.data();
	g->dev.seq2 = g->flat.seq2.data();
	g->dev.in_off = g->flat.in_off.data();
	g->dev.in_nbr = g->flat.in_nbr.data();
	g->dev.out_off = g->flat.out_off.data();
	g->dev.out_nbr = g->flat.out_nbr.data();
	g->nodeRec = ga_build_node_records(g->flat);
	g->dev.node_rec = g->nodeRec.data();
	if (!(g->without & NO_SEEDING)) g->seed.reset(newSeedEngine(&g->dev, g->without));
	*status = 0;
	return g;
}

GaBackendBatch* ga_backend_create_batch(GaBackendGraph* graph, GaRowsProvider rows, const uint64_t* eq, const GaEqSource* src, size_t eqWords, const std::vector<GaJob>& jobs,
                                        const GaRunConfig& cfg, int* status)
{
	EmulGraph* g = static_cast<EmulGraph*>(graph);
	if (g->buildsMatchWords() && !src) { *status = 100; return nullptr; }
	EmulBatch* b = new EmulBatch();
	b->g = g;
	b->rowsProvider = rows;
	b->jobs = jobs;
	b->cfg = cfg;
	if (g->buildsMatchWords())
	{
		b->buildWords(*src, eqWords);
		for (uint8_t f : b->bad) if (f) { b->cfg.emit_runs = 0; break; }
	}
	else b->eq.assign(eq, eq + eqWords);
	if (keepTables)
	{
		keptEq = b->eq;
		keptRows = rows();
		keptJobs.clear();
		for (const GaJob& j : jobs) { keptJobs.push_back(j.rows_off); keptJobs.push_back(j.n_rows); }
	}
	*status = 0;
	return b;
}
