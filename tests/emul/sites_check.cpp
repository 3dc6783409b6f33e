// sites_check.cpp -- TEST-ONLY, stand-alone: a main of its own over the host code of site queries, so that it can be built with
// -fsanitize=address,undefined and run as it is (tests/emul/sites.mk, target `check`; nothing is loaded into another program).  It
// links the product's host code (ga_host.cpp) against the stub back end of ga_emul_sites.cpp, whose pileups live in host memory and
// whose sites() is the program of ga_sites.h compiled with GA_EMULATE over tables of exactly their sizes, and goes through
//   params validation (every refusal the header names), the fold table and its precondition check (overlap, twin of another length,
//   twin that is not the reverse complement, one strand), queries of all three kinds folded and unfolded against a replay written
//   here, the records' fields, caps, ranges, and ga_sites_free (null included).
// Exit status 0 and a line of totals when everything agrees.
#include <cstdio>
#include <string>

#include "ga_emul_sites.cpp"
#include "../../include/graphaligner_amd.h"

namespace {

int failures = 0;
unsigned long long queries = 0, sitesSeen = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; fprintf(stderr, "line %d: ", __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

uint32_t rnd(uint64_t& s) { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }

std::string revcomp(const std::string& s)
{
	std::string r(s.rbegin(), s.rend());
	for (char& c : r) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A';
	return r;
}

ga_site_params_t params(uint32_t flags, uint64_t minDepth, uint64_t minAlt, uint32_t num, uint32_t den, uint64_t first, uint64_t n, uint64_t cap)
{
	ga_site_params_t q;
	memset(&q, 0, sizeof(q));
	q.flags = flags; q.min_depth = minDepth; q.min_alt = minAlt; q.alt_num = num; q.alt_den = den; q.first_entry = first; q.n_entries = n; q.max_sites = cap;
	return q;
}

bool refused(ga_pileup_t* p, const ga_site_params_t& q)
{
	ga_sites_t* out = (ga_sites_t*)(uintptr_t)1;
	const int rc = ga_pileup_sites(p, &q, &out);
	return rc == GA_E_INVALID && out == nullptr;
}

// a chain of bigraph nodes, the counters of every kind set to small random numbers, every query replayed entry by entry
void checkChain(const std::vector<size_t>& lens, uint64_t seed)
{
	ga_graph_t* g = ga_graph_create();
	std::vector<std::string> seqs;
	for (size_t k = 0; k < lens.size(); k++)
	{
		std::string s(lens[k], 'A');
		for (char& c : s) c = "ACGT"[rnd(seed) & 3];
		seqs.push_back(s);
		CHECK(ga_graph_add_bigraph_node(g, (int64_t)k + 1, s.data(), s.size()) == GA_S_OK, "node");
		if (k) CHECK(ga_graph_add_bigraph_edge(g, (int64_t)k, 0, (int64_t)k + 1, 0) == GA_S_OK, "edge");
	}
	CHECK(ga_graph_finalize(g, 0) == GA_S_OK && ga_graph_upload(g, 0) == GA_S_OK, "finalize and upload");
	// the columns: dummy, then every node's forward and reverse copy, dummy
	std::string text = "-";
	std::vector<uint64_t> start{0};
	std::vector<int64_t> ids{0};
	for (size_t k = 0; k < seqs.size(); k++)
		for (int r = 0; r < 2; r++) { start.push_back(text.size()); ids.push_back(2 * ((int64_t)k + 1) + r); text += r ? revcomp(seqs[k]) : seqs[k]; }
	start.push_back(text.size()); ids.push_back(0);
	text += "-";
	start.push_back(text.size());
	const uint64_t columns = text.size();
	CHECK((uint64_t)ga_graph_bp(g) == columns, "columns");
	for (int kind : {GA_PILEUP_BASES, GA_PILEUP_DEPTH})
	{
		const uint32_t K = kind == GA_PILEUP_BASES ? 8 : 1;
		ga_pileup_t* p = nullptr;
		CHECK(ga_pileup_create(g, kind, &p) == GA_S_OK && p, "pileup");
		if (!p) continue;
		std::vector<uint32_t> P((size_t)K * columns, 0);
		for (uint32_t k = 0; k < K; k++) for (uint64_t c = 1; c + 1 < columns; c++) P[k * columns + c] = rnd(seed) % 5 == 0 ? 0 : rnd(seed) % 4;
		P[1 % K * columns + 1] = 0xffffffffu;                   // (a sum that wraps)
		CHECK(ga_emul_sites_poke(p, P.data(), P.size()) == 0, "poke");
		for (uint32_t fold = 0; fold < 2; fold++)
			for (uint64_t minDepth : {(uint64_t)1, (uint64_t)3})
				for (uint64_t minAlt : {(uint64_t)0, (uint64_t)1})
					for (uint32_t num : {0u, 1u})
					{
						const uint64_t first = fold ? 2 : 0, n = columns - first - (minAlt ? 3 : 0), cap = minDepth == 3 ? 4 : 0;
						const ga_site_params_t q = params(fold, minDepth, minAlt, num, 4, first, n, cap);
						ga_sites_t* out = nullptr;
						CHECK(ga_pileup_sites(p, &q, &out) == GA_S_OK && out, "query");
						if (!out) continue;
						queries++;
						uint64_t found = 0;
						for (uint64_t c = first; c < first + n; c++)
						{
							size_t node = 0;
							while (start[node + 1] <= c) node++;
							uint32_t F[8] = {0, 0, 0, 0, 0, 0, 0, 0};
							if (!fold) for (uint32_t k = 0; k < K; k++) F[k] = P[k * columns + c];
							else
							{
								if (node == 0 || node + 1 == ids.size() || (ids[node] & 1)) continue;
								const uint64_t len = start[node + 1] - start[node], c2 = start[node + 1] + len - 1 - (c - start[node]);
								for (uint32_t k = 0; k < K; k++) F[k] = P[k * columns + c] + P[(k >= 1 && k <= 4 ? 5 - k : k) * columns + c2];
							}
							uint64_t D = F[0], X = 0;
							if (K == 8) { for (int k = 1; k < 7; k++) D += F[k]; X = std::max<uint64_t>(D - F[0], F[7]); }
							if (!(D >= minDepth && X >= minAlt && X * 4 >= (uint64_t)num * D)) continue;
							if (found < out->n_sites)
							{
								const ga_site_t& s = out->sites[found];
								CHECK(s.entry == c && memcmp(s.counts, F, sizeof(F)) == 0, "kind %d fold %u: site %llu", kind, fold, (unsigned long long)found);
								CHECK(s.node_id == ids[node] / 2 && s.reverse == (ids[node] & 1) && s.offset == c - start[node] && s.graph_char == text[c], "the record's place");
							}
							found++;
						}
						CHECK(out->n_total == found && out->n_sites == (cap ? std::min(cap, found) : found) && out->entries_scanned == n, "totals: %llu of %llu", (unsigned long long)out->n_sites,
						      (unsigned long long)found);
						sitesSeen += out->n_sites;
						ga_sites_free(out);
					}
		// refusals: every constraint of the header, and what lies exactly on it
		CHECK(refused(p, params(0, 0, 0, 0, 1, 0, columns, 0)), "min_depth 0");
		CHECK(refused(p, params(0, 1, 0, 0, 0, 0, columns, 0)), "alt_den 0");
		CHECK(refused(p, params(0, 1, 0, 0, 65536, 0, columns, 0)), "alt_den above 65535");
		CHECK(refused(p, params(0, 1, 0, 3, 2, 0, columns, 0)), "alt_num above alt_den");
		CHECK(refused(p, params(2, 1, 0, 0, 1, 0, columns, 0)), "a flag that is none");
		CHECK(refused(p, params(0, 1, 0, 0, 1, 0, columns + 1, 0)), "range past the entries");
		CHECK(refused(p, params(0, 1, 0, 0, 1, columns + 1, 0, 0)), "range behind the entries");
		CHECK(refused(p, params(0, 1, 0, 0, 1, 1, ~(uint64_t)0, 0)), "range that wraps");
		ga_sites_t* out = nullptr;
		ga_site_params_t q = params(GA_SITES_FOLD, 1, 0, 65535, 65535, columns, 0, 0);
		CHECK(ga_pileup_sites(p, &q, &out) == GA_S_OK && out && out->n_sites == 0 && out->n_total == 0 && out->sites == nullptr, "an empty range at the end");
		ga_sites_free(out);
		CHECK(ga_pileup_sites(nullptr, &q, &out) == GA_E_INVALID && ga_pileup_sites(p, nullptr, &out) == GA_E_INVALID && ga_pileup_sites(p, &q, nullptr) == GA_E_INVALID, "null arguments");
		ga_pileup_free(p);
	}
	// edge slots: the folded query against the sum over the slot table
	uint64_t nSlots = 0;
	CHECK(ga_graph_edge_slot_count(g, &nSlots) == GA_S_OK, "slots");
	ga_pileup_t* p = nullptr;
	CHECK(ga_pileup_create(g, GA_PILEUP_EDGES, &p) == GA_S_OK && p, "pileup of edges");
	if (p && nSlots)
	{
		std::vector<int64_t> from(nSlots), to(nSlots);
		CHECK(ga_graph_edge_slots(g, 0, nSlots, from.data(), to.data()) == GA_S_OK, "slot table");
		std::vector<uint32_t> cnt(nSlots);
		for (uint32_t& c : cnt) c = rnd(seed) % 3;
		CHECK(ga_emul_sites_poke(p, cnt.data(), cnt.size()) == 0, "poke");
		for (uint64_t t : {(uint64_t)1, (uint64_t)2, (uint64_t)4})
		{
			ga_site_params_t q = params(GA_SITES_FOLD, t, 0, 0, 1, 0, nSlots, 0);
			ga_sites_t* out = nullptr;
			CHECK(ga_pileup_sites(p, &q, &out) == GA_S_OK && out, "edge query");
			if (!out) continue;
			queries++;
			uint64_t found = 0;
			for (uint64_t s = 0; s < nSlots; s++)
			{
				uint64_t m = nSlots;
				for (uint64_t k = 0; k < nSlots; k++) if (from[k] == (to[s] ^ 1) && to[k] == (from[s] ^ 1)) m = k;
				if (from[s] == 0 || to[s] == 0) m = nSlots;          // (an edge of a dummy node has no mirror)
				if (m < s) continue;
				const uint32_t F = cnt[s] + (m < nSlots && m != s ? cnt[m] : 0);
				if (F < t) continue;
				if (found < out->n_sites) CHECK(out->sites[found].entry == s && out->sites[found].counts[0] == F && out->sites[found].from_id == from[s] && out->sites[found].to_id == to[s], "edge site");
				found++;
			}
			CHECK(out->n_total == found && out->n_sites == found, "edge totals");
			sitesSeen += out->n_sites;
			ga_sites_free(out);
		}
	}
	ga_pileup_free(p);
	ga_graph_destroy(g);
}

// graphs the fold must refuse, unfolded queries still answered; and the smallest one it takes
void checkPreconditions()
{
	struct Case { const char* what; std::vector<std::pair<int64_t, std::string>> nodes; int overlap; bool folds; };
	const std::vector<Case> cases = {
		{"overlap", {{2, "ACGTAC"}, {3, "GTACGT"}}, 2, false},
		{"twin of another length", {{2, "ACGTA"}, {3, "ACGT"}}, 0, false},
		{"twin that is not the reverse complement", {{2, "ACGT"}, {3, "AAAA"}}, 0, false},
		{"one strand", {{2, "ACGT"}, {4, "ACGT"}}, 0, false},
		{"mixed", {{2, "ACGT"}, {3, "ACGT"}, {4, "AC"}}, 0, false},
		{"a pair", {{2, "ACGGA"}, {3, "TCCGT"}}, 0, true},
	};
	for (const Case& c : cases)
	{
		ga_graph_t* g = ga_graph_create();
		for (auto& n : c.nodes) CHECK(ga_graph_add_node(g, n.first, n.second.data(), n.second.size(), (int)(n.first & 1)) == GA_S_OK, "node");
		CHECK(ga_graph_finalize(g, c.overlap) == GA_S_OK && ga_graph_upload(g, 0) == GA_S_OK, "finalize and upload");
		const uint64_t columns = (uint64_t)ga_graph_bp(g);
		ga_pileup_t* p = nullptr;
		CHECK(ga_pileup_create(g, GA_PILEUP_DEPTH, &p) == GA_S_OK && p, "pileup");
		std::vector<uint32_t> ones(columns, 1);
		CHECK(ga_emul_sites_poke(p, ones.data(), ones.size()) == 0, "poke");
		ga_sites_t* out = nullptr;
		ga_site_params_t q = params(0, 1, 0, 0, 1, 0, columns, 0);
		CHECK(ga_pileup_sites(p, &q, &out) == GA_S_OK && out && out->n_total == columns, "%s: unfolded", c.what);
		ga_sites_free(out);
		q.flags = GA_SITES_FOLD;
		for (int twice = 0; twice < 2; twice++)
		{
			if (!c.folds) { CHECK(refused(p, q), "%s: fold accepted", c.what); continue; }
			out = nullptr;
			CHECK(ga_pileup_sites(p, &q, &out) == GA_S_OK && out && out->n_total == 5 && out->sites[0].counts[0] == 2 && out->sites[4].entry == 5, "%s: fold", c.what);
			ga_sites_free(out);
		}
		queries += 3;
		ga_pileup_free(p);
		ga_graph_destroy(g);
	}
}

}  // namespace

int main()
{
	ga_sites_free(nullptr);
	checkPreconditions();
	checkChain({5, 1, 70, 1, gast::kTile + 9}, 1);
	checkChain({1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 3}, 2);
	checkChain({64, 63, 65, 2 * gast::kTile}, 3);
	printf("%llu queries through ga_pileup_sites against the stub back end, %llu sites compared, %d failures\n", queries, sitesSeen, failures);
	return failures ? 1 : 0;
}
