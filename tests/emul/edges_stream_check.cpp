// edges_stream_check.cpp -- TEST-ONLY, stand-alone: a main of its own over the host code of edge support, so that it can be built with
// -fsanitize=address,undefined and run as it is (tests/emul/edges.mk, target `check`; nothing is loaded into another program).  It
// reads the file tests/edge_stream_dump.py writes -- the graphs and fabricated streams of tests/test_edge_pileup.py with what the
// models expect -- and puts them through
//   the host library's slot entry points (ga_graph_edge_slot_count, ga_graph_edge_slots: whole table, sub-ranges, refusals) and
//   ga_pileup_create without a device, linked from ga_host.cpp; then, uploaded to a stub back end that hands out pileups in host memory
//   and runs nothing, ga_pileup_create, ga_pileup_stats, ga_pileup_reset and ga_pileup_download of all three kinds (whole pileup,
//   sub-ranges into buffers of exactly their size, refusal of a range past the entries), also on graphs of one strand alone and of
//   mixed strands, where interior nodes have no twin and the mirror-slot table is built from them;
//   the mirror-slot table of ga_backend.h and the edge-support program of ga_edges.h compiled with GA_EMULATE, through the hooks of
//   ga_emul_edges.cpp, the counters followed by guard words.
// Exit status 0 and a line of totals when everything agrees.
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>

#include "ga_emul_edges.cpp"
#include "../../include/graphaligner_amd.h"

// the back end this program links: no device behind it.  It makes pileups in host memory (as the spec sizes them, keeping a copy of
// the mirror-slot table as a device would), answers reset and download, and creates no batch
namespace {
struct StubPileup : GaBackendPileup
{
	uint32_t nPlanes = 0;
	uint64_t entries = 0;
	std::vector<uint32_t> words, mirror;
	int reset() override { std::fill(words.begin(), words.end(), 0u); return 0; }
	int download(uint64_t first, uint64_t n, uint32_t* out) const override
	{
		if (first > entries || n > entries - first) return GA_E_INVALID;
		for (uint32_t k = 0; k < nPlanes; k++) std::copy(words.begin() + (size_t)(k * entries + first), words.begin() + (size_t)(k * entries + first + n), out + (size_t)k * n);
		return 0;
	}
};
struct StubGraph : GaBackendGraph
{
	uint64_t columns = 0, slots = 0;
	bool codesPileup() const override { return true; }
	GaBackendPileup* createPileup(const GaPileupSpec& spec, int* status) override
	{
		*status = GA_E_INVALID;
		if (!spec.planes || spec.planes != ga_pileup_planes_of_kind(spec.kind) || spec.entries != ga_pileup_entries(spec.kind, columns, slots)) return nullptr;
		if (spec.kind == GA_KIND_EDGES && !spec.mirrorSlot) return nullptr;
		StubPileup* p = new StubPileup();
		p->nPlanes = spec.planes; p->entries = spec.entries;
		p->words.assign((size_t)spec.planes * spec.entries, 0xA5A5A5A5u);
		if (spec.kind == GA_KIND_EDGES) p->mirror.assign(spec.mirrorSlot, spec.mirrorSlot + spec.entries);
		p->reset();
		for (size_t k = 0; k < p->words.size(); k++) p->words[k] = (uint32_t)k * 2654435761u;      // (something to tell places apart by)
		*status = 0;
		return p;
	}
};
}  // namespace
GaBackendGraph* ga_backend_upload_graph(const GaFlatGraph& flat, const GaHmmTables&, int device, int* status)
{
	if (device != 0) { *status = GA_E_NO_DEVICE; return nullptr; }
	StubGraph* g = new StubGraph();
	g->columns = flat.node_start.back(); g->slots = ga_edge_slot_count(flat);
	*status = 0;
	return g;
}
GaBackendBatch* ga_backend_create_batch(GaBackendGraph*, GaRowsProvider, const uint64_t*, const GaEqSource*, size_t, const std::vector<GaJob>&, const GaRunConfig&, int* status)
{
	*status = GA_E_NO_DEVICE;
	return nullptr;
}

namespace {

int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; fprintf(stderr, "line %d: ", __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

constexpr uint32_t kGuard = 0xDEADBEEFu;
constexpr size_t kGuards = 64;

struct Fabricated { std::vector<uint32_t> len, off, nbr, twin, mirror; };

std::vector<uint32_t> numbers(std::ifstream& in)
{
	std::string line;
	std::getline(in, line);
	std::istringstream s(line);
	std::vector<uint32_t> v;
	for (uint64_t x; s >> x;) v.push_back((uint32_t)x);
	return v;
}

// the graph uploaded to the stub back end: pileups of the three kinds, their sizes, downloads and refusals
void checkPileups(ga_graph_t* g, uint64_t nSlots)
{
	CHECK(ga_graph_upload(g, 1) == GA_E_NO_DEVICE, "upload to a device that is not there");
	CHECK(ga_graph_upload(g, 0) == GA_S_OK, "upload");
	const uint64_t columns = (uint64_t)ga_graph_bp(g);
	ga_pileup_t* none = nullptr;
	CHECK(ga_pileup_create(g, 3, &none) == GA_E_INVALID && !none, "a kind that is none");
	for (int kind : {GA_PILEUP_DEPTH, GA_PILEUP_BASES, GA_PILEUP_EDGES})
	{
		const uint64_t planes = kind == GA_PILEUP_BASES ? 8 : 1, entries = kind == GA_PILEUP_EDGES ? nSlots : columns;
		ga_pileup_t* p = nullptr;
		CHECK(ga_pileup_create(g, kind, &p) == GA_S_OK && p, "pileup of kind %d", kind);
		if (!p) continue;
		ga_pileup_stats_t st;
		CHECK(ga_pileup_stats(p, &st) == GA_S_OK && st.kind == kind && st.columns == entries && st.items_added == 0, "statistics of kind %d", kind);
		std::vector<uint32_t> whole(planes * entries + 2, kGuard);
		CHECK(ga_pileup_download(p, 0, entries, whole.data()) == GA_S_OK && whole[planes * entries] == kGuard && whole[planes * entries + 1] == kGuard, "whole download");
		for (uint64_t first : {(uint64_t)0, (uint64_t)1, entries / 2, entries - 1, entries})
			for (uint64_t len : {(uint64_t)0, (uint64_t)1, (uint64_t)5, entries - first, entries - first + 1, entries + 1})
			{
				if (first > entries) continue;
				std::vector<uint32_t> part(planes * std::min<uint64_t>(len, entries) + 2, kGuard);
				const int rc = ga_pileup_download(p, first, len, part.data());
				if (len > entries - first)
				{
					CHECK(rc == GA_E_INVALID, "kind %d: range %llu + %llu of %llu accepted", kind, (unsigned long long)first, (unsigned long long)len, (unsigned long long)entries);
					CHECK(part[0] == kGuard, "a refused download wrote");
					continue;
				}
				CHECK(rc == GA_S_OK, "kind %d: range refused", kind);
				for (uint64_t k = 0; k < planes; k++) for (uint64_t i = 0; i < len; i++) CHECK(part[k * len + i] == whole[k * entries + first + i], "kind %d: entry", kind);
				CHECK(part[planes * len] == kGuard && part[planes * len + 1] == kGuard, "words behind a download written");
			}
		CHECK(ga_pileup_download(p, entries + 1, 0, whole.data()) == GA_E_INVALID, "range past the entries");
		CHECK(ga_pileup_reset(p) == GA_S_OK && ga_pileup_download(p, 0, entries, whole.data()) == GA_S_OK, "reset");
		for (uint64_t k = 0; k < planes * entries; k++) CHECK(whole[k] == 0, "reset left a count");
		CHECK(ga_pileup_stats(p, &st) == GA_S_OK && st.kind == kind && st.columns == entries, "statistics after reset");
		ga_pileup_free(p);
	}
}

void checkSlots(std::ifstream& in, size_t nNodes, size_t nEdges, size_t nSlots)
{
	ga_graph_t* g = ga_graph_create();
	std::string tag, seq;
	for (size_t k = 0; k < nNodes; k++) { long long id; in >> tag >> id >> seq; CHECK(ga_graph_add_bigraph_node(g, id, seq.data(), seq.size()) == GA_S_OK, "node %lld", id); }
	for (size_t k = 0; k < nEdges; k++) { long long a, c; int b, d; in >> tag >> a >> b >> c >> d; CHECK(ga_graph_add_bigraph_edge(g, a, b, c, d) == GA_S_OK, "edge"); }
	std::vector<int64_t> wantFrom(nSlots), wantTo(nSlots);
	for (size_t k = 0; k < nSlots; k++) { long long a, b; in >> tag >> a >> b; wantFrom[k] = a; wantTo[k] = b; }
	std::getline(in, tag);
	uint64_t n = 0;
	CHECK(ga_graph_edge_slot_count(g, &n) == GA_E_INVALID, "slot count before finalize");
	CHECK(ga_graph_finalize(g, 0) == GA_S_OK, "finalize");
	CHECK(ga_graph_edge_slot_count(g, &n) == GA_S_OK && n == nSlots, "slot count %llu, expected %zu", (unsigned long long)n, nSlots);
	// the whole table and the ranges of 0, 1, 3 and all remaining slots from the first and the last five places, each into a buffer of exactly its size with guard words behind it
	for (uint64_t first = 0; first <= n; first++)
		for (uint64_t len : {(uint64_t)0, (uint64_t)1, (uint64_t)3, n - first})
		{
			if (first > 4 && first + 4 < n) continue;
			std::vector<int64_t> from(len + 2, -7), to(len + 2, -7);
			const int rc = ga_graph_edge_slots(g, first, len, from.data(), to.data());
			if (len > n - first) { CHECK(rc == GA_E_INVALID, "range %llu + %llu of %llu accepted", (unsigned long long)first, (unsigned long long)len, (unsigned long long)n); continue; }
			CHECK(rc == GA_S_OK, "range refused");
			for (uint64_t k = 0; k < len; k++) CHECK(from[k] == wantFrom[first + k] && to[k] == wantTo[first + k], "slot %llu", (unsigned long long)(first + k));
			CHECK(from[len] == -7 && from[len + 1] == -7 && to[len] == -7 && to[len + 1] == -7, "words behind the slots written");
		}
	CHECK(ga_graph_edge_slots(g, n + 1, 0, nullptr, nullptr) == GA_E_INVALID, "range past the slots");
	ga_pileup_t* p = nullptr;
	for (int kind : {GA_PILEUP_DEPTH, GA_PILEUP_BASES, GA_PILEUP_EDGES, 3}) CHECK(ga_pileup_create(g, kind, &p) == GA_E_INVALID && !p, "pileup without a device");
	checkPileups(g, n);
	ga_graph_destroy(g);
}

// graphs through the digraph-level calls where interior nodes have no twin: one strand alone, and mixed
void checkTwinless()
{
	for (int mixed = 0; mixed < 2; mixed++)
	{
		ga_graph_t* g = ga_graph_create();
		const char* seq = "ACGTACGTACGTACG";
		const int nNodes = 40;
		for (int k = 1; k <= nNodes; k++)
		{
			CHECK(ga_graph_add_node(g, 2 * k, seq, (size_t)(1 + k % 7), 0) == GA_S_OK, "node");
			if (mixed && k % 3 == 0) CHECK(ga_graph_add_node(g, 2 * k + 1, seq, (size_t)(1 + k % 7), 1) == GA_S_OK, "node");
		}
		for (int k = 1; k < nNodes; k++)
		{
			CHECK(ga_graph_add_edge(g, 2 * k, 2 * k + 2) == GA_S_OK, "edge");
			if (k + 2 <= nNodes) CHECK(ga_graph_add_edge(g, 2 * k, 2 * k + 4) == GA_S_OK, "edge");
			if (mixed && k % 3 == 0 && k + 3 <= nNodes) CHECK(ga_graph_add_edge(g, 2 * k + 7, 2 * k + 1) == GA_S_OK, "edge");
		}
		CHECK(ga_graph_finalize(g, 0) == GA_S_OK, "finalize");
		uint64_t n = 0;
		CHECK(ga_graph_edge_slot_count(g, &n) == GA_S_OK && n >= 2u * nNodes - 3, "slots of a twinless graph");
		checkPileups(g, n);
		ga_graph_destroy(g);
	}
}

}  // namespace

int main(int argc, char** argv)
{
	if (argc != 2) { fprintf(stderr, "usage: %s FILE (written by tests/edge_stream_dump.py)\n", argv[0]); return 2; }
	std::ifstream in(argv[1]);
	if (!in) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
	std::vector<Fabricated> fabricated;
	size_t graphs = 0, streams = 0;
	unsigned long long crossings = 0;
	std::string tag;
	checkTwinless();
	while (in >> tag)
	{
		if (tag == "G")
		{
			size_t nNodes, nEdges, nSlots;
			in >> nNodes >> nEdges >> nSlots;
			checkSlots(in, nNodes, nEdges, nSlots);
			graphs++;
		}
		else if (tag == "X")
		{
			size_t n;
			in >> n;
			std::getline(in, tag);
			Fabricated f;
			f.len = numbers(in); f.off = numbers(in); f.nbr = numbers(in); f.twin = numbers(in); f.mirror = numbers(in);
			CHECK(f.len.size() == n && f.off.size() == n + 1 && f.twin.size() == n && f.nbr.size() == f.off.back() && f.mirror.size() == f.off.back(), "fabricated graph");
			std::vector<uint32_t> got(f.mirror.size() + kGuards, kGuard);
			f.nbr.push_back(0);
			CHECK(ga_emul_edges_mirror((uint32_t)n, f.len.data(), f.off.data(), f.nbr.data(), f.twin.data(), got.data()) == (long)f.mirror.size(), "mirror table");
			CHECK(std::equal(f.mirror.begin(), f.mirror.end(), got.begin()), "mirror slots differ");
			for (size_t k = f.mirror.size(); k < got.size(); k++) CHECK(got[k] == kGuard, "words behind the mirror table written");
			fabricated.push_back(f);
		}
		else if (tag == "C")
		{
			size_t gi, nz;
			uint32_t startNode, startOffset, startRow, traceRows, nMoves;
			int backward;
			long items;
			std::string hex;
			in >> gi >> startNode >> startOffset >> startRow >> traceRows >> backward >> nMoves >> hex >> items >> nz;
			if (gi >= fabricated.size()) { CHECK(false, "stream of an unknown graph"); break; }
			const Fabricated& f = fabricated[gi];
			const size_t entries = f.off.back();
			std::vector<uint32_t> want(entries, 0);
			for (size_t k = 0; k < nz; k++) { size_t slot; uint32_t c; in >> slot >> c; if (slot < entries) want[slot] = c; else CHECK(false, "expected slot"); }
			// the moves in a buffer of exactly their size, the counters in one of exactly the entries + guard words
			std::vector<uint8_t> moves(nMoves);
			for (uint32_t k = 0; k < nMoves && 2 * k + 1 < hex.size(); k++) moves[k] = (uint8_t)std::stoul(hex.substr(2 * k, 2), nullptr, 16);
			std::vector<uint32_t> counts(entries + kGuards, kGuard);
			const long got = ga_emul_edges_stream(moves.data(), nMoves, (uint32_t)f.len.size(), f.len.data(), f.off.data(), f.nbr.data(), f.twin.data(), startNode,
			                                      startOffset, startRow, traceRows, backward, counts.data(), entries);
			CHECK(got == items, "stream %zu: %ld crossings, expected %ld", streams, got, items);
			CHECK(std::equal(want.begin(), want.end(), counts.begin()), "stream %zu: counts differ", streams);
			for (size_t k = entries; k < counts.size(); k++) CHECK(counts[k] == kGuard, "stream %zu: words behind the counters written", streams);
			streams++;
			crossings += (unsigned long long)(got > 0 ? got : 0);
		}
		else { CHECK(false, "unknown line %s", tag.c_str()); break; }
	}
	printf("%zu graphs through the slot and pileup entry points (and 2 without twins), %zu fabricated graphs, %zu streams, %llu crossings counted, %d failures\n", graphs, fabricated.size(), streams,
	       crossings, failures);
	return failures ? 1 : 0;
}
