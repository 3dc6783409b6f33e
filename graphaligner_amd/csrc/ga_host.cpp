// ga_host.cpp -- host side of the C ABI (include/graphaligner_amd.h): the graph model the
// reference's loaders build (AlignmentGraph.cpp, BigraphToDigraph.cpp), its upload, and the
// pileups that stay with a graph.  Reads become jobs in ga_prepare.h, the device's traces
// become AlignmentResults in ga_collect.h, both included at the end of this file: the host
// library stays the one translation unit that the test build of tests/emul compiles, in files
// by subject.  ga_host.h has what the three share.  No alignment arithmetic happens here; the
// extension program runs behind ga_backend.h on the GPU.
#include <cmath>
#include <sstream>

#include "ga_host.h"

using namespace gahost;

// threads this process can really run at once: the affinity mask, capped by a cgroup CPU quota.  More threads than that are worse than
// useless under a quota: a burst of 64 threads on 16 cores' worth of quota spends the period's budget in a quarter of the period and the
// whole process -- the thread that waits for the GPU included -- is throttled for the rest of it.
size_t gahost::usableCores()
{
	static const size_t cached = []() -> size_t {
		size_t n = std::thread::hardware_concurrency();
#ifdef __linux__
		cpu_set_t set;
		if (sched_getaffinity(0, sizeof(set), &set) == 0) { const int c = CPU_COUNT(&set); if (c > 0) n = std::min<size_t>(n ? n : (size_t)c, (size_t)c); }
		if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r"))
		{
			char quota[32]; long long period = 0;
			if (fscanf(f, "%31s %lld", quota, &period) == 2 && strcmp(quota, "max") != 0 && period > 0)
				n = std::min<size_t>(n, (size_t)std::max<long long>(1, (atoll(quota) + period / 2) / period));
			fclose(f);
		}
		else if (FILE* q = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r"))
		{
			long long quota = -1, period = 0;
			if (fscanf(q, "%lld", &quota) != 1) quota = -1;
			fclose(q);
			if (FILE* pf = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) { if (fscanf(pf, "%lld", &period) != 1) period = 0; fclose(pf); }
			if (quota > 0 && period > 0) n = std::min<size_t>(n, (size_t)std::max<long long>(1, (quota + period / 2) / period));
		}
#endif
		return std::max<size_t>(1, n);
	}();
	return cached;
}

namespace {

GaHmmTables buildHmm()
{
	// AlignmentCorrectnessEstimation.cpp:6-36, 61-69, 81-83 -- same libm calls, same order
	GaHmmTables t;
	const double cMis = log(0.2), cMat = log(1.0 - 0.2), fMis = log(0.5), fMat = log(1.0 - 0.5);
	t.f2c = log(0.00001); t.f2f = log(1.0 - 0.00001);
	t.c2f = log(0.000000000000001); t.c2c = log(1.0 - 0.000000000000001);
	double lf[65];
	lf[0] = 0;
	for (int i = 1; i <= 64; i++) lf[i] = lf[i - 1] + log(i);
	for (int m = 0; m <= 64; m++)
	{
		double choose = lf[64] - lf[m] - lf[64 - m];
		t.correct_mult[m] = choose + m * cMis + (64 - m) * cMat;
		t.wrong_mult[m] = choose + m * fMis + (64 - m) * fMat;
	}
	t.init_correct = log(0.8);
	t.init_wrong = log(0.2);
	return t;
}

}  // namespace

// ================================================================================================
// graph
// ================================================================================================
// what ga_seed_host.cpp sees of a graph and of a seeded batch (ga_backend.h)
GaGraphView ga_graph_view(const ga_graph* g) { return GaGraphView{g->finalized, &g->ids, &g->flat, g->device}; }
GaBatchSeedView ga_batch_seed_view(const ga_batch* b)
{
	GaBatchSeedView v;
	if (!b || !b->seeded) return v;
	v.seeded = true; v.byLocus = b->byLocus; v.g = b->g; v.nReads = b->reads.size(); v.maxSeeds = b->seedParams.max_seeds;
	v.outN = b->seedOutN.data(); v.outSeed = b->seedOut.data(); v.outLocus = b->seedOutLocus.data(); v.outNLoci = b->seedNLoci.data();
	v.kernel_ms = b->seedMs;
	return v;
}

static int addNode(ga_graph* g, int64_t id, const char* seq, size_t len, bool rev)
{
	if (g->finalized) return GA_E_INVALID;
	if (g->lookup.count(id)) return GA_S_OK;            // duplicates ignored (AlignmentGraph.cpp:51)
	for (size_t i = 0; i < len; i++) if (tables().baseCode[(uint8_t)seq[i]] > 3) return GA_E_INVALID;   // graph is ACGT only (:83-85)
	if (g->nodeStart.size() >= 0x7ffffff0u) return GA_E_INVALID;
	g->lookup[id] = (uint32_t)g->nodeStart.size();
	g->ids.push_back(id);
	g->nodeStart.push_back(g->bases.size());
	g->reverse.push_back(rev ? 1 : 0);
	for (size_t i = 0; i < len; i++) g->bases.push_back(tables().baseCode[(uint8_t)seq[i]]);
	return GA_S_OK;
}

static int addEdge(ga_graph* g, int64_t from, int64_t to)
{
	if (g->finalized) return GA_E_INVALID;
	auto f = g->lookup.find(from), t = g->lookup.find(to);
	if (f == g->lookup.end() || t == g->lookup.end()) return GA_E_INVALID;
	g->edgeList.emplace_back(f->second, t->second);                                               // double edges are dropped at Finalize (:104-105)
	return GA_S_OK;
}

// a node's inNeighbors / outNeighbors exactly as a finished AlignmentGraph holds them (AlignmentGraph.h:49-50)
static int setNeighbors(ga_graph* g, int64_t id, const int64_t* in, size_t nIn, const int64_t* out, size_t nOut)
{
	if (g->finalized) return GA_E_INVALID;
	auto me = g->lookup.find(id);
	if (me == g->lookup.end()) return GA_E_INVALID;
	std::pair<std::vector<uint32_t>, std::vector<uint32_t>> lists;
	for (size_t k = 0; k < nIn; k++) { auto it = g->lookup.find(in[k]); if (it == g->lookup.end()) return GA_E_INVALID; lists.first.push_back(it->second); }
	for (size_t k = 0; k < nOut; k++) { auto it = g->lookup.find(out[k]); if (it == g->lookup.end()) return GA_E_INVALID; lists.second.push_back(it->second); }
	g->givenLists[me->second] = std::move(lists);
	return GA_S_OK;
}

static std::string revcompACGT(const char* seq, size_t len)
{
	std::string r(len, 'N');
	for (size_t i = 0; i < len; i++) r[i] = (char)tables().complement[(uint8_t)seq[len - 1 - i]];
	return r;
}

static int finalizeGraph(ga_graph* g, int overlap)
{
	if (g->finalized) return GA_E_INVALID;
	g->dbgOverlap = overlap;
	// dummy end node (AlignmentGraph.cpp:110-118)
	g->ids.push_back(0); g->nodeStart.push_back(g->bases.size()); g->reverse.push_back(0); g->bases.push_back(4);
	g->finalized = true;
	const uint32_t n = g->nodeCount();
	g->twin.assign(n, 0xffffffffu);
	g->idOdd.assign(n, 0);
	for (uint32_t i = 1; i + 1 < n; i++)
	{
		auto it = g->lookup.find(g->ids[i] ^ 1);
		if (it != g->lookup.end()) g->twin[i] = it->second;
		g->idOdd[i] = (uint8_t)(g->ids[i] & 1);
	}
	GaFlatGraph& f = g->flat;
	f.node_start.assign(g->nodeStart.begin(), g->nodeStart.end());
	f.node_start.push_back(g->bases.size());
	f.seq2.assign((g->bases.size() + 15) / 16 + 8, 0);      // (+ slack: the kernels request base words a little past a node's end)
	for (size_t i = 0; i < g->bases.size(); i++) f.seq2[i >> 4] |= (uint32_t)(g->bases[i] & 3) << ((i & 15) * 2);
	// neighbour lists: every node's in- and out-list in the order its edges were added, a repeated edge kept once (the reference
	// checks std::find before every push_back, AlignmentGraph.cpp:104-105).  Counting sort by node, then per-node de-duplication.
	{
		const auto& E = g->edgeList;
		std::vector<uint32_t> inCount(n + 1, 0), outCount(n + 1, 0);
		for (const auto& e : E) { outCount[e.first + 1]++; inCount[e.second + 1]++; }
		for (uint32_t i = 0; i < n; i++) { inCount[i + 1] += inCount[i]; outCount[i + 1] += outCount[i]; }
		std::vector<uint32_t> inAll(E.size() + 1), outAll(E.size() + 1);
		{
			std::vector<uint32_t> inAt(inCount.begin(), inCount.end() - 1), outAt(outCount.begin(), outCount.end() - 1);
			for (const auto& e : E) { outAll[outAt[e.first]++] = e.second; inAll[inAt[e.second]++] = e.first; }
		}
		auto compact = [&](const std::vector<uint32_t>& count, const std::vector<uint32_t>& all, std::vector<uint32_t>& off, std::vector<uint32_t>& nbr, bool inLists) {
			off.assign(n + 1, 0);
			nbr.clear();
			nbr.reserve(all.size() + 1);
			for (uint32_t i = 0; i < n; i++)
			{
				const size_t first = nbr.size();
				if (!g->givenLists.empty())
				{
					auto given = g->givenLists.find(i);
					if (given != g->givenLists.end())
					{
						// a finished list, taken as it is
						const std::vector<uint32_t>& lst = inLists ? given->second.first : given->second.second;
						nbr.insert(nbr.end(), lst.begin(), lst.end());
						off[i + 1] = (uint32_t)nbr.size();
						continue;
					}
				}
				for (uint32_t k = count[i]; k < count[i + 1]; k++)
				{
					bool seen = false;
					for (size_t q = first; q < nbr.size(); q++) if (nbr[q] == all[k]) { seen = true; break; }
					if (!seen) nbr.push_back(all[k]);
				}
				off[i + 1] = (uint32_t)nbr.size();
			}
			nbr.push_back(0);
		};
		compact(inCount, inAll, f.in_off, f.in_nbr, true);
		compact(outCount, outAll, f.out_off, f.out_nbr, false);
		std::vector<std::pair<uint32_t, uint32_t>>().swap(g->edgeList);
		g->givenLists.clear();
	}
	g->hmm = buildHmm();
	return GA_S_OK;
}

// ================================================================================================
// C ABI
// ================================================================================================
extern "C" {

ga_graph_t* ga_graph_create(void) { return new ga_graph(); }
void ga_graph_destroy(ga_graph_t* g) { if (g) { delete g->device; delete g; } }
int ga_graph_add_node(ga_graph_t* g, int64_t id, const char* seq, size_t len, int rev) { return g ? addNode(g, id, seq, len, rev != 0) : GA_E_INVALID; }
int ga_graph_add_edge(ga_graph_t* g, int64_t from, int64_t to) { return g ? addEdge(g, from, to) : GA_E_INVALID; }
int ga_graph_set_neighbors(ga_graph_t* g, int64_t id, const int64_t* in, size_t nIn, const int64_t* out, size_t nOut)
{
	return g && (in || nIn == 0) && (out || nOut == 0) ? setNeighbors(g, id, in, nIn, out, nOut) : GA_E_INVALID;
}
int ga_graph_add_bigraph_node(ga_graph_t* g, int64_t id, const char* seq, size_t len)
{
	if (!g) return GA_E_INVALID;
	int s = addNode(g, id * 2, seq, len, false);
	if (s) return s;
	std::string rc = revcompACGT(seq, len);
	return addNode(g, id * 2 + 1, rc.data(), rc.size(), true);
}
int ga_graph_add_bigraph_edge(ga_graph_t* g, int64_t from, int fromStart, int64_t to, int toEnd)
{
	if (!g) return GA_E_INVALID;
	// BigraphToDigraph.cpp:32-56 / 70-104
	int64_t fromLeft = fromStart ? from * 2 : from * 2 + 1, fromRight = fromStart ? from * 2 + 1 : from * 2;
	int64_t toLeft = toEnd ? to * 2 : to * 2 + 1, toRight = toEnd ? to * 2 + 1 : to * 2;
	int s = addEdge(g, fromRight, toRight);
	if (s) return s;
	return addEdge(g, toLeft, fromLeft);
}
int ga_graph_finalize(ga_graph_t* g, int overlap) { return g ? finalizeGraph(g, overlap) : GA_E_INVALID; }

static int loadGfa(ga_graph_t* g, const char* text, size_t len, uint32_t maxNodeLen)
{
	// DirectedGraph::StreamGFAGraphFromFile (BigraphToDigraph.cpp:137-189): three passes over the lines
	if (!g || g->finalized) return GA_E_INVALID;
	std::vector<std::pair<const char*, size_t>> lines;
	for (size_t i = 0; i < len;)
	{
		size_t e = i;
		while (e < len && text[e] != '\n') e++;
		if (e > i) lines.emplace_back(text + i, e - i);
		i = e + 1;
	}
	int overlap = 0;
	int64_t maxId = 0;
	for (auto& l : lines)
	{
		if (l.first[0] == 'S' && maxNodeLen) { std::stringstream str(std::string(l.first, std::min<size_t>(l.second, 64))); std::string d; int64_t id = 0; str >> d >> id; maxId = std::max(maxId, id); }
		if (l.first[0] != 'L') continue;
		std::stringstream str(std::string(l.first, l.second));
		std::string d1, d2, d3, d4, d5, ov;
		str >> d1 >> d2 >> d3 >> d4 >> d5 >> ov;
		if (ov.size() < 2) return GA_E_INVALID;
		int o = std::stoi(ov.substr(0, ov.size() - 1));
		if (!(overlap == 0 || overlap == o)) return GA_E_INVALID;
		overlap = o;
	}
	if (maxNodeLen && overlap != 0) return GA_E_INVALID;       // pieces of a node overlap by nothing: splitting is for blunt graphs
	// first / last piece of every split node: the end an edge attaches to
	std::unordered_map<int64_t, std::pair<int64_t, int64_t>> ends;
	int64_t nextId = maxId + 1;
	for (auto& l : lines)
	{
		if (l.first[0] != 'S') continue;
		std::stringstream str(std::string(l.first, l.second));
		std::string d, seq;
		int64_t id;
		str >> d >> id >> seq;
		if ((int)seq.size() <= overlap) return GA_E_INVALID;
		if (maxNodeLen && seq.size() > maxNodeLen)
		{
			// a chain of pieces, the first keeping the node's id; the reverse strand's nodes follow from the pieces like any node's
			int64_t prev = -1;
			for (size_t at = 0; at < seq.size(); at += maxNodeLen)
			{
				const size_t n = std::min<size_t>(maxNodeLen, seq.size() - at);
				const int64_t pid = at == 0 ? id : nextId++;
				int st = ga_graph_add_bigraph_node(g, pid, seq.data() + at, n);
				if (st) return st;
				g->pieces[pid] = ga_graph::Piece{id, at, n, seq.size()};
				if (prev >= 0) { st = ga_graph_add_bigraph_edge(g, prev, 0, pid, 0); if (st) return st; }
				prev = pid;
			}
			ends[id] = std::make_pair(id, prev);
			continue;
		}
		size_t keep = seq.size() - overlap;
		int s = addNode(g, id * 2, seq.data(), keep, false);
		if (s) return s;
		std::string rc = revcompACGT(seq.data(), seq.size());
		s = addNode(g, id * 2 + 1, rc.data(), keep, true);
		if (s) return s;
	}
	for (auto& l : lines)
	{
		if (l.first[0] != 'L') continue;
		std::stringstream str(std::string(l.first, l.second));
		std::string d, fs, te;
		int64_t from, to;
		str >> d >> from >> fs >> to >> te;
		if ((fs != "+" && fs != "-") || (te != "+" && te != "-")) return GA_E_INVALID;
		// an edge leaves `from` at its end ("+") or its start ("-") and enters `to` at its start ("+") or its end ("-")
		auto ef = ends.find(from), et = ends.find(to);
		if (ef != ends.end()) from = fs == "-" ? ef->second.first : ef->second.second;
		if (et != ends.end()) to = te == "-" ? et->second.second : et->second.first;
		int s = ga_graph_add_bigraph_edge(g, from, fs == "-", to, te == "-");
		if (s) return s;
	}
	return finalizeGraph(g, overlap);
}

int ga_graph_load_gfa(ga_graph_t* g, const char* text, size_t len) { return loadGfa(g, text, len, 0); }
int ga_graph_load_gfa_split(ga_graph_t* g, const char* text, size_t len, uint32_t max_node_len) { return max_node_len ? loadGfa(g, text, len, max_node_len) : GA_E_INVALID; }

int ga_graph_split_lookup(const ga_graph_t* g, int64_t bigraph_id, int64_t* orig_id, uint64_t* start, uint64_t* orig_len)
{
	if (!g) return GA_E_INVALID;
	auto it = g->pieces.find(bigraph_id);
	if (it == g->pieces.end()) { if (orig_id) *orig_id = bigraph_id; if (start) *start = 0; if (orig_len) *orig_len = 0; return 1; }
	if (orig_id) *orig_id = it->second.orig;
	if (start) *start = it->second.start;
	if (orig_len) *orig_len = it->second.origLen;
	return GA_S_OK;
}

int ga_graph_upload(ga_graph_t* g, int device)
{
	if (!g) return GA_E_INVALID;
	if (!g->finalized) return GA_E_NOT_FINALIZED;
	delete g->device;
	int status = GA_S_OK;
	g->device = ga_backend_upload_graph(g->flat, g->hmm, device, &status);
	return g->device ? GA_S_OK : (status ? status : GA_E_DEVICE);
}
int64_t ga_graph_node_count(const ga_graph_t* g) { return g ? g->nodeCount() : 0; }
int64_t ga_graph_bp(const ga_graph_t* g) { return g ? (int64_t)g->bases.size() : 0; }

// ---- pileups (include/graphaligner_amd.h: "pileups"; ga_pileup.h) ------------------------------------------------------------------

int ga_graph_node_columns(const ga_graph_t* g, int64_t digraphId, uint64_t* firstColumn, uint64_t* length)
{
	if (!g || !g->finalized) return GA_E_INVALID;
	auto it = g->lookup.find(digraphId);
	if (it == g->lookup.end()) return GA_E_INVALID;
	if (firstColumn) *firstColumn = g->nodeStart[it->second];
	if (length) *length = g->nodeLen(it->second);
	return GA_S_OK;
}

int ga_graph_edge_slot_count(const ga_graph_t* g, uint64_t* n)
{
	if (!g || !n || !g->finalized) return GA_E_INVALID;
	*n = ga_edge_slot_count(g->flat);
	return GA_S_OK;
}

int ga_graph_edge_slots(const ga_graph_t* g, uint64_t first, uint64_t n, int64_t* fromIds, int64_t* toIds)
{
	if (!g || !g->finalized || (n && (!fromIds || !toIds))) return GA_E_INVALID;
	const uint64_t slots = ga_edge_slot_count(g->flat);
	if (first > slots || n > slots - first) return GA_E_INVALID;
	// the node whose in-list holds slot `first`, then onward: slots are the in-lists laid end to end in node-index order
	const std::vector<uint32_t>& off = g->flat.in_off;
	uint32_t to = (uint32_t)(std::upper_bound(off.begin(), off.end(), (uint32_t)first) - off.begin());
	to = to ? to - 1 : 0;
	for (uint64_t k = 0; k < n; k++)
	{
		const uint32_t slot = (uint32_t)(first + k);
		while (to + 1 < off.size() && off[to + 1] <= slot) to++;
		fromIds[k] = g->ids[g->flat.in_nbr[slot]];
		toIds[k] = g->ids[to];
	}
	return GA_S_OK;
}

int ga_pileup_create(const ga_graph_t* g, int kind, ga_pileup_t** out)
{
	if (!g || !out || !g->finalized || !g->device || (kind != GA_PILEUP_DEPTH && kind != GA_PILEUP_BASES && kind != GA_PILEUP_EDGES)) return GA_E_INVALID;
	GaPileupSpec spec;
	spec.kind = kind; spec.planes = ga_pileup_planes_of_kind(kind);
	spec.entries = ga_pileup_entries(kind, g->bases.size(), ga_edge_slot_count(g->flat));
	std::vector<uint32_t> mirror;
	if (kind == GA_PILEUP_EDGES) { mirror = ga_edge_mirror_slots(g->flat, g->twin); mirror.resize(mirror.size() + 1, 0xffffffffu); spec.mirrorSlot = mirror.data(); }
	int status = GA_S_OK;
	GaBackendPileup* dev = g->device->createPileup(spec, &status);
	if (!dev) return status ? status : GA_E_DEVICE;
	ga_pileup* p = new ga_pileup();
	p->g = g; p->kind = kind; p->planes = spec.planes; p->dev = dev;
	p->st.kind = kind; p->st.columns = spec.entries;
	*out = p;
	return GA_S_OK;
}

void ga_pileup_free(ga_pileup_t* p) { delete p; }

int ga_pileup_reset(ga_pileup_t* p)
{
	if (!p) return GA_E_INVALID;
	std::unique_lock<std::shared_mutex> alone(p->use);     // (waits for the adds in flight; none starts before the zeroing is done)
	std::lock_guard<std::mutex> guard(p->lock);
	if (int s = p->dev->reset()) return s;
	const int32_t kind = p->st.kind; const uint64_t columns = p->st.columns;
	memset(&p->st, 0, sizeof(p->st));
	p->st.kind = kind; p->st.columns = columns;
	return GA_S_OK;
}

int ga_batch_pileup_add(ga_batch_t* b, ga_pileup_t* p)
{
	if (!b || !p || !b->dev || !(b->flags & GA_F_PILEUP) || !b->collected || b->g != p->g) return GA_E_INVALID;
	GaPileupAdd add;
	add.list = b->pileList.data(); add.nList = b->pileList.size();
	add.pairs = b->pilePairs.data(); add.nPairs = b->pilePairs.size();
	add.slots = b->pileSlots.data(); add.nSlots = b->pileSlots.size();
	GaPileupAddOut o;
	{
		std::shared_lock<std::shared_mutex> shared(p->use);
		if (int s = b->dev->addToPileup(p->dev, add, o)) return s;
	}
	std::lock_guard<std::mutex> guard(p->lock);
	p->st.add_kernel_ms = o.kernel_ms;
	p->st.batches_added++;
	p->st.reads_from_device += b->pileFromDevice; p->st.reads_from_host += b->pileFromHost;
	p->st.jobs_walked += o.jobs; p->st.moves_read += o.moves; p->st.items_added += o.items;
	return GA_S_OK;
}

int ga_pileup_download(const ga_pileup_t* p, uint64_t firstColumn, uint64_t nColumns, uint32_t* out)
{
	if (!p || (!out && nColumns)) return GA_E_INVALID;
	const uint64_t entries = p->st.columns;              // (the entry count: columns, or slots for the EDGES kind)
	if (firstColumn > entries || nColumns > entries - firstColumn) return GA_E_INVALID;
	std::unique_lock<std::shared_mutex> alone(const_cast<ga_pileup*>(p)->use);      // (a whole add is in the copy or none of it)
	return p->dev->download(firstColumn, nColumns, out);
}

int ga_pileup_stats(const ga_pileup_t* p, ga_pileup_stats_t* out)
{
	if (!p || !out) return GA_E_INVALID;
	std::lock_guard<std::mutex> guard(const_cast<ga_pileup*>(p)->lock);
	*out = p->st;
	return GA_S_OK;
}

// ---- pileup sites (include/graphaligner_amd.h: "pileup sites"; ga_sites.h) ---------------------------------------------------------

// the fold table of a columns query (ga_backend.h: GA_FOLD_*) and the fold's preconditions: overlap 0, and every node but the dummy
// ones has a twin that is another node, of its length, with its reverse complement as bases.  Looked at once per graph
static bool foldTableOf(const ga_graph* g, const uint32_t** table)
{
	std::lock_guard<std::mutex> guard(g->foldLock);
	if (g->foldState == 0)
	{
		const uint32_t n = g->nodeCount();
		bool ok = g->dbgOverlap == 0 && g->twin.size() == n && g->idOdd.size() == n;
		std::vector<uint32_t> t(n, GA_FOLD_NONE);
		for (uint32_t i = 1; ok && i + 1 < n; i++)
		{
			const uint32_t o = g->twin[i];
			if (o == 0 || o >= n - 1 || o == i || g->twin[o] != i || g->nodeLen(o) != g->nodeLen(i)) { ok = false; break; }
			const uint32_t len = g->nodeLen(i);
			const uint64_t a = g->nodeStart[i], b = g->nodeStart[o];
			for (uint32_t k = 0; ok && k < len; k++) ok = g->bases[a + k] <= 3 && g->bases[b + (len - 1 - k)] == 3 - g->bases[a + k];
			t[i] = o | (g->idOdd[i] ? 0u : GA_FOLD_FORWARD);
		}
		g->foldTable.swap(t);
		g->foldState = ok ? 1 : -1;
	}
	*table = g->foldTable.data();
	return g->foldState == 1;
}

int ga_pileup_sites(ga_pileup_t* p, const ga_site_params_t* q, ga_sites_t** out)
{
	if (!p || !q || !out) return GA_E_INVALID;
	*out = nullptr;
	const uint64_t entries = p->st.columns;
	if ((q->flags & ~GA_SITES_FOLD) || q->min_depth < 1 || q->alt_den < 1 || q->alt_den > 65535 || q->alt_num > q->alt_den) return GA_E_INVALID;
	if (q->first_entry > entries || q->n_entries > entries - q->first_entry) return GA_E_INVALID;
	const ga_graph* g = p->g;
	const bool edges = p->kind == GA_PILEUP_EDGES;
	GaSiteQuery dq;
	dq.fold = (q->flags & GA_SITES_FOLD) != 0;
	dq.min_depth = q->min_depth; dq.min_alt = q->min_alt; dq.alt_num = q->alt_num; dq.alt_den = q->alt_den;
	dq.first = q->first_entry; dq.n = q->n_entries; dq.max_sites = q->max_sites;
	if (dq.fold && !edges)
	{
		if (!foldTableOf(g, &dq.foldTable)) return GA_E_INVALID;
		dq.nNodes = g->nodeCount();
	}
	GaSitesOut got;
	{
		std::unique_lock<std::shared_mutex> alone(p->use);   // (a whole add is in what the query reads or none of it)
		if (int s = p->dev->sites(dq, got)) return s;
	}
	const uint64_t cap = dq.max_sites ? std::min<uint64_t>(dq.max_sites, got.n_total) : got.n_total;
	if (got.recs.size() != cap) return GA_E_DEVICE;
	std::unique_ptr<ga_sites_t> res(new ga_sites_t());
	res->n_sites = got.recs.size(); res->n_total = got.n_total; res->entries_scanned = dq.n; res->kernel_ms = got.kernel_ms;
	res->sites = res->n_sites ? new ga_site_t[(size_t)res->n_sites]() : nullptr;
	// the records' places in the graph: entries ascend, so the node (or the in-list) of each is found from the one before onward
	const std::vector<uint32_t>& inOff = g->flat.in_off;
	for (size_t k = 0; k < got.recs.size(); k++)
	{
		const GaSiteRec& r = got.recs[k];
		ga_site_t& s = res->sites[k];
		s.entry = r.entry;
		memcpy(s.counts, r.counts, sizeof(s.counts));
		if (r.entry >= entries || (k && r.entry <= got.recs[k - 1].entry)) { ga_sites_free(res.release()); return GA_E_DEVICE; }
		if (edges)
		{
			const uint32_t to = (uint32_t)(std::upper_bound(inOff.begin(), inOff.end(), (uint32_t)r.entry) - inOff.begin()) - 1;
			s.from_id = g->ids[g->flat.in_nbr[(size_t)r.entry]];
			s.to_id = g->ids[to];
			s.graph_char = '-';
		}
		else
		{
			const uint32_t node = (uint32_t)(std::upper_bound(g->nodeStart.begin(), g->nodeStart.end(), r.entry) - g->nodeStart.begin()) - 1;
			s.node_id = g->ids[node] / 2;
			s.offset = (uint32_t)(r.entry - g->nodeStart[node]);
			s.reverse = (uint8_t)(g->ids[node] & 1);
			s.graph_char = g->baseChar(node, s.offset);
		}
	}
	*out = res.release();
	return GA_S_OK;
}

void ga_sites_free(ga_sites_t* s)
{
	if (!s) return;
	delete[] s->sites;
	delete s;
}

const char* ga_status_string(int s)
{
	switch (s)
	{
		case GA_S_OK: return "ok";
		case GA_S_ASSERTION: return "reference assertion";
		case GA_S_UNSUPPORTED_BAND: return "band >= 200000 bp and no device memory for the pass that carries the sparse method";
		case GA_S_BAD_SEED: return "seed node not in graph";
		case GA_S_CAPACITY: return "device buffer capacity";
		case GA_S_UNSUPPORTED_CYCLE: return "cyclic band left unresolved by the kernel ladder";
		case GA_S_UNSUPPORTED_RAMP: return "ramp redo left unresolved by the kernel ladder";
		case GA_E_INVALID: return "invalid argument";
		case GA_E_NO_DEVICE: return "no gfx950 device / graph not uploaded";
		case GA_E_DEVICE: return "device error";
		case GA_E_NOT_FINALIZED: return "graph not finalized";
	}
	return "unknown";
}
const char* ga_version(void) { return "graphaligner_amd 0.1 (gfx950)"; }

}  // extern "C"

// ================================================================================================
// batches: preparation and result assembly
// ================================================================================================
#define GA_HOST_PARTS
#include "ga_prepare.h"
#include "ga_collect.h"
