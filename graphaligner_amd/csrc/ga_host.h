// ga_host.h -- what the host library's files share (ga_host.cpp: tables, graph model, loaders, pileups; ga_prepare.h: reads into
// jobs; ga_collect.h: the device's traces into results).  Internal: never installed, never read by the device build.
// (With this header ga_seed_host.cpp could see ga_graph and ga_batch itself; GaGraphView / GaBatchSeedView of ga_backend.h stay until
// a change that may touch a header the device build reads.)
#pragma once
#include <sched.h>
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <string_view>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/graphaligner_amd.h"
#include "ga_backend.h"

namespace gahost {

constexpr int W = 64;

// ---- character tables ------------------------------------------------------------------------
struct CharTables
{
	uint8_t rowCode[256];    // bits 0-3: which of A,C,G,T the read char matches; bits 4-6: exact code; bit 7: not IUPAC
	uint8_t rowCodeRc[256];  // rowCode of the complement
	uint8_t complement[256]; // 0 = the reference's ReverseComplement asserts on this char
	uint8_t baseCode[256];   // A0 C1 G2 T3, 255 otherwise
	CharTables()
	{
		for (int c = 0; c < 256; c++) { rowCode[c] = GA_ROW_INVALID; complement[c] = 0; baseCode[c] = 255; }
		auto setMatch = [&](char upper, int mask) {
			rowCode[(uint8_t)upper] = (uint8_t)(mask | (7 << 4));
			rowCode[(uint8_t)(upper + 32)] = (uint8_t)(mask | (7 << 4));
		};
		const int A = 1, C = 2, G = 4, T = 8;
		// characterMatch (GraphAligner.h:2039-2110)
		setMatch('A', A); setMatch('C', C); setMatch('G', G); setMatch('T', T); setMatch('N', A | C | G | T);
		setMatch('R', A | G); setMatch('Y', C | T); setMatch('K', G | T); setMatch('M', C | A); setMatch('S', C | G); setMatch('W', A | T);
		setMatch('B', C | G | T); setMatch('D', A | G | T); setMatch('H', A | C | T); setMatch('V', A | C | G);
		// the "previousEq" comparison is a raw char == against the upper-case graph base (:1503,1540)
		rowCode[(uint8_t)'A'] = (uint8_t)(A | (0 << 4)); rowCode[(uint8_t)'C'] = (uint8_t)(C | (1 << 4));
		rowCode[(uint8_t)'G'] = (uint8_t)(G | (2 << 4)); rowCode[(uint8_t)'T'] = (uint8_t)(T | (3 << 4));
		baseCode[(uint8_t)'A'] = 0; baseCode[(uint8_t)'C'] = 1; baseCode[(uint8_t)'G'] = 2; baseCode[(uint8_t)'T'] = 3;
		// ReverseComplement (CommonUtils.cpp:60-136): 'H'/'h' fall through to assert(false); 'U' -> 'A'
		const char* from = "ACTGNURYKMSWBVD";
		const char* to = "TGACNAYRMKSWVBH";
		for (int i = 0; from[i]; i++) { complement[(uint8_t)from[i]] = (uint8_t)to[i]; complement[(uint8_t)(from[i] + 32)] = (uint8_t)to[i]; }
		for (int c = 0; c < 256; c++) rowCodeRc[c] = rowCode[complement[c]];
	}
};
inline const CharTables& tables() { static const CharTables t; return t; }

// ---- jobs and results ------------------------------------------------------------------------
// a read as the batch keeps it: a view into the batch's one buffer of read copies
typedef std::string_view ReadSeq;

struct Pos { uint32_t node, offset; uint64_t row; };
typedef std::vector<Pos> Trace;

struct SeedPlan
{
	bool valid = false;          // lookups succeeded and the position is inside the read
	int early = GA_S_OK;         // status fixed before any device work (bad seed, assertion while splitting)
	uint32_t seedNodeIndex = 0;  // nodeLookup.at(id * 2), what the "already aligned" test compares (GraphAligner.h:423-425)
	int64_t fwJob = -1, bwJob = -1;
	uint64_t pos = 0;
};

struct ReadPlan { size_t firstSeed = 0, nSeeds = 0; };

// (a mapping's edit sequence is a piece of the read: kept as a span of it, copied once into the results)
struct SeqSpan { uint64_t pos, len; };
struct Partial { bool failed = true; int32_t score = 0; std::vector<ga_mapping_t> maps; std::vector<SeqSpan> seqs; };

// ---- host threads ----------------------------------------------------------------------------
// threads this process can really run at once: the affinity mask, capped by a cgroup CPU quota (ga_host.cpp)
size_t usableCores();

// how many host threads a loop over n items gets: one per `grain` items (+ 1), at most maxThreads, at most the usable cores or what
// GA_HOST_THREADS says in their place (0 or no number: one thread)
inline size_t hostThreads(size_t n, size_t maxThreads, size_t grain)
{
	size_t t = usableCores();
	if (const char* e = getenv("GA_HOST_THREADS")) t = (size_t)atoi(e);
	return std::max<size_t>(1, std::min<size_t>(std::min<size_t>(t, maxThreads), n / grain + 1));
}

// run fn(lo, hi, thread) over [0, n) on hostThreads(n, maxThreads, grain) threads, in pieces of pieceOf(threads) items handed out
// from a counter: where they are smaller than a thread's share, threads that get short ones take more of them.  `thread` numbers the
// threads from 0, for what a caller keeps once per thread.  Returns the number of threads.
template <typename P, typename F> size_t forChunks(size_t n, size_t maxThreads, size_t grain, P pieceOf, F fn)
{
	const size_t nThreads = hostThreads(n, maxThreads, grain), piece = pieceOf(nThreads);
	std::atomic<size_t> next{0};
	std::vector<std::thread> pool;
	for (size_t t = 0; t < nThreads; t++)
		pool.emplace_back([&, t]() { for (size_t lo; (lo = next.fetch_add(piece)) < n;) fn(lo, std::min(n, lo + piece), t); });
	for (auto& th : pool) th.join();
	return nThreads;
}
// pieceOf for one equal piece per thread
inline auto evenPieces(size_t n) { return [n](size_t threads) { return (n + threads - 1) / threads; }; }

// ---- result arrays ---------------------------------------------------------------------------
// Large result arrays are recycled: unmapping a gigabyte when results are freed and faulting a fresh one in for the next batch costs
// more than assembling the results.  A few buffers are kept (GA_RESULT_POOL_MB, default 4096; 0 = none), best fit first.
class BufferPool
{
	struct Item { void* p; size_t cap; };
	std::mutex lock;
	std::vector<Item> items;
	size_t held = 0;
	static size_t limit()
	{
		static const size_t v = []() { const char* e = getenv("GA_RESULT_POOL_MB"); return (size_t)(e ? atoll(e) : 4096) << 20; }();
		return v;
	}
public:
	void* take(size_t bytes, size_t& cap)
	{
		{
			std::lock_guard<std::mutex> g(lock);
			int best = -1;
			for (size_t i = 0; i < items.size(); i++)
				if (items[i].cap >= bytes && items[i].cap <= 2 * bytes + (1u << 20) && (best < 0 || items[i].cap < items[(size_t)best].cap)) best = (int)i;
			if (best >= 0)
			{
				Item it = items[(size_t)best];
				items.erase(items.begin() + best);
				held -= it.cap;
				cap = it.cap;
				return it.p;
			}
		}
		cap = bytes + bytes / 16 + 64;
		return malloc(cap);
	}
	void give(void* p, size_t cap)
	{
		if (!p) return;
		{
			std::lock_guard<std::mutex> g(lock);
			if (cap >= (1u << 20) && held + cap <= limit() && items.size() < 16) { items.push_back(Item{p, cap}); held += cap; return; }
		}
		free(p);
	}
};
inline BufferPool& resultPool() { static BufferPool* pool = new BufferPool();  return *pool; }    // (never destroyed: results may be freed at exit)
struct PooledBuffer
{
	void* p = nullptr;
	size_t cap = 0;
	void* get(size_t bytes) { resultPool().give(p, cap); p = resultPool().take(bytes, cap); return p; }
	~PooledBuffer() { resultPool().give(p, cap); }
};

struct ResultsOwner
{
	ga_results_t pub;
	std::vector<ga_read_result_t> reads;
	std::vector<ga_mapping_t> mappings;
	std::vector<char> edits;
	std::vector<ga_trace_item_t> trace;
	std::vector<ga_read_ops_t> readOps;
	std::vector<uint32_t> ops;
	std::vector<ga_read_path_seq_t> readPath;
	std::vector<char> pathBases;
	// the arrays of a whole batch (hundreds of MB, not cleared first): from the process-wide pool above, back to it with the results
	PooledBuffer allReads, allMappings, allTrace, allReadOps, allOps, allReadPath, allPathBases;
	std::shared_ptr<char> seqKeep;        // edit_bytes of a batch's results = the batch's copy of the reads, kept alive here
};

}  // namespace gahost

// ================================================================================================
// graph
// ================================================================================================
struct ga_graph
{
	int dbgOverlap = 0;
	bool finalized = false;
	std::vector<uint64_t> nodeStart;
	std::unordered_map<int64_t, uint32_t> lookup;
	std::vector<int64_t> ids;
	std::vector<std::pair<uint32_t, uint32_t>> edgeList;      // (from, to) node indices in the order the edges were added; the CSR lists are built at Finalize
	// nodes whose finished neighbour lists were handed over verbatim (ga_graph_set_neighbors): node index -> (in-list, out-list)
	std::unordered_map<uint32_t, std::pair<std::vector<uint32_t>, std::vector<uint32_t>>> givenLists;
	std::vector<uint8_t> reverse;
	std::vector<uint8_t> bases;         // 0..3, 4 for the dummy columns
	GaFlatGraph flat;
	GaHmmTables hmm;
	GaBackendGraph* device = nullptr;
	// per node index, made at Finalize for the plan of seeded batches (ga_plan.h): the node whose digraph id is this one's ^ 1
	// (0xffffffff: there is none), and digraph id & 1
	std::vector<uint32_t> twin;
	std::vector<uint8_t> idOdd;
	// site queries that fold columns (ga_sites.h): the per-node fold table and whether the graph meets the fold's preconditions, made
	// at the first such query (0: not looked at yet, 1: folds, -1: does not)
	mutable std::mutex foldLock;
	mutable int foldState = 0;
	mutable std::vector<uint32_t> foldTable;
	// optional node splitting (ga_graph_load_gfa_split): piece bigraph id -> the node it was cut from
	struct Piece { int64_t orig; uint64_t start, len, origLen; };
	std::unordered_map<int64_t, Piece> pieces;

	ga_graph()
	{
		// dummy start node, one column (AlignmentGraph.cpp:22-30)
		ids.push_back(0); nodeStart.push_back(0); reverse.push_back(0); bases.push_back(4);
	}
	uint32_t nodeCount() const { return (uint32_t)nodeStart.size(); }
	uint64_t nodeEnd(uint32_t n) const { return n + 1 == nodeStart.size() ? bases.size() : nodeStart[n + 1]; }
	uint32_t nodeLen(uint32_t n) const { return (uint32_t)(nodeEnd(n) - nodeStart[n]); }
	char baseChar(uint32_t node, uint32_t offset) const { uint8_t b = bases[nodeStart[node] + offset]; return b < 4 ? "ACGT"[b] : '-'; }
	// neighbour lists in insertion order, without double edges (AlignmentGraph.cpp:104-105); valid once finalized
	uint32_t inDegree(uint32_t n) const { return flat.in_off[n + 1] - flat.in_off[n]; }
	uint32_t inNeighbor(uint32_t n, uint32_t k) const { return flat.in_nbr[flat.in_off[n] + k]; }
	bool hasOutNeighbor(uint32_t n, uint32_t to) const
	{
		for (uint32_t e = flat.out_off[n]; e < flat.out_off[n + 1]; e++) if (flat.out_nbr[e] == to) return true;
		return false;
	}
	int reverseNode(uint32_t n, uint32_t& outNode) const
	{
		// GetReverseNode (AlignmentGraph.cpp:199-214)
		int64_t big = ids[n] / 2;
		auto it = lookup.find(ids[n] % 2 == 1 ? big * 2 : big * 2 + 1);
		if (it == lookup.end() || it->second == n || nodeLen(it->second) != nodeLen(n)) return GA_S_ASSERTION;
		outNode = it->second;
		return GA_S_OK;
	}
};

// ================================================================================================
// batch
// ================================================================================================
struct ga_batch
{
	const ga_graph* g = nullptr;
	std::vector<std::string> names;
	std::vector<gahost::ReadSeq> seqs;    // into seqBuf
	char* seqBuf = nullptr;               // the batch's own copy of the reads, one buffer; shared with the results collected from the batch:
	std::shared_ptr<char> seqKeep;        // an Edit's sequence is a piece of the read (GraphAligner.h:829, 845), so results point into it
	size_t seqBufBytes = 0;
	std::vector<gahost::ReadPlan> reads;
	std::vector<gahost::SeedPlan> seeds;
	struct RowFill { size_t read; uint64_t off, n, padded, pos; bool backward; };
	std::vector<RowFill> fills;         // where every job's rows come from
	std::vector<uint8_t> rows;          // row codes, built when a kernel that wants them is about to run (see buildRows)
	std::atomic<int> anyInvalidRow{0};    // some read has a character outside IUPAC (its results need the TraceItem pass)
	std::unique_ptr<std::atomic<uint8_t>[]> readInvalid;   // ... per read: a row of one of its jobs has such a character (noted while the match words are built)
	std::unique_ptr<uint64_t[]> eq;       // match words per slice (not cleared first: every slice is written by the host threads)
	size_t eqWords = 0;
	std::vector<GaJob> jobs;
	GaRunConfig cfg;
	uint32_t flags = 0;
	GaBackendBatch* dev = nullptr;
	bool ran = false;
	uint64_t columnUpdates = 0, slicesRun = 0, rowsTotal = 0;
	// a batch made by ga_batch_prepare_seeded: the seeding kernel's outputs as they were downloaded (ga_backend.h: GaSeededPlan) and the
	// times of ga_batch_prepare_stats_t
	bool seeded = false, byLocus = false;
	GaSeedParams seedParams{};
	std::vector<uint32_t> seedOutN, seedOut, seedOutLocus, seedNLoci;
	double seedMs = 0, planMs = 0, eqMs = 0, hostMs = 0;
	// GA_F_OPS: where the runs of the last collect's aligned reads came from
	uint64_t opsFromDevice = 0, opsFromHost = 0;
	// GA_F_PATHSEQ: ... and the bases
	uint64_t pathFromDevice = 0, pathFromHost = 0;
	// GA_F_PILEUP: what the last collect left for ga_batch_pileup_add (valid while `collected`): the winning jobs of the aligned reads
	// (job | 0x80000000, longest first), the items of the reads the host derives them for as (plane << 56 | column), and the two read counts
	bool collected = false;
	std::vector<uint32_t> pileList;
	std::vector<uint64_t> pilePairs;
	std::vector<uint32_t> pileSlots;      // ... and the crossings of those same reads as edge slots, for pileups of the EDGES kind
	uint64_t pileFromDevice = 0, pileFromHost = 0;
	~ga_batch() { delete dev; }
};

// ---- pileups (include/graphaligner_amd.h: "pileups"; ga_pileup.h) ------------------------------------------------------------------
struct ga_pileup
{
	const ga_graph* g = nullptr;
	int kind = 0;
	uint32_t planes = 0;                  // ga_pileup_planes_of_kind(kind); the entry count is st.columns
	GaBackendPileup* dev = nullptr;
	std::mutex lock;                      // (two batches may add at the same time: the statistics change hands under it)
	std::shared_mutex use;                // adds share the counters (their adds are atomic); reset and download take them alone
	ga_pileup_stats_t st{};
	~ga_pileup() { delete dev; }
};
