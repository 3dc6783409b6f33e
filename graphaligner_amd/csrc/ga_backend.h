// ga_backend.h -- the seam between the host library (graph model, job building, result
// assembly: ga_host.cpp with its parts ga_prepare.h and ga_collect.h) and whatever executes the extension program.  The product links
// ga_device.hip (gfx950, HIP).  tests/emul/ links a host emulation of the same programs so the
// device logic can be checked in the CPU-only container; that object is never part of the
// shipped library.  (It can withhold a capability, tests/emul/ga_emul.h: it then answers with the defaults of the classes below.)
#pragma once
#if defined(__SSE2__)
#include <emmintrin.h>
#endif
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <functional>
#include <memory>
#include <vector>

#include "ga_types.h"

struct GaFlatGraph                      // host copy of what goes to HBM
{
	std::vector<uint64_t> node_start;   // n_nodes + 1
	std::vector<uint32_t> seq2;
	std::vector<uint32_t> in_off, in_nbr, out_off, out_nbr;
};

// the per-node records of GaDevGraph::node_rec
inline std::vector<uint32_t> ga_build_node_records(const GaFlatGraph& f)
{
	const size_t n = f.node_start.size() - 1;
	std::vector<uint32_t> rec(n * GA_NODE_REC_WORDS, 0);
	for (size_t i = 0; i < n; i++)
	{
		uint32_t* r = rec.data() + i * GA_NODE_REC_WORDS;
		r[0] = (uint32_t)f.node_start[i];
		r[1] = (uint32_t)(f.node_start[i] >> 32);
		r[2] = (uint32_t)(f.node_start[i + 1] - f.node_start[i]);
		const uint32_t inDeg = f.in_off[i + 1] - f.in_off[i], outDeg = f.out_off[i + 1] - f.out_off[i];
		r[3] = (inDeg < 0xffffu ? inDeg : 0xffffu) | ((outDeg < 0xffffu ? outDeg : 0xffffu) << 16);
		for (uint32_t k = 0; k < 4 && k < outDeg; k++) r[4 + k] = f.out_nbr[f.out_off[i] + k];
		for (uint32_t k = 0; k < 4 && k < inDeg; k++)
		{
			const uint32_t m = f.in_nbr[f.in_off[i] + k];
			r[8 + k] = m;
			r[12 + k] = (uint32_t)(f.node_start[m + 1] - f.node_start[m]);
		}
	}
	return rec;
}

struct GaRunConfig
{
	int initial_bw = 0, ramp_bw = 0;
	uint32_t max_slices = 0;            // max over jobs of n_rows / 64
	uint32_t max_rows = 0;
	uint32_t emit_runs = 0;             // 1: no result of the batch needs a cell list: the lanes = reads kernel hands back node runs instead of moves
	uint32_t emit_ops = 0;              // 1: GA_F_OPS: after the last pass the back end codes every job's operations as runs (ga_ops.h)
	uint32_t emit_pileup = 0;           // 1: GA_F_PILEUP: the batch keeps what addToPileup walks (the moves, the reads, the twin table); no launch in run
	uint32_t emit_pathseq = 0;          // 1: GA_F_PATHSEQ: after the last pass (and the operations) the back end writes every job's path sequence (ga_pathseq.h)
};

struct GaRunStats
{
	double kernel_ms = 0;               // all passes of the last run
	double main_ms = 0;                 // the first pass (lanes = reads kernel)
	int main_variant = 0;               // its template arguments: band nodes per lane * 1000 + record block * 10 + (1 when 32 lanes per wave)
	uint32_t slots = 0, waves_per_cu = 0;
	uint64_t scratch_bytes = 0;
	uint64_t jobs_retried = 0;
	uint64_t stamps[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // diagnostic builds: summed shader cycles per phase
};

// What the match words are built from when the back end builds them itself (GaBackendGraph::buildsMatchWords): the batch's copy of
// the reads and, per job, where its rows come from -- rows k < n are read characters (forward: seq[seq_off + pos + k] through rowCode;
// backward: seq[seq_off + n - 1 - k] through rowCodeRc), rows n .. padded - 1 are padCode; the job's first slice is eq_slice.
struct GaEqFill { uint64_t seq_off, eq_slice; uint32_t pos, n, padded, backward; };
struct GaEqSource
{
	const char* seq = nullptr; size_t seqBytes = 0;
	const GaEqFill* fills = nullptr; size_t nFills = 0;
	const uint8_t* rowCode = nullptr; const uint8_t* rowCodeRc = nullptr;       // 256 entries each
	uint8_t padCode = 0;
	const uint32_t* twin = nullptr;     // per node: the node whose digraph id is this one's ^ 1 (0xffffffff: none); what GA_F_OPS mirrors backward cells with
};

// What a batch run with GaRunConfig::emit_ops hands back (ga_ops.h): job j's runs are runs[offsets[j] .. offsets[j + 1]), in the final order
// of the job's part of the read's TraceItem list, each run type | length << 3; the HIP-event times of the counting and the writing launch;
// the jobs coded and the moves read.  The arrays stay the back end's (valid from fetch until fetchDone or the next fetch)
struct GaOpsOut { const uint32_t* runs = nullptr; const uint64_t* offsets = nullptr; uint64_t n_runs = 0; double count_ms = 0, write_ms = 0; uint64_t jobs = 0, moves = 0; };

// What a batch run with GaRunConfig::emit_pathseq hands back (ga_pathseq.h): job j's bases are bases[offsets[j] .. offsets[j + 1]), ASCII, in
// the final order of the job's part of the read's alignment; the HIP-event times of the counting and the writing launch; the jobs walked
// and the moves read.  The arrays stay the back end's (valid from fetch until fetchDone or the next fetch)
struct GaPathSeqOut { const uint8_t* bases = nullptr; const uint64_t* offsets = nullptr; uint64_t n_bases = 0; double count_ms = 0, write_ms = 0; uint64_t jobs = 0, moves = 0; };

// ---- pileups (ga_pileup.h): counters per column of the graph that stay with the graph; batches add to them after their collect --------
// what one add is given: the winning jobs (job index | 0x80000000 when the part has cells), longest first, and the items the host derived
// from TraceItem lists as (plane of the BASES kind << 56 | column)
constexpr uint32_t GA_PILEUP_COUNTS = 0x80000000u;   // in a list entry: this part of the read's alignment has cells
// ... and, for a pileup of the EDGES kind, the crossings of those same lists as slot indices
struct GaPileupAdd { const uint32_t* list = nullptr; size_t nList = 0; const uint64_t* pairs = nullptr; size_t nPairs = 0; const uint32_t* slots = nullptr; size_t nSlots = 0; };
// ... and hands back: the HIP-event time of its kernel(s), the jobs walked, the moves read, the items added (both sources)
struct GaPileupAddOut { double kernel_ms = 0; uint64_t jobs = 0, moves = 0, items = 0; };
#if defined(__HIPCC__)
#define GA_HOST_DEVICE __host__ __device__
#else
#define GA_HOST_DEVICE
#endif
GA_HOST_DEVICE inline uint64_t ga_pileup_pair(uint32_t basesPlane, uint64_t column) { return ((uint64_t)basesPlane << 56) | column; }
// the plane of an item of the BASES kind (8 planes) in a pileup of `kind` planes; 0xffffffff: not counted there (DEPTH: an insertion)
GA_HOST_DEVICE inline uint32_t ga_pileup_plane_in_kind(uint32_t kind, uint32_t basesPlane)
{
	if (kind == 8) return basesPlane < 8 ? basesPlane : 0xffffffffu;
	return basesPlane < 7 ? 0u : 0xffffffffu;
}
// A pileup's sizes in one place.  Its KIND names what is counted (the constants of include/graphaligner_amd.h), its PLANES are how many
// counters an entry has, its ENTRIES are what is counted over: the graph's columns or, for the EDGES kind, its slots -- the in-neighbour
// lists laid end to end, ga_edge_slot_count.  Everything that sizes, bounds or copies a pileup goes through these two functions.
constexpr int GA_KIND_DEPTH = 1, GA_KIND_BASES = 8, GA_KIND_EDGES = 32;
GA_HOST_DEVICE inline uint32_t ga_pileup_planes_of_kind(int kind) { return kind == GA_KIND_BASES ? 8u : kind == GA_KIND_DEPTH || kind == GA_KIND_EDGES ? 1u : 0u; }
GA_HOST_DEVICE inline uint64_t ga_pileup_entries(int kind, uint64_t columns, uint64_t slots) { return kind == GA_KIND_EDGES ? slots : columns; }
// what a back end makes a pileup from; mirrorSlot (EDGES only): per slot the slot of the other strand's copy of the edge, or 0xffffffff
struct GaPileupSpec { int kind = 0; uint32_t planes = 0; uint64_t entries = 0; const uint32_t* mirrorSlot = nullptr; };

// ---- slots (ga_edges.h): the edge from -> to has the slot in_off[to] + (place of `from` in to's in-list) --------------------------
inline uint64_t ga_edge_slot_count(const GaFlatGraph& f) { return f.in_off.empty() ? 0 : f.in_off.back(); }
// 0xffffffff: no such node or no such edge
inline uint32_t ga_edge_slot_of(const GaFlatGraph& f, uint32_t from, uint32_t to)
{
	if (f.in_off.empty() || to >= f.in_off.size() - 1) return 0xffffffffu;       // (no `to + 1`: 0xffffffff, "none", must not wrap)
	for (uint32_t e = f.in_off[to]; e < f.in_off[to + 1]; e++) if (f.in_nbr[e] == from) return e;
	return 0xffffffffu;
}
// per slot of from -> to the slot of twin(to) -> twin(from); 0xffffffff where a twin or that edge does not exist, or a dummy node is touched
inline std::vector<uint32_t> ga_edge_mirror_slots(const GaFlatGraph& f, const std::vector<uint32_t>& twin)
{
	const uint32_t n = f.in_off.empty() ? 0 : (uint32_t)f.in_off.size() - 1;
	std::vector<uint32_t> mirror((size_t)ga_edge_slot_count(f), 0xffffffffu);
	for (uint32_t to = 1; to + 1 < n; to++)
		for (uint32_t e = f.in_off[to]; e < f.in_off[to + 1]; e++)
		{
			const uint32_t from = f.in_nbr[e];
			if (from == 0 || from >= n - 1 || to >= twin.size() || from >= twin.size()) continue;
			// (a node whose other strand was never added has the twin 0xffffffff: compared without an add that would wrap)
			const uint32_t mTo = twin[from], mFrom = twin[to];
			if (mTo == 0 || mFrom == 0 || mTo >= n - 1 || mFrom >= n - 1) continue;
			mirror[e] = ga_edge_slot_of(f, mFrom, mTo);
		}
	return mirror;
}

// ---- site queries (ga_sites.h): fold the two strands' counters and keep the entries that pass a threshold ------------------------------
// one site as the back end leaves it: the entry and its folded counts (planes the kind does not have are 0)
struct GaSiteRec { uint64_t entry; uint32_t counts[8]; };
// the per-node fold table of a columns query: the node of the other strand (0x7fffffff: none) | 0x80000000 on a forward copy
constexpr uint32_t GA_FOLD_NONE = 0x7fffffffu, GA_FOLD_FORWARD = 0x80000000u;
// a query the host has validated (include/graphaligner_amd.h: ga_site_params_t); foldTable: fold queries over a columns kind only, one
// word per node, the same array at every query of a graph (a back end may keep its copy)
struct GaSiteQuery
{
	bool fold = false;
	uint64_t min_depth = 1, min_alt = 0;
	uint32_t alt_num = 0, alt_den = 1;
	uint64_t first = 0, n = 0, max_sites = 0;
	const uint32_t* foldTable = nullptr; size_t nNodes = 0;
};
struct GaSitesOut { std::vector<GaSiteRec> recs; uint64_t n_total = 0; double kernel_ms = 0; };

class GaBackendPileup
{
public:
	virtual ~GaBackendPileup() {}
	virtual int reset() = 0;
	// out[plane * n + i] = the counter of (plane, first + i), for every plane of the kind; first + n <= entries
	virtual int download(uint64_t first, uint64_t n, uint32_t* out) const = 0;
	// the sites of the query in ascending entry order, the first max_sites of them; a back end without it refuses (100 = GA_E_INVALID)
	virtual int sites(const GaSiteQuery&, GaSitesOut&) { return 100; }
};

// ---- seeding (ga_seed.h): a k-mer index of the uploaded graph and, per batch of reads, the seeds it gives ------------------------
struct GaSeedIndexInfo { uint64_t kmers_seen = 0, entries = 0, distinct_keys = 0, bytes = 0; double build_ms = 0; uint32_t k = 0, sample_shift = 0, dir_bits = 0; };
// of a walk index (max_walks = 0: the index is an in-node one); walk_kmers: walks of the tail starts that were not skipped
struct GaSeedWalkInfo { uint32_t max_walks = 0; uint64_t tail_starts = 0, tail_starts_skipped = 0, walk_kmers = 0, duplicates_dropped = 0; };
// per read r: n_seeds[r] seeds at [r * max_seeds ..): node INDEX, read position and support of each; the number of hits used; truncated.
// findLoci also fills, per seed, the hits of its locus and the locus' smallest and largest read position and, per read, the number of
// loci that have a candidate; find leaves those four empty
struct GaSeedOut
{
	std::vector<uint32_t> n_seeds, n_hits, truncated;
	std::vector<uint32_t> node, pos, support;
	std::vector<uint32_t> locus_hits, locus_first_p, locus_last_p, n_loci;
	double kernel_ms = 0;
};
// the coordinate of the current index (include/graphaligner_amd.h: ga_seed_coord_stats_t); kind 0 = file order, where the rest is 0
struct GaSeedCoordInfo { int kind = 0; uint32_t trees = 0, cycles_cut = 0, cycle_rounds = 0, depth_rounds = 0; uint64_t extent_sum = 0; double build_ms = 0; };
class GaSeedEngine
{
public:
	virtual ~GaSeedEngine() {}
	// linx[node] = 2 * lin + strand flag (include/graphaligner_amd.h: the linear coordinate); one per node, dummy nodes included
	virtual int build(uint32_t k, uint32_t sampleShift, const std::vector<int64_t>& linx) = 0;
	// the same with the k-mers of walks across edges (maxWalks 1..256); a back end without it refuses (100 = GA_E_INVALID)
	virtual int buildWalks(uint32_t, uint32_t, uint32_t, const std::vector<int64_t>&) { return 100; }
	virtual GaSeedWalkInfo walkInfo() const { return GaSeedWalkInfo(); }
	virtual bool built() const = 0;
	virtual GaSeedIndexInfo info() const = 0;
	virtual int copy(uint64_t* keys, uint32_t* nodes, uint32_t* offsets, size_t capacity) const = 0;
	// reads: seqs[i] of lens[i] characters
	virtual int find(const char* const* seqs, const size_t* lens, size_t nReads, const GaSeedParams& p, GaSeedOut& out) = 0;
	// the same with one seed per locus (ga_find_seeds_loci); a back end without it refuses (100 = GA_E_INVALID)
	virtual int findLoci(const char* const*, const size_t*, size_t, const GaSeedParams&, GaSeedOut&) { return 100; }
	// replaces the coordinate of the current index: 0 file order (the array build() was given), 1 topology (ga_seed.h); a back end
	// without the topology pass keeps the file order it has and refuses the rest (100 = GA_E_INVALID)
	virtual int setCoordinate(int kind, GaSeedCoordInfo& out) { if (kind != 0 || !built()) return 100; out = GaSeedCoordInfo(); return 0; }
	virtual GaSeedCoordInfo coordInfo() const { return GaSeedCoordInfo(); }
	// lin of the first min(n_nodes, capacity) nodes as the index holds it now
	virtual int copyLin(int64_t*, size_t) const { return 100; }
};

// ---- seeded batches (ga_plan.h): seeds found and jobs planned on the back end's side, from one upload of the reads ---------------
// what the host hands over: the batch's block (reads in the seeder's layout -- every read at a multiple of 16 with 16 bytes of padding
// behind it --, then the read records and the hand-out order, as DevSeedEngine lays a batch out), the graph's twin table and the tables
struct GaSeededRequest
{
	const char* block = nullptr;
	size_t seqBytes = 0, oRecs = 0, oOrder = 0, blockBytes = 0;   // (offsets of the records and the order inside the block; its used size)
	size_t nReads = 0;
	GaSeedParams p{};
	bool byLocus = false;
	uint32_t overlap = 0;
	const uint32_t* twin = nullptr; const uint8_t* rev = nullptr;       // per node (ga_plan.h: PlanLaunch)
	const uint8_t* hasComplement = nullptr;                             // 256 entries
	const uint8_t* rowCode = nullptr; const uint8_t* rowCodeRc = nullptr; uint8_t padCode = 0;
	uint64_t rowsBound = 0;                                             // no plan of these reads has more rows (padded) than this
};
// what comes back, in one download: pointers into a block that `keep` holds
struct GaSeededPlan
{
	std::shared_ptr<char> keep;
	const uint32_t* outN = nullptr;        // [nReads][3] seeds, hits used, truncated
	const uint32_t* outSeed = nullptr;     // [nReads][max_seeds][3] node index, read position, support
	const uint32_t* outLocus = nullptr;    // by locus: [nReads][max_seeds][3]
	const uint32_t* outNLoci = nullptr;    // by locus: [nReads]
	const GaPlanSeed* seeds = nullptr;     // [nReads][max_seeds]
	const GaJob* jobs = nullptr; const GaEqFill* fills = nullptr; const uint32_t* fillRead = nullptr; size_t nJobs = 0;
	const uint8_t* badFills = nullptr;     // per fill: a row outside IUPAC (back ends that build the match words; else null)
	uint64_t rowsTotal = 0;
	double seed_ms = 0, plan_ms = 0, eq_ms = 0;
};

// (see ga_backend_create_batch below)
typedef std::function<const std::vector<uint8_t>&()> GaRowsProvider;
class GaBackendBatch;
class GaBackendGraph
{
public:
	virtual ~GaBackendGraph() {}
	// first half of a seeded batch: upload, seeding, plan, match words (where the back end builds them), download.  The batch it returns
	// runs once finishSeeded has been given the host's copy of the jobs.  A back end without the feature refuses (100 = GA_E_INVALID)
	virtual GaBackendBatch* beginSeededBatch(const GaSeededRequest&, GaSeededPlan&, int* status) { *status = 100; return nullptr; }
	// nullptr: this back end has no seeding (the host emulation of tests/emul with seeding withheld)
	virtual GaSeedEngine* seedEngine() { return nullptr; }
	// true: ga_backend_create_batch wants a GaEqSource and builds the match words on its side (the product: a kernel over the uploaded
	// reads); false: it wants the finished words (the host emulation of tests/emul with its own words withheld)
	virtual bool buildsMatchWords() const { return false; }
	// true: this back end codes operations (GaRunConfig::emit_ops); on one that does not, a prepare with GA_F_OPS is refused
	virtual bool codesOps() const { return false; }
	// spec.planes planes of spec.entries zeroed counters each, or nullptr + *status (102 = GA_E_DEVICE: no memory).  A back end without
	// pileups has no factory (100 = GA_E_INVALID) and a prepare with GA_F_PILEUP is refused on it
	virtual GaBackendPileup* createPileup(const GaPileupSpec&, int* status) { *status = 100; return nullptr; }
	virtual bool codesPileup() const { return false; }
	// true: this back end writes path sequences (GaRunConfig::emit_pathseq); on one that does not, a prepare with GA_F_PATHSEQ is refused
	virtual bool writesPathSeq() const { return false; }
	// host memory for a batch's copy of the reads (the product: pinned blocks from a pool, so that their upload is one DMA transfer)
	virtual std::shared_ptr<char> hostBlock(size_t bytes)
	{
		void* mem = nullptr;
		const size_t two = (size_t)2 << 20;
		if (posix_memalign(&mem, two, (bytes + two - 1) & ~(two - 1)) != 0) return std::shared_ptr<char>();
		return std::shared_ptr<char>((char*)mem, [](char* p) { free(p); });
	}
};
class GaBackendBatch
{
public:
	virtual ~GaBackendBatch() {}
	// second half of a seeded batch (GaBackendGraph::beginSeededBatch); eq: the finished match words for a back end that does not build them
	virtual int finishSeeded(const std::vector<GaJob>&, const GaRunConfig&, GaRowsProvider, const uint64_t*, size_t) { return 100; }
	// back ends that build the match words: per fill of the GaEqSource, 1 when one of its rows is a character outside IUPAC
	virtual const std::vector<uint8_t>* invalidFills() const { return nullptr; }
	// GaRunConfig::emit_runs as it ended up (a back end that builds the match words clears it when a row is such a character)
	virtual bool emittingRuns() const = 0;
	virtual int run() = 0;                                                   // device work only; returns ga_status
	// moves of job i: (*traceBytes)[outs[i].trace_off ..+trace_len); the bytes stay the backend's (valid until fetchDone or the next fetch)
	virtual int fetch(std::vector<GaJobOut>& outs, const uint8_t** traceBytes, uint64_t* nBytes) = 0;
	// after fetch, of a batch run with emit_ops: the runs, their places and the launches' times; a back end without it refuses
	virtual int fetchOps(GaOpsOut&) { return 100; }
	// after fetch, of a batch run with emit_pathseq: the bases, their places and the launches' times; a back end without it refuses
	virtual int fetchPathSeq(GaPathSeqOut&) { return 100; }
	virtual void fetchDone() {}
	// of a batch run with emit_pileup, after fetch and until the next run: adds the listed jobs' items to a pileup of this batch's graph
	virtual int addToPileup(GaBackendPileup*, const GaPileupAdd&, GaPileupAddOut&) { return 100; }
	virtual GaRunStats stats() const = 0;
};

// what the seeding entry points (ga_seed_host.cpp) need of a graph, which is ga_host.cpp's own
struct ga_graph;
struct GaGraphView { bool finalized; const std::vector<int64_t>* ids; const GaFlatGraph* flat; GaBackendGraph* device; };
GaGraphView ga_graph_view(const ga_graph* g);

// what ga_batch_seeds (ga_seed_host.cpp) needs of a batch made by ga_batch_prepare_seeded, which is ga_host.cpp's own
struct ga_batch;
struct GaBatchSeedView
{
	bool seeded = false, byLocus = false;
	const ga_graph* g = nullptr;
	size_t nReads = 0; uint32_t maxSeeds = 0;
	const uint32_t* outN = nullptr; const uint32_t* outSeed = nullptr; const uint32_t* outLocus = nullptr; const uint32_t* outNLoci = nullptr;
	double kernel_ms = 0;
};
GaBatchSeedView ga_batch_seed_view(const ga_batch* b);

// returns nullptr + sets *status (GA_E_NO_DEVICE ...) on failure
GaBackendGraph* ga_backend_upload_graph(const GaFlatGraph& g, const GaHmmTables& hmm, int device, int* status);
// eq: per job and 64-row slice five 64-bit words (job j, slice s at (jobs[j].rows_off / 64 + s) * 5): the match words of the slice's rows
// against A, C, G, T and a meta word (bits 0-2 exact-compare code of the slice's last row, bit 3 = a row with an invalid character)
// rows: the row codes (one byte per padded read base) are only needed by the wave-per-read ladder kernels, so they are built and uploaded
// on demand: the provider returns them (building them at its first call)
// (eq or src: the finished words, or what a back end that builds them itself builds them from)
GaBackendBatch* ga_backend_create_batch(GaBackendGraph* g, GaRowsProvider rows, const uint64_t* eq, const GaEqSource* src, size_t eqWords, const std::vector<GaJob>& jobs,
                                        const GaRunConfig& cfg, int* status);

// the match words of ga_backend_create_batch from the row codes
inline void ga_build_eq_words(const uint8_t* rows, uint64_t nRows, uint64_t* eq)
{
	for (uint64_t s = 0; s < nRows / 64; s++)
	{
		uint64_t e[4] = {0, 0, 0, 0};
		uint32_t invalid = 0;
		const uint8_t* r = rows + s * 64;
#if defined(__SSE2__) && !defined(__HIP_DEVICE_COMPILE__)
		// bit b of 16 codes at a time: shifted up to the bytes' sign bits, collected by movemask
		__m128i any = _mm_setzero_si128();
		for (int q = 0; q < 4; q++)
		{
			const __m128i v = _mm_loadu_si128((const __m128i*)(r + 16 * q));
			any = _mm_or_si128(any, v);
			e[0] |= (uint64_t)(uint32_t)_mm_movemask_epi8(_mm_slli_epi16(v, 7)) << (16 * q);
			e[1] |= (uint64_t)(uint32_t)_mm_movemask_epi8(_mm_slli_epi16(v, 6)) << (16 * q);
			e[2] |= (uint64_t)(uint32_t)_mm_movemask_epi8(_mm_slli_epi16(v, 5)) << (16 * q);
			e[3] |= (uint64_t)(uint32_t)_mm_movemask_epi8(_mm_slli_epi16(v, 4)) << (16 * q);
		}
		invalid = (uint32_t)_mm_movemask_epi8(any);            // GA_ROW_INVALID is the codes' top bit
#else
		for (int i = 0; i < 64; i++)
		{
			const uint8_t c = r[i];
			for (int b = 0; b < 4; b++) e[b] |= (uint64_t)((c >> b) & 1) << i;
			invalid |= c & GA_ROW_INVALID;
		}
#endif
		uint64_t* o = eq + s * 5;
		o[0] = e[0]; o[1] = e[1]; o[2] = e[2]; o[3] = e[3];
		o[4] = (uint64_t)((r[63] >> 4) & 7) | (invalid ? 8u : 0u);
	}
}
