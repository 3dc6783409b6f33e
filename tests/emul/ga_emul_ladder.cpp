// ga_emul_ladder.cpp -- TEST-ONLY (ga_emul.h): the device extension program of graphaligner_amd/csrc/ga_kernel.h and the lanes = reads
// program of ga_lanes.h run on the host, every wave64 primitive emulated by ga_wave_emul.h, through the passes of DevBatch::run.  Which
// variant runs over which jobs, and in which order, is the product's policy (graphaligner_amd/csrc/ga_ladder.h, gald::climb); what is
// the emulation's own is EmulBatch::launch -- a loop over the pass's jobs, with capacities of its own -- and how a batch starts (see
// climb below).  The two passes with 4 096 band nodes can be withheld (GA_EMUL_WITHOUT=wide,wide_sparse): the tests compare the ladders.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "ga_emul.h"
#include "../../graphaligner_amd/csrc/ga_kernel.h"
#include "../../graphaligner_amd/csrc/ga_ladder.h"
#include "../../graphaligner_amd/csrc/ga_lanes.h"

namespace {

uint64_t gLastWideSparse = 0;      // jobs the last pass took in the last run()

// Two switches for what a job finds in its buffers (tests/test_emulated_wave_reuse.py).  On the device a wave's scratch slot and its
// LDS are never cleared: the first job of a wave finds whatever the allocation held, every later one the leavings of the job before.
//   GA_EMUL_POISON=1  every buffer a job or a lanes group gets is filled with 0xA5 before its first use (not the sparse method's
//                     generation-stamped tables: the device zeroes those once per launch, and so does the emulation)
//   GA_EMUL_REUSE=1   one WaveState and one set of slot buffers per wave-per-read variant, one scratch + LDS image per lanes variant,
//                     kept across all jobs / groups of a run() and never cleared in between; they grow to the largest job without
//                     losing what they hold.  The sparse tables are zeroed once per run().  A lanes variant's first (= longest) group
//                     sets cap_rows / cap_moves for all its groups, as a launch does, so later groups run with larger capacities
//                     than without the switch: capacities only grow, a job can at most be finished by an earlier pass, and the
//                     results are expected to be the same (every one is compared with the oracle).
bool envOn(const char* name) { const char* e = getenv(name); return e && atoi(e); }

template <typename T> void growTo(std::vector<T>& v, size_t n, bool poison)
{
	T fill;
	memset(&fill, poison ? 0xA5 : 0, sizeof(T));
	if (v.size() < n) v.resize(n, fill);
}

template <int MAXN> struct SlotBufs
{
	std::vector<uint32_t> endA, endB, arena, sliceOff, ckpt, below, ovr;
	std::vector<uint8_t> flags, staging, sparse;
	std::unique_ptr<gak::WaveState<MAXN>> ws;
};

struct LanesBufs
{
	std::vector<uint8_t> scratch;
	std::vector<uint32_t> lds;
	uint32_t capRows = 0, capMoves = 0;      // GA_EMUL_REUSE: the variant's first (= longest) group sets the layout for all, as a launch does
};

}  // namespace

namespace gae {

// GA_EMUL_REUSE: the buffers of every kernel variant, for one run()
struct KeptBuffers
{
	SlotBufs<32> lean32;
	SlotBufs<64> lean64, general64;
	SlotBufs<256> general256, sparse256;
	SlotBufs<4096> wide4096, wideSparse4096;
	LanesBufs lanes10, lanes24, lanes56;
	template <int MAXN, bool GENERAL, bool SPARSE> SlotBufs<MAXN>& slot()
	{
		if constexpr (MAXN == 32) { static_assert(!GENERAL && !SPARSE, "no such variant"); return lean32; }
		else if constexpr (MAXN == 64) { static_assert(!SPARSE, "no such variant"); if constexpr (GENERAL) return general64; else return lean64; }
		else if constexpr (MAXN == 4096) { static_assert(GENERAL, "no such variant"); if constexpr (SPARSE) return wideSparse4096; else return wide4096; }
		else { static_assert(MAXN == 256 && GENERAL, "no such variant"); if constexpr (SPARSE) return sparse256; else return general256; }
	}
	template <int N> LanesBufs& lanes()
	{
		static_assert(N == 10 || N == 24 || N == 56, "no such variant");
		if constexpr (N == 10) return lanes10; else if constexpr (N == 24) return lanes24; else return lanes56;
	}
};

template <int MAXN, bool GENERAL, bool SPARSE> void EmulBatch::runOne(uint32_t job, uint32_t capCols, uint64_t arenaWords, uint32_t traceCap)
{
	SlotBufs<MAXN> own;
	SlotBufs<MAXN>& b = reuse ? kept->slot<MAXN, GENERAL, SPARSE>() : own;
	growTo(b.endA, capCols, poison); growTo(b.endB, capCols, poison); growTo(b.arena, arenaWords, poison); growTo(b.sliceOff, cfg.max_slices + 1, poison);
	growTo(b.flags, cfg.max_slices + 1, poison);
	growTo(b.staging, traceCap + 64, poison);
	growTo(b.ckpt, cfg.max_slices + 2, poison); growTo(b.below, cfg.max_slices + 1, poison);
	const uint32_t maxBw = (uint32_t)std::max(std::max(cfg.initial_bw, cfg.ramp_bw), 1);
	growTo(b.sparse, SPARSE ? gak::sparse_mem_bytes<MAXN>(maxBw) : 0, false);
	growTo(b.ovr, SPARSE ? 2 * (cfg.max_slices + 2) : 0, poison);
	gak::Slot slot{b.endA.data(), b.endB.data(), b.arena.data(), b.sliceOff.data(), b.flags.data(), b.staging.data(), b.ckpt.data(), b.below.data(), SPARSE ? b.sparse.data() : nullptr, SPARSE ? b.ovr.data() : nullptr, maxBw};
	GaLaunch L;
	memset(&L, 0, sizeof(L));
	L.graph = g->dev; L.hmm = &g->hmm; L.rows = rows.data(); L.jobs = jobs.data(); L.outs = outs.data();
	L.traces = pool.data(); L.trace_top = &poolTop; L.trace_pool_cap = pool.size();
	L.n_jobs = (uint32_t)jobs.size(); L.trace_cap = traceCap; L.cap_cols = capCols; L.max_slices = cfg.max_slices;
	L.arena_words = arenaWords; L.initial_bw = cfg.initial_bw; L.ramp_bw = cfg.ramp_bw;
	if (!b.ws)
	{
		b.ws = std::make_unique<gak::WaveState<MAXN>>();
		if (poison) memset(b.ws.get(), 0xA5, sizeof(gak::WaveState<MAXN>));
	}
	gak::run_job<MAXN, GENERAL, SPARSE>(L, *b.ws, slot, job);
}

// the lanes = reads program (ga_lanes.h): a wave's 64 lanes are run one after the other through each phase; the points
// where the real wave decides something together (any lane still live, the slice's row range) sit between the phases
template <int N> void EmulBatch::runLanesGroup(const std::vector<uint32_t>& group, uint32_t capCols, uint32_t capRows, uint32_t capMoves)
{
	using namespace gal;
	GaLanesLaunch L;
	memset(&L, 0, sizeof(L));
	L.graph = g->dev; L.hmm = &g->hmm; L.eq = eq.data(); L.jobs = jobs.data(); L.outs = outs.data();
	L.n_jobs = (uint32_t)jobs.size(); L.lanes_per_wave = 64;
	L.traces = pool.data(); L.trace_top = &poolTop; L.trace_pool_cap = pool.size();
	L.cap_cols = capCols; L.cap_rows = capRows; L.max_slices = cfg.max_slices; L.cap_moves = capMoves;
	L.initial_bw = cfg.initial_bw; L.ramp_bw = cfg.ramp_bw;
	L.emit_runs = cfg.emit_runs;
	LanesBufs own;
	LanesBufs& b = reuse ? kept->lanes<N>() : own;
	if (reuse)
	{
		if (!b.capRows) { b.capRows = capRows; b.capMoves = capMoves; }
		capRows = L.cap_rows = std::max(capRows, b.capRows); capMoves = L.cap_moves = std::max(capMoves, b.capMoves);
	}
	const WaveLayout lay = wave_layout<N>(capCols, capRows, cfg.max_slices, capMoves);
	// (on the device the lanes of a wave take their arena blocks from one pool; run one after the other, every lane gets an arena of its own)
	const uint64_t laneArena = lay.bytes - lay.arena;
	growTo(b.scratch, lay.arena + 64 * laneArena + 256, poison);
	growTo(b.lds, (size_t)(Lay<N>::WORDS + kStageWordsLane) * 64, poison);         // tables + the words of the staging image behind them
	std::vector<uint8_t>& scratch = b.scratch;
	std::vector<uint32_t>& lds = b.lds;
	std::vector<LaneMem> mem(64);
	std::vector<LaneState> st(64);
	for (int lane = 0; lane < 64; lane++)
	{
		LaneMem& m = mem[lane];
		m.lane = lane; m.tid = lane; m.ls = 64;
		m.lds.base = lds.data() + lane; m.lds.lw = 64;
		m.endPrev = (uint32_t*)(scratch.data() + lay.endA) + lane;
		m.endCur = (uint32_t*)(scratch.data() + lay.endB) + lane;
		m.hdr = (uint32_t*)(scratch.data() + lay.hdr) + lane;
		m.snodes = (uint32_t*)(scratch.data() + lay.snodes) + lane;
		m.moves = (uint32_t*)(scratch.data() + lay.moves) + lane;
		m.arena = scratch.data() + lay.arena + (uint64_t)lane * laneArena;
		m.stage = nullptr;
		const bool has = lane < (int)group.size();
		lane_begin<N>(L, m, st[lane], has ? group[lane] : 0, has);
	}
	// (on the device one arena row belongs to one step of the wave; a lane run on its own simply counts its own steps)
	std::vector<uint32_t> rowTop(64, 0);
	for (uint32_t slice = 0; ; slice++)
	{
		bool any = false;
		for (int lane = 0; lane < 64; lane++)
		{
			lane_band<N>(L, mem[lane], st[lane], slice);
			any = any || st[lane].live;
		}
		if (!any) break;
		for (int lane = 0; lane < 64; lane++) fill_slice<N, 8>(L.graph, mem[lane], st[lane], slice, st[lane].live, rowTop[lane], L.cap_rows, L.cap_cols);
		for (int lane = 0; lane < 64; lane++) lane_end_slice<N>(L, mem[lane], st[lane], slice);
	}
	for (int lane = 0; lane < 64; lane++) lane_finish<N>(L, mem[lane], st[lane], lane < (int)group.size());
}

// The emulation's own geometry: deliberately small capacities in the early rungs, so that small test batches climb the ladder too.
// lanes = reads variants: a group's arena rows = slices of its longest job * rowsMul + 64, its moves = rows * movesMul + 512
struct LanesGeom { uint32_t capCols, rowsMul, movesMul; };
constexpr LanesGeom kLanesGeom[] = {{2048, 600, 2}, {4096, 2500, 3}, {8192, 2500, 3}};
// wave-per-read rungs, in the order of gald::kRungs, per job: arena words = 64 + slices * (kSliceHdrWords + arenaWordsPerSlice) *
// arenaMul, trace bytes = rows * traceMul + traceAdd
struct WaveGeom { uint32_t capCols; uint64_t arenaWordsPerSlice; uint32_t arenaMul, traceMul, traceAdd; };
constexpr WaveGeom kWaveGeom[] = {
	{2048, 3 * 40 + 5 * 700, 1, 2, 512},             // <32,false>
	{4096, 3 * 64 + 5 * 1500, 1, 3, 1024},           // <64,false>
	{4096, 3 * 64 + 5 * 1500, 2, 3, 1024},           // <64,true>
	{200000, 3 * 256 + 5 * 20000, 3, 8, 4096},       // <256,true>
	{200000, 3 * 4096 + 5 * 32768, 1, 8, 4096},      // <4096,true>: a bit-vector band of more than 256 nodes, or a projection heap of more than 1 024 entries
	{2000000, 3 * 256 + 6 * 300000, 1, 8, 4096},     // <256,true,true>: a band of 200 000 cells or more (ga_sparse.h)
	{2000000, 3 * 4096 + 6 * 300000, 1, 8, 4096},    // <4096,true,true>
};
static_assert(sizeof(kWaveGeom) / sizeof(kWaveGeom[0]) == sizeof(gald::kRungs) / sizeof(gald::kRungs[0]), "one geometry per wave-per-read rung");

// what a kernel launch over `list` is on the device: the lanes = reads program over groups of 64 jobs, the wave-per-read program
// over one job after the other
int EmulBatch::launch(gald::Variant v, const std::vector<uint32_t>& list, bool)
{
	if (getenv("GA_EMUL_DEBUG")) fprintf(stderr, "emul: pass %d, variant %d: %zu jobs\n", passNo - 1, (int)v, list.size());
	if (gald::isLanes(v))
	{
		const LanesGeom& geo = kLanesGeom[v];
		for (size_t at = 0; at < list.size(); at += 64)
		{
			std::vector<uint32_t> group(list.begin() + at, list.begin() + std::min(list.size(), at + 64));
			const uint32_t maxRows = jobs[group[0]].n_rows;
			const uint32_t capRows = (maxRows / 64) * geo.rowsMul + 64, capMoves = maxRows * geo.movesMul + 512;
			if (v == gald::kLanes10) runLanesGroup<10>(group, geo.capCols, capRows, capMoves);
			else if (v == gald::kLanes24) runLanesGroup<24>(group, geo.capCols, capRows, capMoves);
			else runLanesGroup<56>(group, geo.capCols, capRows, capMoves);
		}
		return 0;
	}
	if ((v == gald::kWide && (g->without & NO_WIDE)) || (v == gald::kWideSparse && (g->without & NO_WIDE_SPARSE))) return 0;
	if (v == gald::kWideSparse) gLastWideSparse = list.size();
	if (rows.empty()) rows = rowsProvider();         // the wave-per-read kernels read the row codes
	const WaveGeom& geo = kWaveGeom[v - gald::kLean32];
	for (uint32_t j : list)
	{
		const uint64_t arenaWords = 64 + (uint64_t)(jobs[j].n_rows / 64) * (gak::kSliceHdrWords + geo.arenaWordsPerSlice) * geo.arenaMul;
		const uint32_t traceCap = jobs[j].n_rows * geo.traceMul + geo.traceAdd;
		switch (v)
		{
		case gald::kLean32: runOne<32, false>(j, geo.capCols, arenaWords, traceCap); break;
		case gald::kLean64: runOne<64, false>(j, geo.capCols, arenaWords, traceCap); break;
		case gald::kGeneral64: runOne<64, true>(j, geo.capCols, arenaWords, traceCap); break;
		case gald::kGeneral256: runOne<256, true>(j, geo.capCols, arenaWords, traceCap); break;
		case gald::kWide: runOne<4096, true>(j, geo.capCols, arenaWords, traceCap); break;
		case gald::kSparse256: runOne<256, true, true>(j, geo.capCols, arenaWords, traceCap); break;
		default: runOne<4096, true, true>(j, geo.capCols, arenaWords, traceCap); break;
		}
	}
	return 0;
}

void EmulBatch::climb()
{
	outs.assign(jobs.size(), GaJobOut{});
	for (auto& o : outs) o.status = GA_NOT_RUN;
	uint64_t totalRows = 0;
	for (auto& j : jobs) totalRows += j.n_rows;
	pool.assign(totalRows * 3 + 4096 * jobs.size() + 64, 0);
	if (const char* t = getenv("GA_TEST_TRACE_POOL_BYTES")) pool.assign((size_t)atoll(t) & ~(size_t)3, 0);
	poolTop = 0;
	gLastWideSparse = 0;
	poison = envOn("GA_EMUL_POISON");
	reuse = envOn("GA_EMUL_REUSE");
	KeptBuffers buffers;
	kept = &buffers;
	// the hand-out order of the device queues: longest first
	std::vector<uint32_t> order(jobs.size());
	for (uint32_t i = 0; i < jobs.size(); i++) order[i] = i;
	std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return jobs[a].n_rows > jobs[b].n_rows; });
	passOf.assign(jobs.size(), 0);
	passNo = 0;
	// the emulation's first pass: GA_LANES as the product reads it, but with no choice by the graph's shape (unset: lanes first), the lanes
	// sizes always from <10,64>, and a later size for any number of jobs, so that small test batches still reach all three
	const char* e = getenv("GA_LANES");
	const gald::FirstPass fp = {!(e && atoi(e) == 0), gald::kLanes10, 0};
	gald::climb(order, outs, passOf, passNo, retried, fp, [&](gald::Variant v, const std::vector<uint32_t>& list, bool first) { return launch(v, list, first); });
	if (getenv("GA_EMUL_DEBUG") && (poison || reuse)) fprintf(stderr, "emul: poison %d, reuse %d\n", (int)poison, (int)reuse);
	kept = nullptr;
	if (getenv("GA_EMUL_DEBUG")) { int hist[100] = {0}; for (auto& o : outs) hist[o.status < 100 ? o.status : 99]++; fprintf(stderr, "emul: %zu jobs, %d passes, %llu retried, %llu by <4096,true,true>; final statuses:", jobs.size(), passNo, (unsigned long long)retried, (unsigned long long)gLastWideSparse); for (int i = 0; i < 100; i++) if (hist[i]) fprintf(stderr, " %d:%d", i, hist[i]); fprintf(stderr, "\n"); }
}

}  // namespace gae

// how many jobs of the last run() the last pass, <4096,true,true>, took (tests/test_wide_sparse.py)
extern "C" uint64_t ga_emul_wide_sparse_jobs_taken() { return gLastWideSparse; }
