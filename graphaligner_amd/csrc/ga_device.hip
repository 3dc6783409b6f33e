// ga_device.hip -- gfx950 back end: keeps the flattened graph resident in HBM and runs the
// extension program (ga_kernel.h) as a persistent launch: one 64-lane workgroup (= one
// wavefront) per slot, each slot pulling read directions from a device-side queue and owning a
// private region of HBM for its slices' VP/VN words.  Reads are independent, so there is no
// inter-workgroup communication besides the queue counter and the trace-pool bump counter.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <vector>

#include "../../include/graphaligner_amd.h"
#include "ga_backend.h"
#include "ga_kernel.h"
#include "ga_ladder.h"
#include "ga_lanes.h"
#include "ga_seed_dev.h"
#include "ga_plan.h"
#include "ga_ops.h"
#include "ga_pileup.h"
#include "ga_edges.h"
#include "ga_sites.h"

namespace {

#define HIP_OK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { fprintf(stderr, "graphaligner_amd: %s failed: %s\n", #call, hipGetErrorString(e_)); return GA_E_DEVICE; } } while (0)

struct SlotLayout
{
	uint64_t endPrev, endCur, sliceOff, arena, trace, flags, ckpt, belowOff, sparse, ovr, state, bytes;
};
// (sparseNodes: the band nodes of the variant whose sparse tables are laid out -- they are sized per variant, gak::SparseLimits)
__host__ __device__ inline SlotLayout slotLayout(uint32_t capCols, uint32_t maxSlices, uint64_t arenaWords, uint32_t traceCap, uint32_t sparseBw = 0, uint64_t stateBytes = 0, int sparseNodes = 256)
{
	auto up = [](uint64_t x) { return (x + 255) & ~255ull; };
	SlotLayout l;
	uint64_t at = 0;
	l.endPrev = at; at = up(at + 4ull * capCols);
	l.endCur = at; at = up(at + 4ull * capCols);
	l.sliceOff = at; at = up(at + 4ull * (maxSlices + 1));
	l.arena = at; at = up(at + 4ull * arenaWords);
	l.trace = at; at = up(at + 1ull * traceCap + 64);
	l.flags = at; at = up(at + maxSlices + 1);
	l.ckpt = at; at = up(at + 4ull * (maxSlices + 2));
	l.belowOff = at; at = up(at + 4ull * (maxSlices + 1));
	// the variant that carries the sparse method: its tables (first, so that the host can clear them) and the override windows
	l.sparse = at; if (sparseBw) at = up(at + (sparseNodes > 256 ? gak::sparse_mem_bytes<4096>(sparseBw) : gak::sparse_mem_bytes<256>(sparseBw)));
	l.ovr = at; if (sparseBw) at = up(at + 8ull * (maxSlices + 2));
	// the variant whose band tables do not fit in LDS: its WaveState (0 bytes for every other variant)
	l.state = at; if (stateBytes) at = up(at + stateBytes);
	l.bytes = at;
	return l;
}

#ifndef GA_WAVES_EU
#define GA_WAVES_EU 4
#endif
template <int MAXN, bool GENERAL, bool SPARSE = false>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(GA_WAVES_EU, 8))) ga_extend_kernel(GaLaunch L)
{
	__shared__ gak::WaveState<MAXN> ws;
	const SlotLayout lay = slotLayout(L.cap_cols, L.max_slices, L.arena_words, L.trace_cap, SPARSE ? L.sparse_bw : 0u);
	uint8_t* base = L.scratch + (uint64_t)blockIdx.x * L.slot_bytes;
	gak::Slot slot;
	slot.end_prev = (uint32_t*)(base + lay.endPrev);
	slot.end_cur = (uint32_t*)(base + lay.endCur);
	slot.slice_off = (uint32_t*)(base + lay.sliceOff);
	slot.arena = (uint32_t*)(base + lay.arena);
	slot.trace = base + lay.trace;
	slot.slice_flags = base + lay.flags;
	slot.ckpt = (uint32_t*)(base + lay.ckpt);
	slot.below_off = (uint32_t*)(base + lay.belowOff);
	slot.sparse = SPARSE ? base + lay.sparse : nullptr;
	slot.ovr = SPARSE ? (uint32_t*)(base + lay.ovr) : nullptr;
	slot.sparse_max_bw = SPARSE ? L.sparse_bw : 0u;
	while (true)
	{
		uint32_t k = gaw::wave_atomic_add(L.next_job, 1u);
		if (k >= L.n_jobs) break;                      // every wave reaches this exit once the queue is drained
		uint32_t job = L.job_list ? L.job_list[k] : k;
		gak::run_job<MAXN, GENERAL, SPARSE>(L, ws, slot, job);
		__syncthreads();
	}
}

// ---- bands of up to 4 096 nodes: the same program with its band tables (WaveState<4096>, some 780 KB) in the wave's scratch slot in
// HBM instead of LDS.  The last bit-vector pass of the ladder, for the few jobs whose band overflowed 256 nodes or whose projection
// heap overflowed: one wave per CU at most.  The state is not cleared between jobs, as LDS is not; lanes hand values to each other
// through it, which ws_order / ws_handover (ga_kernel.h) order with a workgroup-scope fence in this kernel.
constexpr int kWideNodes = 4096;
constexpr uint32_t kCutoffCols = gak::kCutoff;       // (a band of this many columns is no bit-vector band)
__global__ void __launch_bounds__(64) ga_wide_kernel(GaLaunch L)
{
	const SlotLayout lay = slotLayout(L.cap_cols, L.max_slices, L.arena_words, L.trace_cap, 0u, sizeof(gak::WaveState<kWideNodes>));
	uint8_t* base = L.scratch + (uint64_t)blockIdx.x * L.slot_bytes;
	gak::WaveState<kWideNodes>& ws = *(gak::WaveState<kWideNodes>*)(base + lay.state);
	gak::Slot slot;
	slot.end_prev = (uint32_t*)(base + lay.endPrev);
	slot.end_cur = (uint32_t*)(base + lay.endCur);
	slot.slice_off = (uint32_t*)(base + lay.sliceOff);
	slot.arena = (uint32_t*)(base + lay.arena);
	slot.trace = base + lay.trace;
	slot.slice_flags = base + lay.flags;
	slot.ckpt = (uint32_t*)(base + lay.ckpt);
	slot.below_off = (uint32_t*)(base + lay.belowOff);
	slot.sparse = nullptr;
	slot.ovr = nullptr;
	slot.sparse_max_bw = 0u;
	while (true)
	{
		uint32_t k = gaw::wave_atomic_add(L.next_job, 1u);
		if (k >= L.n_jobs) break;                      // every wave reaches this exit once the queue is drained
		uint32_t job = L.job_list ? L.job_list[k] : k;
		gak::run_job<kWideNodes, true, false>(L, ws, slot, job);
		__syncthreads();
	}
}

// ---- bands of 200 000 cells and more with up to 4 096 nodes: the sparse method and the backtrace override (ga_sparse.h) over the
// state in HBM.  The very last pass, for the jobs that ga_extend_kernel<256,true,true> left with GA_CAP_NODES: fans and tangles of
// hundreds to thousands of nodes.  Launch shape, queue and state as in ga_wide_kernel; the sparse tables are those of
// gak::SparseLimits<4096>.
__global__ void __launch_bounds__(64) ga_wide_sparse_kernel(GaLaunch L)
{
	const SlotLayout lay = slotLayout(L.cap_cols, L.max_slices, L.arena_words, L.trace_cap, L.sparse_bw, sizeof(gak::WaveState<kWideNodes>), kWideNodes);
	uint8_t* base = L.scratch + (uint64_t)blockIdx.x * L.slot_bytes;
	gak::WaveState<kWideNodes>& ws = *(gak::WaveState<kWideNodes>*)(base + lay.state);
	gak::Slot slot;
	slot.end_prev = (uint32_t*)(base + lay.endPrev);
	slot.end_cur = (uint32_t*)(base + lay.endCur);
	slot.slice_off = (uint32_t*)(base + lay.sliceOff);
	slot.arena = (uint32_t*)(base + lay.arena);
	slot.trace = base + lay.trace;
	slot.slice_flags = base + lay.flags;
	slot.ckpt = (uint32_t*)(base + lay.ckpt);
	slot.below_off = (uint32_t*)(base + lay.belowOff);
	slot.sparse = base + lay.sparse;
	slot.ovr = (uint32_t*)(base + lay.ovr);
	slot.sparse_max_bw = L.sparse_bw;
	while (true)
	{
		uint32_t k = gaw::wave_atomic_add(L.next_job, 1u);
		if (k >= L.n_jobs) break;                      // every wave reaches this exit once the queue is drained
		uint32_t job = L.job_list ? L.job_list[k] : k;
		gak::run_job<kWideNodes, true, true>(L, ws, slot, job);
		__syncthreads();
	}
}

// ---- lanes = reads (ga_lanes.h): every lane owns one job, the wave's lanes advance slice by slice together -----------
// N band nodes per lane in LDS (10 N words per lane), slice records in blocks of R columns per lane, LW = lane stride of
// the LDS tables = how many lanes of a wave carry jobs.
// FORM: what the traceback hands back, 1 node runs or 0 moves, fixed when the kernel is compiled (lane_finish).  Each size is built
// twice: ga_lanes_kernel<N, LW> hands back node runs, ga_lanes_moves_kernel<N, LW> moves; the launch picks by GaLanesLaunch::emit_runs.
template <int N> constexpr int kLanesLdsWords(int lw) { return gal::Lay<N>::WORDS * lw + lw * gal::kStageWords64 * 2 + 128; }  // tables, the staging image of LW lanes, the lanes' arena blocks
template <int N, int LW, int FORM>
__device__ __forceinline__ void lanes_wave(const gal::GaLanesLaunch& L, uint32_t* lds)
{
	using namespace gal;
	const int lane = (int)threadIdx.x;
	const WaveLayout lay = wave_layout<N>(L.cap_cols, L.cap_rows, L.max_slices, L.cap_moves, LW);
	uint8_t* base = L.scratch + (uint64_t)blockIdx.x * L.wave_bytes;
	while (true)
	{
		const uint32_t grp = gaw::wave_atomic_add(L.next_group, 1u);
		const uint64_t first = (uint64_t)grp * L.lanes_per_wave;
		if (first >= L.n_jobs) break;                      // every wave reaches this exit once the queue is drained
		const bool hasJob = lane < (int)L.lanes_per_wave && lane < LW && first + (uint32_t)lane < L.n_jobs;
		const uint32_t jobIndex = hasJob ? (L.job_list ? L.job_list[first + (uint32_t)lane] : (uint32_t)(first + (uint32_t)lane)) : 0u;
		LaneMem m;
		m.lane = lane < LW ? lane : 0;      // (lanes beyond the variant's LW carry no job: they shadow lane 0's addresses and store nothing)
		m.tid = lane;
		m.flushPart = (uint32_t)lane % 12u; m.flushLane = (uint32_t)lane / 12u;
		m.ls = LW;
		m.lds.base = lds + (lane < LW ? lane : 0);
		m.lds.lw = LW;
		m.stage = (uint64_t*)(lds + Lay<N>::WORDS * LW);
		m.laneBlocks = lds + Lay<N>::WORDS * LW + LW * kStageWords64 * 2;
		m.usedChunks = 12u * (L.lanes_per_wave < (uint32_t)LW ? L.lanes_per_wave : (uint32_t)LW);
		m.endPrev = (uint32_t*)(base + lay.endA) + m.lane;
		m.endCur = (uint32_t*)(base + lay.endB) + m.lane;
		m.hdr = (uint32_t*)(base + lay.hdr) + m.lane;
		m.snodes = (uint32_t*)(base + lay.snodes) + m.lane;
		m.moves = (uint32_t*)(base + lay.moves) + m.lane;
		m.arena = base + lay.arena;
		LaneState st;
#if GA_STAMPS == 3
		const uint64_t wall0 = wall_clock64(), cyc0 = gaw::stamp();
#endif
		uint64_t tA = gaw::stamp(), tB, acc[4] = {0, 0, 0, 0};
#define GAL_LAP(i) do { tB = gaw::stamp(); acc[i] += tB - tA; tA = tB; } while (0)
		lane_begin<N>(L, m, st, jobIndex, hasJob);
		uint32_t blockTop = 0;                             // wave-uniform: the arena's next free block of 8 rows
		for (uint32_t slice = 0; ; slice++)
		{
			lane_band<N>(L, m, st, slice);
			GAL_LAP(0);
			if (!__ballot(st.live)) break;
			fill_slice<N, 8, LW>(L.graph, m, st, slice, st.live, blockTop, L.cap_rows, L.cap_cols);
			GAL_LAP(1);
			lane_end_slice<N>(L, m, st, slice);
			GAL_LAP(2);
		}
		lane_finish<N, FORM>(L, m, st, hasJob);
		GAL_LAP(3);
#undef GAL_LAP
#ifdef GA_STAMPS
		// diagnostic build: the wave's cycles per phase, booked on its first job (names in bench.py)
		if (hasJob && lane == 0) { GaJobOut* o = L.outs + st.job; o->stamps[1] = acc[0]; o->stamps[4] = acc[1]; o->stamps[0] = acc[2]; o->stamps[5] = acc[3]; o->stamps[2] = st.laps[0]; o->stamps[3] = st.laps[1]; o->stamps[6] = st.laps[2]; o->stamps[7] = st.laps[7];
#if GA_STAMPS == 4
			// fourth diagnostic layout: the parts of the band phase in [0..4], the band phase in [6], the fill in [7]
			o->stamps[6] = acc[0]; o->stamps[7] = acc[1];
			for (int i = 0; i < 5; i++) o->stamps[i] = st.blaps[i];
#endif
#if GA_STAMPS == 3
			// third diagnostic layout: when the wave ran, on the constant 100 MHz clock, and how many shader cycles that was
			o->stamps[0] = wall0; o->stamps[1] = wall_clock64(); o->stamps[4] = gaw::stamp() - cyc0;
#endif
#if GA_STAMPS == 2
			// second diagnostic layout: the parts of the traceback's general step instead of end_slice / band / fill
			o->stamps[0] = st.laps[4]; o->stamps[1] = st.laps[5]; o->stamps[4] = st.laps[6];
#endif
		}
#endif
		__syncthreads();
	}
}
template <int N, int LW>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 2))) ga_lanes_kernel(gal::GaLanesLaunch L)
{
	__shared__ uint32_t lds[kLanesLdsWords<N>(LW)];
	lanes_wave<N, LW, 1>(L, lds);
}
template <int N, int LW>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 2))) ga_lanes_moves_kernel(gal::GaLanesLaunch L)
{
	__shared__ uint32_t lds[kLanesLdsWords<N>(LW)];
	lanes_wave<N, LW, 0>(L, lds);
}

// ---- the match words of the lanes = reads kernel, built from the reads' bytes (ga_backend.h: GaEqSource) -------------------------
// One wave per job (its rows come from one read, forwards from the seed or backwards before it); lane r of the wave holds row r of the
// slice in hand: the character's row code through a 512-byte table in LDS, four ballots = the slice's match words against A, C, G, T
// (characterMatch, GraphAligner.h:2039-2110; what the reference builds as EqVector, :2338-2351), one more for "a row outside IUPAC".
// The row codes themselves (one byte per padded row: what the wave-per-read kernels read) are written on the way.
__device__ __forceinline__ void eq_words_body(const uint8_t* __restrict__ seq, const GaEqFill* __restrict__ fills, uint32_t nFills, const uint8_t* __restrict__ lut,
                                              uint32_t padCode, uint64_t* __restrict__ eq, uint8_t* __restrict__ flags, uint8_t* __restrict__ rows)
{
	__shared__ uint8_t t[512];
	const uint32_t lane = threadIdx.x;
	for (uint32_t i = lane; i < 512; i += 64) t[i] = lut[i];
	__syncthreads();
	for (uint32_t fi = blockIdx.x; fi < nFills; fi += gridDim.x)
	{
		const GaEqFill f = fills[fi];
		const uint8_t* s = seq + f.seq_off;
		bool bad = false;
		for (uint32_t r0 = 0; r0 < f.padded; r0 += 64)
		{
			const uint32_t k = r0 + lane;
			uint32_t code = padCode;
			if (k < f.n) code = f.backward ? t[256 + s[f.n - 1 - k]] : t[s[f.pos + k]];
			rows[f.eq_slice * 64 + k] = (uint8_t)code;
			const uint64_t e0 = __ballot(code & 1u), e1 = __ballot(code & 2u), e2 = __ballot(code & 4u), e3 = __ballot(code & 8u);
			const uint64_t inv = __ballot(code & GA_ROW_INVALID);
			const uint32_t last = (uint32_t)__builtin_amdgcn_readlane((int)code, 63);
			const uint64_t meta = (uint64_t)((last >> 4) & 7u) | (inv ? 8u : 0u);     // exact-compare code of the slice's last row | a row outside IUPAC
			if (lane < 5) eq[(f.eq_slice + r0 / 64) * 5 + lane] = lane == 0 ? e0 : lane == 1 ? e1 : lane == 2 ? e2 : lane == 3 ? e3 : meta;
			bad = bad || inv != 0;
		}
		if (lane == 0) flags[fi] = bad ? 1 : 0;
	}
}
__global__ void __launch_bounds__(64) ga_eq_words_kernel(const uint8_t* __restrict__ seq, const GaEqFill* __restrict__ fills, uint32_t nFills, const uint8_t* __restrict__ lut,
                                                         uint32_t padCode, uint64_t* __restrict__ eq, uint8_t* __restrict__ flags, uint8_t* __restrict__ rows)
{
	eq_words_body(seq, fills, nFills, lut, padCode, eq, flags, rows);
}
// the same over fills that the plan kernels left in device memory (ga_plan.h): their number is the plan's first total, read on the device
__global__ void __launch_bounds__(64) ga_eq_words_planned_kernel(const uint8_t* __restrict__ seq, const GaEqFill* __restrict__ fills, const uint64_t* __restrict__ totals,
                                                                 const uint8_t* __restrict__ lut, uint32_t padCode, uint64_t* __restrict__ eq, uint8_t* __restrict__ flags,
                                                                 uint8_t* __restrict__ rows)
{
	eq_words_body(seq, fills, (uint32_t)totals[0], lut, padCode, eq, flags, rows);
}

// ---- the job plan of a seeded batch (ga_plan.h): three launches around two scans -------------------------------------------------
// one wave per read at a time: first_bad[read]
__global__ void __launch_bounds__(64) ga_plan_first_bad_kernel(gap::PlanLaunch L, const uint8_t* __restrict__ hasComplement)
{
	__shared__ uint8_t t[256];
	const uint32_t lane = threadIdx.x;
	for (uint32_t i = lane; i < 256; i += 64) t[i] = hasComplement[i];
	__syncthreads();
	for (uint32_t r = blockIdx.x; r < L.n_reads; r += gridDim.x)
	{
		uint32_t bad = gap::first_bad_lane(L, t, r, lane);
		for (int d = 32; d >= 1; d >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)bad, d, 64); bad = o < bad ? o : bad; }
		if (lane == 0) L.first_bad[r] = bad;
	}
}
// one lane per seed slot, and one more for the scans' last element
__global__ void __launch_bounds__(256) ga_plan_slot_kernel(gap::PlanLaunch L)
{
	const uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x;
	if (s <= (uint64_t)L.n_reads * L.max_seeds) gap::plan_slot(L, (uint32_t)s);
}
__global__ void __launch_bounds__(256) ga_plan_write_kernel(gap::PlanLaunch L)
{
	const uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x, nSlots = (uint64_t)L.n_reads * L.max_seeds;
	if (s < nSlots) gap::plan_write(L, (uint32_t)s);
	else if (s == nSlots) gap::plan_tail(L);
}

// ---- per-base operations as runs (ga_ops.h): one wave per job at a time, the same program counting and writing ------------------
__global__ void __launch_bounds__(64) ga_ops_count_kernel(gao::OpsLaunch L)
{
	__shared__ gao::OpsLds lds;
	gao::run_wave<false>(L, lds, blockIdx.x, gridDim.x);
}
__global__ void __launch_bounds__(64) ga_ops_write_kernel(gao::OpsLaunch L)
{
	__shared__ gao::OpsLds lds;
	gao::run_wave<true>(L, lds, blockIdx.x, gridDim.x);
}

// ---- pileups (ga_pileup.h): the walk of the operations program with an atomic add per item; the items of the host's list ----------
__global__ void __launch_bounds__(64) ga_pileup_bases_kernel(gapl::PileupLaunch P)
{
	__shared__ gapl::PileupLds lds;
	gapl::run_wave<gapl::KIND_BASES>(P, lds, blockIdx.x, gridDim.x);
}
__global__ void __launch_bounds__(64) ga_pileup_depth_kernel(gapl::PileupLaunch P)
{
	__shared__ gapl::PileupLds lds;
	gapl::run_wave<gapl::KIND_DEPTH>(P, lds, blockIdx.x, gridDim.x);
}
__global__ void __launch_bounds__(256) ga_pileup_pairs_kernel(const uint64_t* pairs, uint64_t n, uint32_t* planes, uint64_t columns, uint32_t kind)
{
	const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
	if (i < n) gapl::add_pair(pairs, i, planes, columns, kind);
}

// ---- edge support (ga_edges.h): the same walk with one atomic add per counted node crossing; the crossings of the host's list ----------
__global__ void __launch_bounds__(64) ga_pileup_edges_kernel(gaed::EdgesLaunch P)
{
	__shared__ gao::OpsLds lds;
	gaed::run_wave(P, lds, blockIdx.x, gridDim.x);
}
__global__ void __launch_bounds__(256) ga_pileup_slots_kernel(const uint32_t* slots, uint64_t n, uint32_t* counts, uint64_t entries)
{
	const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
	if (i < n) gaed::add_slot(slots, i, counts, entries);
}

// ---- site queries (ga_sites.h): one streaming pass over a pileup's planes marks the sites, a scan places them, a second pass writes them ----
__global__ void __launch_bounds__(64) ga_pileup_sites_mark_kernel(gast::SitesLaunch L)
{
	__shared__ gast::SitesLds lds;
	gast::mark_wave(L, lds, blockIdx.x, gridDim.x);
}
__global__ void __launch_bounds__(64) ga_pileup_sites_write_kernel(gast::SitesLaunch L)
{
	gast::write_wave(L, blockIdx.x, gridDim.x);
}

// every job's output record starts a run as "not run" (what a job keeps when no pass ever picks it up)
__global__ void ga_outs_init_kernel(GaJobOut* outs, uint32_t n)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	GaJobOut o;
	memset(&o, 0, sizeof(o));
	o.status = GA_NOT_RUN;
	outs[i] = o;
}

// pinned host blocks for the batches' copies of the reads (page-locking half a GB per batch costs more than copying it): a block goes
// back to the pool when the last holder -- the batch, or results whose edit sequences point into it -- lets go of it
struct PinnedPool
{
	std::mutex lock;
	std::vector<std::pair<size_t, char*>> idle;
	~PinnedPool() { for (auto& b : idle) hipHostFree(b.second); }
};

// the counters of one pileup: `nPlanes` planes of one 32-bit word per entry (ga_backend.h: a column, or a slot for the EDGES kind), in the
// HBM of the graph's device; the EDGES kind keeps its mirror-slot table next to them
struct DevGraph;
struct DevPileup : GaBackendPileup
{
	DevGraph* g = nullptr;             // (a pileup is freed before its graph)
	int device = 0;
	uint32_t kind = 0, nPlanes = 0;
	uint64_t entries = 0;
	uint32_t* planes = nullptr;
	uint32_t* mirror = nullptr;
	~DevPileup() override { hipSetDevice(device); if (planes) hipFree(planes); if (mirror) hipFree(mirror); }
	size_t bytes() const { return (size_t)nPlanes * entries * 4; }
	int reset() override
	{
		// (the caller lets no add into this pileup run at the same time -- ga_pileup_reset holds the pileup exclusively -- and an add has
		// finished when addToPileup returns: the null stream alone is waited for, not the device with every other batch's kernels)
		HIP_OK(hipSetDevice(device));
		HIP_OK(hipMemsetAsync(planes, 0, bytes(), nullptr));
		HIP_OK(hipStreamSynchronize(nullptr));
		return 0;
	}
	int download(uint64_t first, uint64_t n, uint32_t* out) const override
	{
		if (first > entries || n > entries - first) return GA_E_INVALID;
		HIP_OK(hipSetDevice(device));
		// (an add has finished on its batch's stream when addToPileup returns: nothing to wait for)
		for (uint32_t k = 0; k < nPlanes && n; k++) HIP_OK(hipMemcpy(out + (size_t)k * n, planes + (size_t)k * entries + first, n * 4, hipMemcpyDeviceToHost));
		return 0;
	}
	// (below DevGraph, whose block list, node table and stream it uses)
	int sites(const GaSiteQuery& q, GaSitesOut& out) override;
	struct SiteBlocks { std::vector<std::pair<size_t, void*>> taken; };
	int sitesWith(const GaSiteQuery& q, GaSitesOut& out, SiteBlocks& blocks);
};

struct DevGraph : GaBackendGraph
{
	std::shared_ptr<PinnedPool> pinned = std::make_shared<PinnedPool>();
	bool buildsMatchWords() const override { return true; }
	bool codesOps() const override { return true; }
	bool codesPileup() const override { return true; }
	GaBackendPileup* createPileup(const GaPileupSpec& spec, int* status) override
	{
		*status = GA_E_INVALID;
		const bool edges = spec.kind == GA_KIND_EDGES;
		if (spec.planes == 0 || spec.planes != ga_pileup_planes_of_kind(spec.kind) || spec.entries != ga_pileup_entries(spec.kind, totalBp, edgeSlots)) return nullptr;
		if (edges && (!spec.mirrorSlot || spec.entries >= 0xffffffffull)) return nullptr;
		*status = GA_E_DEVICE;
		if (hipSetDevice(device) != hipSuccess) return nullptr;
		std::unique_ptr<DevPileup> p(new DevPileup());
		p->g = this; p->device = device; p->kind = (uint32_t)spec.kind; p->nPlanes = spec.planes; p->entries = spec.entries;
		if (hipMalloc((void**)&p->planes, std::max<size_t>(p->bytes(), 16)) != hipSuccess) { p->planes = nullptr; (void)hipGetLastError(); return nullptr; }
		if (edges)
		{
			if (hipMalloc((void**)&p->mirror, std::max<size_t>((size_t)p->entries * 4, 16)) != hipSuccess) { p->mirror = nullptr; (void)hipGetLastError(); return nullptr; }
			if (p->entries && hipMemcpy(p->mirror, spec.mirrorSlot, (size_t)p->entries * 4, hipMemcpyHostToDevice) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
		}
		if (p->reset() != 0) return nullptr;
		*status = 0;
		return p.release();
	}
	std::shared_ptr<char> hostBlock(size_t bytes) override
	{
		const size_t two = (size_t)2 << 20;
		bytes = (bytes + two - 1) & ~(two - 1);
		std::shared_ptr<PinnedPool> pool = pinned;
		char* p = nullptr;
		size_t cap = 0;
		{
			std::lock_guard<std::mutex> guard(pool->lock);
			size_t best = pool->idle.size();
			for (size_t i = 0; i < pool->idle.size(); i++)
				if (pool->idle[i].first >= bytes && pool->idle[i].first <= 2 * bytes + two && (best == pool->idle.size() || pool->idle[i].first < pool->idle[best].first)) best = i;
			if (best != pool->idle.size()) { cap = pool->idle[best].first; p = pool->idle[best].second; pool->idle.erase(pool->idle.begin() + (long)best); }
		}
		if (!p)
		{
			hipSetDevice(device);
			if (hipHostMalloc((void**)&p, bytes, hipHostMallocDefault) != hipSuccess) return GaBackendGraph::hostBlock(bytes);      // (pageable memory: the upload is then a staged copy)
			cap = bytes;
		}
		return std::shared_ptr<char>(p, [pool, cap](char* q) {
			std::lock_guard<std::mutex> guard(pool->lock);
			if (pool->idle.size() < 6) pool->idle.emplace_back(cap, q); else hipHostFree(q);
		});
	}

	// seeding (ga_seed.h): the k-mer index of this graph and its buffers, built on request
	std::unique_ptr<gasd::DevSeedEngine> seed;
	GaSeedEngine* seedEngine() override { return seed.get(); }

	// seeded batches (ga_plan.h): twin[n] and digraph id & 1 per node, uploaded at the first seeded prepare, freed with the graph
	std::mutex twinLock;
	uint32_t* dTwin = nullptr;
	uint8_t* dRev = nullptr;
	uint32_t* dOpsTwin = nullptr;      // the twin table alone, for GA_F_OPS batches of ga_batch_prepare (uploaded at the first of them)
	// site queries (ga_sites.h): the per-node fold table, uploaded at the first fold query over a columns kind, freed with the graph; the
	// stream and the two events the queries run on (one query at a time: sitesLock)
	std::mutex sitesLock;
	uint32_t* dFold = nullptr;
	hipStream_t sitesStream = nullptr;
	hipEvent_t evS[2] = {nullptr, nullptr};
	GaBackendBatch* beginSeededBatch(const GaSeededRequest& req, GaSeededPlan& plan, int* status) override;

	int device = 0;
	GaDevGraph g;
	GaHmmTables* hmm = nullptr;
	std::vector<void*> allocs;
	int cus = 0;
	uint64_t totalBp = 0;
	uint64_t edgeSlots = 0;            // the in-neighbour lists' total length: the entries of a pileup of the EDGES kind
	// scratch pool owned by the graph: batches reuse it instead of allocating tens of GB each
	uint8_t* pool = nullptr;
	size_t poolBytes = 0;
	bool poolBusy = false;
	~DevGraph() override
	{
		hipSetDevice(device);
		for (void* p : allocs) hipFree(p);
		for (auto& b : idleBlocks) hipFree(b.second);
		if (pool) hipFree(pool);
		if (hostPool) hipHostFree(hostPool);
		for (hipEvent_t e : evS) if (e) hipEventDestroy(e);
		if (sitesStream) hipStreamDestroy(sitesStream);
	}
	// device buffers of the batches (match words, jobs, outputs, trace pool): handed back here instead of hipFree'd, because hipFree
	// waits for the whole device -- i.e. for the kernels of whatever batch is running -- and the stages of consecutive batches are
	// meant to overlap (sharding.run_overlapped).  A later batch of similar size takes them again.
	std::mutex blockLock;
	std::vector<std::pair<size_t, void*>> idleBlocks;
	void* takeBlock(size_t bytes)
	{
		{
			std::lock_guard<std::mutex> lock(blockLock);
			size_t best = idleBlocks.size();
			for (size_t i = 0; i < idleBlocks.size(); i++)
				if (idleBlocks[i].first >= bytes && idleBlocks[i].first <= bytes + bytes / 2 + 4096 && (best == idleBlocks.size() || idleBlocks[i].first < idleBlocks[best].first)) best = i;
			if (best != idleBlocks.size())
			{
				void* p = idleBlocks[best].second;
				idleBlocks.erase(idleBlocks.begin() + (long)best);
				return p;
			}
		}
		void* p = nullptr;
		if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
		return p;
	}
	void giveBlock(void* p, size_t bytes)
	{
		std::lock_guard<std::mutex> lock(blockLock);
		// (bounded: beyond a few dozen idle blocks the oldest go back to the device)
		if (idleBlocks.size() >= 48) { hipFree(idleBlocks.front().second); idleBlocks.erase(idleBlocks.begin()); }
		idleBlocks.emplace_back(bytes, p);
	}
	// (one graph can serve batches run from several host threads: the pool changes hands under a lock)
	std::mutex poolLock;
	uint8_t* takePool(size_t bytes)
	{
		std::lock_guard<std::mutex> lock(poolLock);
		if (poolBusy) return nullptr;
		if (bytes > poolBytes)
		{
			if (pool) hipFree(pool);
			pool = nullptr; poolBytes = 0;
			if (hipMalloc((void**)&pool, bytes) != hipSuccess) { pool = nullptr; return nullptr; }
			poolBytes = bytes;
		}
		poolBusy = true;
		return pool;
	}
	void givePool() { std::lock_guard<std::mutex> lock(poolLock); poolBusy = false; }
	size_t poolBytesIfFree() { std::lock_guard<std::mutex> lock(poolLock); return poolBusy ? 0 : poolBytes; }
	// pinned host buffer for the moves on their way back (page-locking half a GB per batch would cost more than the copy)
	std::mutex hostLock;
	uint8_t* hostPool = nullptr;
	size_t hostPoolBytes = 0;
	bool hostPoolBusy = false;
	uint8_t* takeHost(size_t bytes)
	{
		std::lock_guard<std::mutex> lock(hostLock);
		if (hostPoolBusy) return nullptr;
		if (bytes > hostPoolBytes)
		{
			if (hostPool) hipHostFree(hostPool);
			hostPool = nullptr; hostPoolBytes = 0;
			const size_t want = bytes + bytes / 8;
			if (hipHostMalloc((void**)&hostPool, want, hipHostMallocDefault) != hipSuccess) { hostPool = nullptr; return nullptr; }
			hostPoolBytes = want;
		}
		hostPoolBusy = true;
		return hostPool;
	}
	void giveHost() { std::lock_guard<std::mutex> lock(hostLock); hostPoolBusy = false; }
	template <typename T> int put(const std::vector<T>& v, const T** out)
	{
		void* p = nullptr;
		HIP_OK(hipMalloc(&p, std::max<size_t>(v.size() * sizeof(T), 16)));
		allocs.push_back(p);
		HIP_OK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
		*out = (const T*)p;
		return 0;
	}
};

// ---- site queries (ga_sites.h) -----------------------------------------------------------------------------------------------------
int DevPileup::sites(const GaSiteQuery& q, GaSitesOut& out)
{
	out = GaSitesOut();
	const bool edges = kind == (uint32_t)GA_KIND_EDGES, foldNodes = q.fold && !edges;
	if (!g || q.first > entries || q.n > entries - q.first || q.alt_den == 0) return GA_E_INVALID;
	if (foldNodes && (!q.foldTable || q.nNodes != g->g.n_nodes)) return GA_E_INVALID;
	if (q.fold && edges && !mirror) return GA_E_INVALID;
	if (q.n == 0) return 0;
	std::lock_guard<std::mutex> one(g->sitesLock);
	HIP_OK(hipSetDevice(device));
	if (!g->sitesStream) HIP_OK(hipStreamCreateWithFlags(&g->sitesStream, hipStreamNonBlocking));
	for (hipEvent_t& e : g->evS) if (!e) HIP_OK(hipEventCreate(&e));
	if (foldNodes && !g->dFold)
	{
		void* t = nullptr;
		HIP_OK(hipMalloc(&t, std::max<size_t>(q.nNodes * 4, 16)));
		g->allocs.push_back(t);
		HIP_OK(hipMemcpy(t, q.foldTable, q.nNodes * 4, hipMemcpyHostToDevice));
		g->dFold = (uint32_t*)t;
	}
	SiteBlocks blocks;
	const int rc = sitesWith(q, out, blocks);
	// the blocks go back to the graph's list whether or not the query went through (after an error, once the stream is idle)
	if (rc) (void)hipStreamSynchronize(g->sitesStream);
	for (auto& b : blocks.taken) g->giveBlock(b.second, b.first);
	return rc;
}

int DevPileup::sitesWith(const GaSiteQuery& q, GaSitesOut& out, SiteBlocks& blocks)
{
	hipStream_t stream = g->sitesStream;
	auto take = [&](size_t bytes) -> void* {
		bytes = std::max<size_t>((bytes + 255) & ~(size_t)255, 256);
		void* p = g->takeBlock(bytes);
		if (p) blocks.taken.emplace_back(bytes, p);
		return p;
	};
	gast::SitesLaunch L;
	memset(&L, 0, sizeof(L));
	L.planes = planes; L.entries = entries; L.kind = kind; L.nPlanes = nPlanes;
	L.fold = q.fold ? 1u : 0u; L.n_nodes = g->g.n_nodes;
	L.node_start = g->g.node_start; L.fold_table = g->dFold; L.mirror = mirror;
	L.first = q.first; L.n = q.n;
	L.min_depth = q.min_depth; L.min_alt = q.min_alt; L.alt_num = q.alt_num; L.alt_den = q.alt_den;
	L.n_tiles = (q.n + gast::kTile - 1) / gast::kTile;
	const size_t nT = (size_t)L.n_tiles;
	uint64_t* dCounts = (uint64_t*)take((nT + 1) * 8);
	uint64_t* dOffsets = (uint64_t*)take((nT + 1) * 8);
	L.mask = (uint64_t*)take(nT * gast::kRounds * 8);
	if (!dCounts || !dOffsets || !L.mask) return GA_E_DEVICE;
	L.counts = dCounts; L.offsets = dOffsets;
	size_t tmpBytes = 0;
	HIP_OK(rocprim::exclusive_scan(nullptr, tmpBytes, dCounts, dOffsets, (uint64_t)0, nT + 1, rocprim::plus<uint64_t>(), stream));
	void* dTmp = take(tmpBytes + 16);
	if (!dTmp) return GA_E_DEVICE;
	HIP_OK(hipMemsetAsync(dCounts + nT, 0, 8, stream));
	// enough waves to keep the memory system busy: a wave has 8 (fold: 16) loads of 256 bytes in flight
	const uint32_t waves = (uint32_t)std::min<uint64_t>(L.n_tiles, (uint64_t)std::max(g->cus, 1) * 32);
	HIP_OK(hipEventRecord(g->evS[0], stream));
	hipLaunchKernelGGL(ga_pileup_sites_mark_kernel, dim3(waves), dim3(64), 0, stream, L);
	HIP_OK(hipGetLastError());
	HIP_OK(rocprim::exclusive_scan(dTmp, tmpBytes, dCounts, dOffsets, (uint64_t)0, nT + 1, rocprim::plus<uint64_t>(), stream));
	uint64_t total = 0;
	HIP_OK(hipMemcpyAsync(&total, dOffsets + nT, 8, hipMemcpyDeviceToHost, stream));
	HIP_OK(hipStreamSynchronize(stream));
	if (total > q.n) return GA_E_DEVICE;
	const uint64_t nRecs = q.max_sites ? std::min(total, q.max_sites) : total;
	if (nRecs)
	{
		L.recs = (GaSiteRec*)take((size_t)nRecs * sizeof(GaSiteRec));
		if (!L.recs) return GA_E_DEVICE;
		L.n_recs = nRecs;
		hipLaunchKernelGGL(ga_pileup_sites_write_kernel, dim3(waves), dim3(64), 0, stream, L);
		HIP_OK(hipGetLastError());
	}
	HIP_OK(hipEventRecord(g->evS[1], stream));
	out.recs.resize((size_t)nRecs);
	if (nRecs) HIP_OK(hipMemcpyAsync(out.recs.data(), L.recs, (size_t)nRecs * sizeof(GaSiteRec), hipMemcpyDeviceToHost, stream));
	HIP_OK(hipStreamSynchronize(stream));
	float ms = 0;
	HIP_OK(hipEventElapsedTime(&ms, g->evS[0], g->evS[1]));
	out.n_total = total; out.kernel_ms = ms;
	return 0;
}

// the few switches the library reads from the environment, once per batch: GA_LANES (1 / 0: force which kernel goes first -- the GPU
// parity tests run every case both ways), GA_DEBUG_PASSES (one line per launch on stderr) and two test hooks: the trace pool's size
// and a cap on the waves a launch starts
struct Knobs
{
	int lanes = -1;                 // -1: by graph shape
	int spread = 1;                 // 1: a small batch is spread over all wave slots; 0: full waves; k > 1: k jobs per wave (GA_LANES_SPREAD, for experiments)
	bool debugPasses = false;
	uint64_t tracePoolBytes = 0;    // 0: sized from the batch
	uint32_t waveSlots = 0;         // 0: as many waves as fit; k: no launch starts more than k (GA_TEST_WAVE_SLOTS: a wave then takes group after group / job after job)
	Knobs()
	{
		if (const char* e = getenv("GA_LANES")) lanes = atoi(e) != 0 ? 1 : 0;
		debugPasses = getenv("GA_DEBUG_PASSES") != nullptr;
		if (const char* e = getenv("GA_LANES_SPREAD")) spread = atoi(e);
		if (const char* t = getenv("GA_TEST_TRACE_POOL_BYTES")) tracePoolBytes = (uint64_t)atoll(t) & ~3ull;
		if (const char* e = getenv("GA_TEST_WAVE_SLOTS")) waveSlots = (uint32_t)std::max(atoi(e), 0);
	}
};

struct DevBatch : GaBackendBatch
{
	DevGraph* g = nullptr;
	Knobs knobs;
	hipStream_t stream = nullptr;
	hipEvent_t evA = nullptr, evB = nullptr;
	std::vector<std::pair<size_t, void*>> allocs;     // (bytes, block) from the graph's block list
	std::vector<GaJob> jobs;
	GaRunConfig cfg;
	GaLaunch L;                 // what every pass shares (graph, reads, jobs, outputs, trace pool); scratch geometry is set per pass
	const uint64_t* dEq = nullptr;
	uint32_t* dList = nullptr;  // job list of the current pass
	size_t dListCap = 0;
	std::vector<GaJobOut> outs;
	bool outsLocked = false;
	std::vector<uint32_t> orderHost;   // all jobs, longest first (the device queues hand them out in this order)
	std::vector<uint8_t> passOf;       // which pass of the last run finished each job (0 = the first)
	int passNo = 0;
	GaRunStats st;
	GaRowsProvider rowsProvider;       // row codes for the wave-per-read kernels, uploaded when the first of them is about to run
	uint8_t* privateScratch = nullptr; // only when the graph's pool is taken by another batch
	size_t privateBytes = 0;

	~DevBatch() override
	{
		hipSetDevice(g->device);
		if (hostFromPool) g->giveHost();
		if (outsLocked) hipHostUnregister(outs.data());
		for (auto& a : allocs) g->giveBlock(a.second, a.first);
		if (privateScratch) hipFree(privateScratch);
		if (evA) hipEventDestroy(evA);
		if (evB) hipEventDestroy(evB);
		for (hipEvent_t e : evP) if (e) hipEventDestroy(e);
		for (hipEvent_t e : evO) if (e) hipEventDestroy(e);
		for (hipEvent_t e : evU) if (e) hipEventDestroy(e);
		if (stream) hipStreamDestroy(stream);
	}
	// a block of alloc() that the batch no longer needs, handed back before the batch ends
	void release(void* p)
	{
		for (size_t i = 0; i < allocs.size(); i++)
			if (allocs[i].second == p) { g->giveBlock(p, allocs[i].first); allocs.erase(allocs.begin() + (long)i); return; }
	}
	template <typename T> int alloc(T** out, size_t count)
	{
		const size_t bytes = (std::max<size_t>(count * sizeof(T), 16) + 255) & ~(size_t)255;
		void* p = g->takeBlock(bytes);
		if (!p) { fprintf(stderr, "graphaligner_amd: no device memory for %zu bytes\n", bytes); return GA_E_DEVICE; }
		allocs.emplace_back(bytes, p);
		*out = (T*)p;
		return 0;
	}

	int ensureRows()
	{
		if (L.rows) return 0;
		if (builtRows) { L.rows = builtRows; return 0; }                          // (written by the match-word kernel)
		const std::vector<uint8_t>& rows = rowsProvider();
		uint8_t* dRows;
		if (alloc(&dRows, rows.size())) return GA_E_DEVICE;
		HIP_OK(hipMemcpyAsync(dRows, rows.data(), rows.size(), hipMemcpyHostToDevice, stream));
		L.rows = dRows;
		return 0;
	}

	uint8_t* builtRows = nullptr;      // the row codes, when the match-word kernel wrote them
	std::vector<uint8_t> badFills;     // per fill of the GaEqSource: a row outside IUPAC
	const std::vector<uint8_t>* invalidFills() const override { return &badFills; }
	bool emittingRuns() const override { return cfg.emit_runs != 0; }

	// the stream and the events, before anything else
	int open()
	{
		HIP_OK(hipSetDevice(g->device));
		// (non-blocking: a copy or a kernel of this batch must not wait for another batch's kernel through the null stream)
		HIP_OK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
		HIP_OK(hipEventCreate(&evA));
		HIP_OK(hipEventCreate(&evB));
		memset(&L, 0, sizeof(L));
		L.graph = g->g;
		L.hmm = g->hmm;
		return 0;
	}
	// what every pass shares of the jobs and the configuration
	void setJobs(const std::vector<GaJob>& jobsIn)
	{
		jobs = jobsIn;
		L.n_jobs = (uint32_t)jobs.size();
		L.initial_bw = cfg.initial_bw;
		L.ramp_bw = cfg.ramp_bw;
		L.max_slices = std::max<uint32_t>(cfg.max_slices, 1);
	}

	int init(const uint64_t* eq, const GaEqSource* src, size_t eqWords, const std::vector<GaJob>& jobsIn)
	{
		if (int s = open()) return s;
		setJobs(jobsIn);
		GaJob* dJobs; uint64_t* eqDev;
		if (alloc(&eqDev, eqWords)) return GA_E_DEVICE;
		if (alloc(&dJobs, jobs.size())) return GA_E_DEVICE;
		if (!src && !eq) return GA_E_INVALID;
		if (src)
		{
			// the reads go up as they are (one transfer from the batch's pinned copy) and a kernel turns them into the match words
			uint8_t *dSeq, *dLut, *dFlags, *dRows; GaEqFill* dFills;
			const size_t rowBytes = (eqWords / 5) * 64 + 64;                         // (+ slack so a 64-byte row load never leaves the buffer)
			if (alloc(&dSeq, src->seqBytes + 64) || alloc(&dFills, src->nFills) || alloc(&dLut, 512) || alloc(&dFlags, src->nFills) || alloc(&dRows, rowBytes)) return GA_E_DEVICE;
			HIP_OK(hipMemsetAsync(dRows + rowBytes - 128, 0, 128, stream));
			builtRows = dRows;
			resSeq = dSeq; resSeqBytes = src->seqBytes; resFills = dFills;
			if ((cfg.emit_ops || cfg.emit_pileup) && src->twin)
			{
				std::lock_guard<std::mutex> guard(g->twinLock);
				if (!g->dTwin && !g->dOpsTwin)
				{
					void* tw = nullptr;
					HIP_OK(hipMalloc(&tw, (size_t)g->g.n_nodes * 4));
					g->allocs.push_back(tw);
					HIP_OK(hipMemcpyAsync(tw, src->twin, (size_t)g->g.n_nodes * 4, hipMemcpyHostToDevice, stream));
					HIP_OK(hipStreamSynchronize(stream));
					g->dOpsTwin = (uint32_t*)tw;
				}
			}
			memcpy(opsLut, src->rowCode, 256);
			uint8_t lut[512];
			memcpy(lut, src->rowCode, 256); memcpy(lut + 256, src->rowCodeRc, 256);
			HIP_OK(hipMemcpyAsync(dSeq, src->seq, src->seqBytes, hipMemcpyHostToDevice, stream));
			HIP_OK(hipMemcpyAsync(dFills, src->fills, src->nFills * sizeof(GaEqFill), hipMemcpyHostToDevice, stream));
			HIP_OK(hipMemcpyAsync(dLut, lut, 512, hipMemcpyHostToDevice, stream));
			HIP_OK(hipMemsetAsync(eqDev + (eqWords - 5), 0, 40, stream));             // (the slack slice behind the last job)
			badFills.assign(src->nFills, 0);
			if (src->nFills)
			{
				const uint32_t blocks = (uint32_t)std::min<size_t>(src->nFills, (size_t)g->cus * 64);
				hipLaunchKernelGGL(ga_eq_words_kernel, dim3(blocks), dim3(64), 0, stream, dSeq, dFills, (uint32_t)src->nFills, dLut, (uint32_t)src->padCode, eqDev, dFlags, dRows);
				HIP_OK(hipGetLastError());
				HIP_OK(hipMemcpyAsync(badFills.data(), dFlags, src->nFills, hipMemcpyDeviceToHost, stream));
			}
			HIP_OK(hipStreamSynchronize(stream));                                      // (lut is on this stack; the flags decide emit_runs below)
			for (uint8_t f : badFills) if (f) { cfg.emit_runs = 0; break; }
		}
		else HIP_OK(hipMemcpyAsync(eqDev, eq, eqWords * 8, hipMemcpyHostToDevice, stream));
		HIP_OK(hipMemcpyAsync(dJobs, jobs.data(), jobs.size() * sizeof(GaJob), hipMemcpyHostToDevice, stream));
		L.rows = nullptr;
		L.jobs = dJobs;
		dEq = eqDev;
		return finish();
	}

	// the hand-out order, the output records and the trace pool, from the host's copy of the jobs
	int finish()
	{
		// the device queues hand jobs out longest first: the short ones fill the tail of a launch, and the 64 jobs a lanes = reads
		// wave carries together have similar lengths
		orderHost.resize(jobs.size());
		for (uint32_t i = 0; i < jobs.size(); i++) orderHost[i] = i;
		std::stable_sort(orderHost.begin(), orderHost.end(), [&](uint32_t a, uint32_t b) { return jobs[a].n_rows > jobs[b].n_rows; });
		dListCap = std::max<size_t>(jobs.size(), 1);
		if (alloc(&dList, dListCap)) return GA_E_DEVICE;
		if (alloc(&L.outs, jobs.size())) return GA_E_DEVICE;
		// (the host copy of the records is page-locked: they come back after every pass, 128 bytes per job)
		outs.assign(jobs.size(), GaJobOut{});
		for (auto& o : outs) o.status = GA_NOT_RUN;
		outsLocked = !outs.empty() && hipHostRegister(outs.data(), outs.size() * sizeof(GaJobOut), hipHostRegisterDefault) == hipSuccess;
		if (alloc(&L.next_job, 4)) return GA_E_DEVICE;
		if (alloc(&L.trace_top, 2)) return GA_E_DEVICE;
		uint64_t totalRows = 0;
		for (auto& j : jobs) totalRows += j.n_rows;
		// one byte per move (a path makes at most ~1.5 moves per row), or 20 bytes per node run: room for a node change every 5 rows
		// (a job that does not fit reports GA_CAP_TRACE and is rerun by the ladder, which writes moves)
		L.trace_pool_cap = ((totalRows * (cfg.emit_runs ? 4 : 1) + totalRows / 2 + 256ull * jobs.size() + 4096) + 3) & ~3ull;
		// (test hook: a deliberately small pool, so that the claims' overflow path runs -- tests/parity_cases.py)
		if (knobs.tracePoolBytes) L.trace_pool_cap = knobs.tracePoolBytes;
		if (alloc(&L.traces, L.trace_pool_cap)) return GA_E_DEVICE;
		HIP_OK(hipStreamSynchronize(stream));
		return 0;
	}

	// ---- seeded batch (ga_plan.h): everything from the one upload of the reads to the one download of seeds and plan ----------------
	uint8_t planLut[768];              // row codes, row codes of the complement, "has a complement": lives as long as its upload may run
	hipEvent_t evP[4] = {nullptr, nullptr, nullptr, nullptr};
	int beginSeeded(const GaSeededRequest& req, GaSeededPlan& plan)
	{
		if (int s = open()) return s;
		gasd::DevSeedEngine* eng = g->seed.get();
		if (!eng || !eng->built()) return GA_E_INVALID;
		const size_t nReads = req.nReads, nSlots = nReads * req.p.max_seeds, nJobsCap = 2 * nSlots;
		if (nSlots >= ((size_t)1 << 30)) return GA_E_INVALID;                  // (slot and job numbers are 32-bit)
		for (hipEvent_t& e : evP) HIP_OK(hipEventCreate(&e));
		auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
		// what comes back in the one download
		const size_t oOutN = 0, oOutSeed = oOutN + up(nReads * 12), oOutLocus = oOutSeed + up(nSlots * 12), oOutNLoci = oOutLocus + (req.byLocus ? up(nSlots * 12) : 0);
		const size_t oTotals = oOutNLoci + (req.byLocus ? up(nReads * 4) : 0), oSeeds = oTotals + 256, oJobs = oSeeds + up(nSlots * sizeof(GaPlanSeed));
		const size_t oFills = oJobs + up(nJobsCap * sizeof(GaJob)), oFillRead = oFills + up(nJobsCap * sizeof(GaEqFill)), oFlags = oFillRead + up(nJobsCap * 4);
		const size_t downBytes = oFlags + up(nJobsCap);
		// what stays: the reads' block, and the plan's work arrays
		const size_t oFirstBad = 0, oNBw = oFirstBad + up(nReads * 4), oNFw = oNBw + up((nSlots + 1) * 4), oSlotJobs = oNFw + up((nSlots + 1) * 4);
		const size_t oJobAt = oSlotJobs + up((nSlots + 1) * 4), oSlotRows = oJobAt + up((nSlots + 1) * 4), oRowsAt = oSlotRows + up((nSlots + 1) * 8);
		const size_t workBytes = oRowsAt + up((nSlots + 1) * 8);
		const size_t eqWords = (size_t)(req.rowsBound / 64 + 1) * 5, rowBytes = (size_t)req.rowsBound + 128;
		uint8_t *dIn, *dDown, *dWork, *dLut, *dRows; uint64_t* eqDev;
		if (alloc(&dIn, req.blockBytes + 64) || alloc(&dDown, downBytes) || alloc(&dWork, workBytes) || alloc(&dLut, 768) || alloc(&dRows, rowBytes) || alloc(&eqDev, eqWords)) return GA_E_DEVICE;
		{
			std::lock_guard<std::mutex> guard(g->twinLock);
			if (!g->dTwin)
			{
				void* tw = nullptr; void* rv = nullptr;
				HIP_OK(hipMalloc(&tw, (size_t)g->g.n_nodes * 4));
				g->allocs.push_back(tw);
				HIP_OK(hipMalloc(&rv, (size_t)g->g.n_nodes));
				g->allocs.push_back(rv);
				HIP_OK(hipMemcpyAsync(tw, req.twin, (size_t)g->g.n_nodes * 4, hipMemcpyHostToDevice, stream));
				HIP_OK(hipMemcpyAsync(rv, req.rev, (size_t)g->g.n_nodes, hipMemcpyHostToDevice, stream));
				HIP_OK(hipStreamSynchronize(stream));
				g->dRev = (uint8_t*)rv;
				g->dTwin = (uint32_t*)tw;
			}
		}
		memcpy(planLut, req.rowCode, 256); memcpy(planLut + 256, req.rowCodeRc, 256); memcpy(planLut + 512, req.hasComplement, 256);
		// the one upload: reads, read records, hand-out order
		HIP_OK(hipMemcpyAsync(dIn, req.block, req.blockBytes, hipMemcpyHostToDevice, stream));
		HIP_OK(hipMemcpyAsync(dLut, planLut, 768, hipMemcpyHostToDevice, stream));
		HIP_OK(hipMemsetAsync(dDown, 0, oTotals + 256, stream));                   // (the seeding kernel adds to cleared outputs)
		gap::PlanLaunch P;
		memset(&P, 0, sizeof(P));
		P.node_start = g->g.node_start; P.twin = g->dTwin; P.rev = g->dRev;
		P.n_nodes = g->g.n_nodes; P.n_reads = (uint32_t)nReads; P.max_seeds = req.p.max_seeds; P.overlap = req.overlap;
		P.seq = dIn; P.reads = (const gas::SeedRead*)(dIn + req.oRecs);
		P.out_n = (const uint32_t*)(dDown + oOutN); P.out_seed = (const uint32_t*)(dDown + oOutSeed);
		P.first_bad = (uint32_t*)(dWork + oFirstBad); P.n_bw = (uint32_t*)(dWork + oNBw); P.n_fw = (uint32_t*)(dWork + oNFw);
		P.slot_jobs = (uint32_t*)(dWork + oSlotJobs); P.job_at = (uint32_t*)(dWork + oJobAt); P.slot_rows = (uint64_t*)(dWork + oSlotRows); P.rows_at = (uint64_t*)(dWork + oRowsAt);
		P.seeds = (GaPlanSeed*)(dDown + oSeeds); P.jobs = (GaJob*)(dDown + oJobs); P.fills = (GaEqFill*)(dDown + oFills); P.fill_read = (uint32_t*)(dDown + oFillRead);
		P.totals = (uint64_t*)(dDown + oTotals); P.eq = eqDev; P.rows = dRows;
		size_t tmpA = 0, tmpB = 0;
		HIP_OK(rocprim::exclusive_scan(nullptr, tmpA, P.slot_jobs, P.job_at, 0u, nSlots + 1, rocprim::plus<uint32_t>(), stream));
		HIP_OK(rocprim::exclusive_scan(nullptr, tmpB, P.slot_rows, P.rows_at, (uint64_t)0, nSlots + 1, rocprim::plus<uint64_t>(), stream));
		uint8_t* dTmp;
		if (alloc(&dTmp, std::max(tmpA, tmpB) + 16)) return GA_E_DEVICE;
		plan.keep = g->hostBlock(downBytes);
		if (!plan.keep) return GA_E_DEVICE;
		{
			// the engine's hit and label buffers are per graph: its lock is held until this stream has finished the seeding kernel
			std::lock_guard<std::mutex> guard(eng->lock);
			auto queue = [&]() -> int {
			HIP_OK(hipEventRecord(evP[0], stream));
			if (nReads)
			{
				if (int s = eng->launchResident(req.p, nReads, req.byLocus, dIn, P.reads, (const uint32_t*)(dIn + req.oOrder), (uint32_t*)(dDown + oOutN), (uint32_t*)(dDown + oOutSeed),
				                                (uint32_t*)(dDown + oOutLocus), (uint32_t*)(dDown + oOutNLoci), stream)) return s;
			}
			HIP_OK(hipEventRecord(evP[1], stream));
			if (nReads)
			{
				const uint32_t waves = (uint32_t)std::min<size_t>(nReads, (size_t)g->cus * 32);
				hipLaunchKernelGGL(ga_plan_first_bad_kernel, dim3(waves), dim3(64), 0, stream, P, (const uint8_t*)(dLut + 512));
			}
			const uint32_t slotBlocks = (uint32_t)((nSlots + 1 + 255) / 256);
			hipLaunchKernelGGL(ga_plan_slot_kernel, dim3(slotBlocks), dim3(256), 0, stream, P);
			HIP_OK(rocprim::exclusive_scan(dTmp, tmpA, P.slot_jobs, P.job_at, 0u, nSlots + 1, rocprim::plus<uint32_t>(), stream));
			HIP_OK(rocprim::exclusive_scan(dTmp, tmpB, P.slot_rows, P.rows_at, (uint64_t)0, nSlots + 1, rocprim::plus<uint64_t>(), stream));
			hipLaunchKernelGGL(ga_plan_write_kernel, dim3(slotBlocks), dim3(256), 0, stream, P);
			HIP_OK(hipEventRecord(evP[2], stream));
			// the match words from the fills as they lie in device memory
			if (nSlots)
			{
				const uint32_t blocks = (uint32_t)std::min<size_t>(nJobsCap, (size_t)g->cus * 64);
				hipLaunchKernelGGL(ga_eq_words_planned_kernel, dim3(blocks), dim3(64), 0, stream, (const uint8_t*)dIn, (const GaEqFill*)P.fills, (const uint64_t*)P.totals, (const uint8_t*)dLut,
				                   (uint32_t)req.padCode, eqDev, dDown + oFlags, dRows);
			}
			HIP_OK(hipGetLastError());
			HIP_OK(hipEventRecord(evP[3], stream));
			// the one download
			HIP_OK(hipMemcpyAsync(plan.keep.get(), dDown, downBytes, hipMemcpyDeviceToHost, stream));
			HIP_OK(hipEventSynchronize(evP[1]));
			return 0;
			};
			// (a failure after the first launch: nothing of this batch may still run when the lock goes and the caller frees the batch,
			// whose blocks and the graph's hit buffers the next prepare takes)
			if (int s = queue()) { hipStreamSynchronize(stream); return s; }
		}
		HIP_OK(hipStreamSynchronize(stream));
		// (the scans' arrays, their temporary storage and the tables serve the prepare only: back to the graph's block list now)
		release(dWork); release(dTmp); release(dLut);
		float ms[3] = {0, 0, 0};
		for (int k = 0; k < 3; k++) HIP_OK(hipEventElapsedTime(&ms[k], evP[k], evP[k + 1]));
		for (hipEvent_t& e : evP) { hipEventDestroy(e); e = nullptr; }
		const char* h = plan.keep.get();
		plan.outN = (const uint32_t*)(h + oOutN); plan.outSeed = (const uint32_t*)(h + oOutSeed);
		if (req.byLocus) { plan.outLocus = (const uint32_t*)(h + oOutLocus); plan.outNLoci = (const uint32_t*)(h + oOutNLoci); }
		plan.seeds = (const GaPlanSeed*)(h + oSeeds); plan.jobs = (const GaJob*)(h + oJobs); plan.fills = (const GaEqFill*)(h + oFills);
		plan.fillRead = (const uint32_t*)(h + oFillRead); plan.badFills = (const uint8_t*)(h + oFlags);
		const uint64_t* totals = (const uint64_t*)(h + oTotals);
		plan.nJobs = (size_t)totals[0]; plan.rowsTotal = totals[1];
		plan.seed_ms = ms[0]; plan.plan_ms = ms[1]; plan.eq_ms = ms[2];
		if (plan.nJobs > nJobsCap || plan.rowsTotal > req.rowsBound) return GA_E_DEVICE;
		badFills.assign(plan.badFills, plan.badFills + plan.nJobs);
		resSeq = dIn; resSeqBytes = req.blockBytes; resFills = (const GaEqFill*)P.fills;
		memcpy(opsLut, req.rowCode, 256);
		builtRows = dRows;
		L.rows = nullptr;
		L.jobs = (const GaJob*)P.jobs;
		dEq = eqDev;
		return 0;
	}
	int finishSeeded(const std::vector<GaJob>& jobsIn, const GaRunConfig& c, GaRowsProvider rows, const uint64_t*, size_t) override
	{
		HIP_OK(hipSetDevice(g->device));
		cfg = c;
		rowsProvider = rows;
		setJobs(jobsIn);
		for (uint8_t f : badFills) if (f) { cfg.emit_runs = 0; break; }
		return finish();
	}

	// scratch for one pass: the graph's pool, or a private allocation while another batch holds the pool
	uint8_t* takeScratch(size_t bytes, bool& fromPool)
	{
		uint8_t* p = g->takePool(bytes);
		fromPool = p != nullptr;
		if (p) return p;
		if (bytes > privateBytes)
		{
			if (privateScratch) hipFree(privateScratch);
			privateScratch = nullptr; privateBytes = 0;
			if (hipMalloc((void**)&privateScratch, bytes) != hipSuccess) { privateScratch = nullptr; return nullptr; }
			privateBytes = bytes;
		}
		return privateScratch;
	}
	size_t scratchBudget() const
	{
		size_t freeB = 0, totalB = 0;
		if (hipMemGetInfo(&freeB, &totalB) != hipSuccess) return 0;
		const size_t poolFree = g->poolBytesIfFree();
		return (size_t)((freeB + (poolFree ? poolFree : privateBytes)) * 0.85);
	}
	int uploadList(const std::vector<uint32_t>& list)
	{
		HIP_OK(hipMemcpyAsync(dList, list.data(), list.size() * 4, hipMemcpyHostToDevice, stream));
		return 0;
	}
	int afterPass(float& ms)
	{
		HIP_OK(hipGetLastError());
		HIP_OK(hipEventRecord(evB, stream));
		HIP_OK(hipMemcpyAsync(outs.data(), L.outs, outs.size() * sizeof(GaJobOut), hipMemcpyDeviceToHost, stream));
		HIP_OK(hipStreamSynchronize(stream));
		HIP_OK(hipEventElapsedTime(&ms, evA, evB));
		st.kernel_ms += ms;
		return 0;
	}

	// ---- the ladder: ga_ladder.h decides which variant runs over which jobs, in which order; here is how each one is run ------------
	// lanes = reads variants <10,64>, <24,32>, <56,16>: arena rows per lane and slice -- the band's columns rounded up to blocks of 8 per
	// node, with room for the widest slices.  (10 / 24 / 56 band nodes per lane = 4 / 2 / 1 waves per CU next to the 12.8 KB block image.
	// The wider tables trade lanes for LDS per lane: 32 and 16 lanes per wave keep four waves on every CU -- the same number of reads in
	// flight as 64-lane waves that leave three SIMDs of four idle, in four times as many instruction streams.)
	static constexpr uint32_t kLanesRowsPerSlice[] = {288, 480, 768};

	// one launch of the lanes = reads kernel over `list` (job indices, longest first)
	template <int N, int LW> int lanesPass(const std::vector<uint32_t>& list, uint32_t rowsPerSlice, bool first)
	{
		gal::GaLanesLaunch P;
		memset(&P, 0, sizeof(P));
		P.graph = L.graph; P.hmm = L.hmm; P.eq = dEq; P.jobs = L.jobs; P.outs = L.outs;
		P.job_list = dList; P.n_jobs = (uint32_t)list.size();
		P.lanes_per_wave = LW;
		P.next_group = L.next_job;
		P.traces = L.traces; P.trace_top = L.trace_top; P.trace_pool_cap = L.trace_pool_cap;
		P.initial_bw = L.initial_bw; P.ramp_bw = L.ramp_bw;
		P.emit_runs = cfg.emit_runs;
		uint32_t maxRows = 0;
		for (uint32_t i : list) maxRows = std::max(maxRows, jobs[i].n_rows);
		P.max_slices = std::max<uint32_t>(maxRows / 64, 1);
		P.cap_cols = std::min<uint32_t>(N * 256u, 0xff00u);
		// (node runs are five words each: the staging plane holds a run per ten rows -- six times what a path over 64-bp nodes makes; a
		// job that needs more reports GA_CAP_TRACE and climbs on)
		P.cap_moves = maxRows * 2 + 1024;
		const uint32_t ldsBytes = gal::Lay<N>::WORDS * LW * 4 + LW * gal::kStageWords64 * 8 + 512;
		const uint32_t wavesPerCu = std::max<uint32_t>(1, std::min<uint32_t>(8, 163840u / ldsBytes));
		// arena rows of a wave = the band columns of its lanes (in blocks of 8 per node), `rowsPerSlice` per lane and slice: sized for the
		// lanes a wave will really carry
		auto layoutFor = [&](uint32_t lanes) {
			P.cap_rows = (uint32_t)std::min<uint64_t>(((uint64_t)P.max_slices * rowsPerSlice * lanes + 64 + 7u) & ~7ull, 0x7ffffff0ull);
			return gal::wave_layout<N>(P.cap_cols, P.cap_rows, P.max_slices, P.cap_moves, LW);
		};
		gal::WaveLayout lay = layoutFor(LW);
		const uint64_t fit = scratchBudget() / std::max<uint64_t>(lay.bytes, 1);
		uint64_t slotsHere = std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)g->cus * wavesPerCu, std::max<uint64_t>(fit, 64)));
		if (knobs.waveSlots) slotsHere = std::min<uint64_t>(slotsHere, knobs.waveSlots);
		// a SMALL batch is spread over all wave slots: a wave's steps cost the same with fewer lanes, and fewer lanes wait for each
		// other less.  A batch that gives at least six of ten slots a full wave runs in full waves: round 3's kernel is more sensitive
		// to the waves it shares its CU's memory path with than to the lanes it waits for (50 000 reads: 782 full waves 28.5 ms,
		// 1 021 waves of 49 reads 30.2 ms on the same box, profiles/r3_ab_lanes_per_wave.txt; round 2's kernel: the other way round)
		uint32_t lanesPer = LW;
		if (knobs.spread > 1) lanesPer = (uint32_t)std::min<int>(LW, knobs.spread);
		else if (knobs.spread && list.size() * 10 < slotsHere * LW * 6)
			lanesPer = (uint32_t)std::min<uint64_t>(LW, std::max<uint64_t>(8, (list.size() + slotsHere - 1) / slotsHere));
		P.lanes_per_wave = lanesPer;
		lay = layoutFor(lanesPer);
		P.wave_bytes = lay.bytes;
		const uint64_t groups = (list.size() + lanesPer - 1) / lanesPer;
		const uint32_t waves = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(slotsHere, groups));
		bool fromPool = false;
		uint8_t* scratch = takeScratch((size_t)waves * lay.bytes, fromPool);
		if (!scratch) return 0;                            // no memory for this variant: the jobs keep their status and climb on
		P.scratch = scratch;
		int rc = uploadList(list);
		if (!rc)
		{
			hipMemsetAsync(L.next_job, 0, 16, stream);
			hipEventRecord(evA, stream);
			if (P.emit_runs) hipLaunchKernelGGL((ga_lanes_kernel<N, LW>), dim3(waves), dim3(64), 0, stream, P);
			else hipLaunchKernelGGL((ga_lanes_moves_kernel<N, LW>), dim3(waves), dim3(64), 0, stream, P);
			float ms = 0;
			rc = afterPass(ms);
			if (first) { st.main_ms = ms; st.main_variant = N * 1000 + 80 + (LW == 64 ? 0 : 1); st.slots = waves; st.waves_per_cu = wavesPerCu; st.scratch_bytes = (uint64_t)waves * lay.bytes; }
			if (knobs.debugPasses) fprintf(stderr, "graphaligner_amd: lanes pass <%d,%d>: %zu jobs on %u waves of %u lanes (%.1f GB scratch), %.2f ms\n", N, LW, list.size(), waves, lanesPer, waves * (double)lay.bytes / 1e9, ms);
#if GA_STAMPS == 3
			{
				uint64_t lo = ~0ull, hi = 0, n = 0; double life = 0, cyc = 0, lateStart = 0;
				for (auto& o : outs) if (o.stamps[1]) { lo = std::min(lo, o.stamps[0]); hi = std::max(hi, o.stamps[1]); }
				for (auto& o : outs) if (o.stamps[1]) { n++; life += (double)(o.stamps[1] - o.stamps[0]); cyc += (double)o.stamps[4]; lateStart = std::max(lateStart, (double)(o.stamps[0] - lo)); }
				{
					// the spread of the waves' lifetimes, and what goes with a long one (fill steps are not known per wave; traceback rounds are)
					std::vector<std::pair<double, uint64_t>> lives;
					for (auto& o : outs) if (o.stamps[1]) lives.push_back({(double)(o.stamps[1] - o.stamps[0]) / 1e5, o.stamps[7]});
					std::sort(lives.begin(), lives.end());
					auto at = [&](double q) { return lives[(size_t)(q * (lives.size() - 1))]; };
					if (!lives.empty()) fprintf(stderr, "graphaligner_amd: wave life ms p10 %.2f p50 %.2f p90 %.2f p99 %.2f max %.2f; traceback rounds of the p10 / p50 / p99 / max wave: %llu / %llu / %llu / %llu, fast iterations %llu / %llu / %llu / %llu\n",
						at(0.1).first, at(0.5).first, at(0.9).first, at(0.99).first, at(1.0).first,
						(unsigned long long)(at(0.1).second & 0xffffffffu), (unsigned long long)(at(0.5).second & 0xffffffffu), (unsigned long long)(at(0.99).second & 0xffffffffu), (unsigned long long)(at(1.0).second & 0xffffffffu),
						(unsigned long long)(at(0.1).second >> 32), (unsigned long long)(at(0.5).second >> 32), (unsigned long long)(at(0.99).second >> 32), (unsigned long long)(at(1.0).second >> 32));
				}
				if (n) fprintf(stderr, "graphaligner_amd: %llu waves: first start to last end %.3f ms, mean wave life %.3f ms = %.1f M shader cycles (%.2f GHz), latest start %.3f ms after the first\n",
				               (unsigned long long)n, (hi - lo) / 1e5, life / n / 1e5, cyc / n / 1e6, cyc / life / 10.0, lateStart / 1e5);
			}
#endif
		}
		if (fromPool) g->givePool();
		return rc;
	}

	// the wave-per-read variants: the kernel behind each and what the host has to know about it.  The two with 4 096 band nodes keep
	// their WaveState in the wave's scratch slot in HBM (stateBytes); the two that carry the sparse method have generation-stamped
	// tables, sized for sparseNodes band nodes, that start from zero once per launch.
	struct WaveKernel
	{
		void (*kernel)(GaLaunch);
		int maxN;
		bool general;
		uint64_t stateBytes;
		int sparseNodes;          // 0: the variant does not carry the sparse method
		bool clearSlotBySlot;     // the sparse tables are some 160 MB of a 360 MB slot: cleared slot by slot, and without them cleared nothing is launched
	};
	// the slots of ga_wide_sparse_kernel are some 360 MB each (arena for 2^20-column slices, 2^23 queue entries): a fallback for a few
	// jobs, capped so that a batch of many such jobs does not claim the whole device for it
	static constexpr uint32_t kWideSparseSlots = 32;
	// the scratch slot of each wave-per-read rung, in the order of gald::kRungs
	struct WaveGeom
	{
		uint32_t capCols;
		uint64_t arenaWordsPerSlice;
		uint32_t traceMul, wavesPerCu;
		uint64_t arenaWordsExtra;
		uint32_t slotCap;         // 0: as many slots as fit
	};
	static constexpr WaveGeom kWaveGeom[] = {
		// <GA_FIRST_N,false>: the lean variant over everything (32 band nodes in LDS, 24 waves per CU)
		{4096, 3 * 64 + 5 * 800, 2, 24, 0, 0},
		// <64,false>: 64 band nodes in LDS
		{8192, 3 * 64 + 5 * 2048, 3, 12, 0, 0},
		// <64,true>, <256,true>: the general variants, which also carry the paths for bands with cycles and for ramp redos; 256 band
		// nodes with large buffers
		{8192, 3 * 64 + 5 * 4096, 4, 8, 0, 0},
		{65536, 3 * 256 + 5 * 8192, 6, 4, 0, 0},
		// <4096,true>: bit-vector bands of more than 256 nodes (tangles of short nodes, wide bubbles, fans): 4 096 band nodes with the
		// tables in HBM, one wave per CU.  A bit-vector band has at most 199 999 columns.  Arena per slice: the node table of 4 096 nodes
		// and 32 768 columns -- four times the figure of the pass before for sixteen times its nodes, because what overflows 256 band
		// nodes is short nodes (the passes before allow 32 columns per table node; 8 per node here), and few slices of a job are that
		// wide.  A job that needs more reports GA_CAP_ARENA and goes on to the next pass like every other capacity miss.
		{kCutoffCols, 3 * (uint64_t)kWideNodes + 5 * 32768, 8, 1, 0, 0},
		// <256,true,true>: bands of 200 000 cells and more (the reference's sparse method and backtrace override, ga_sparse.h), with room
		// for every column of every node such a slice touches: 2^20 columns
		{1u << 20, 3 * 256 + 5 * 20000, 8, 1, 48ull << 20, 0},
		// <4096,true,true>: such bands with more than 256 nodes (fans and tangles of hundreds to thousands of nodes): the same with
		// 4 096 band nodes, the state in HBM and tables sized for it.  Arena as above.  No such job, no launch.
		{1u << 20, 3 * (uint64_t)kWideNodes + 5 * 20000, 8, 1, 48ull << 20, kWideSparseSlots},
	};
	static_assert(sizeof(kWaveGeom) / sizeof(kWaveGeom[0]) == sizeof(gald::kRungs) / sizeof(gald::kRungs[0]), "one scratch geometry per wave-per-read rung");

	// one launch of a wave-per-read kernel over `again` (job indices, longest first)
	int wavePass(const WaveKernel& k, const WaveGeom& geo, const std::vector<uint32_t>& again)
	{
		if (ensureRows()) return GA_E_DEVICE;
		GaLaunch Rl = L;
		uint32_t maxRows = 0;
		for (uint32_t i : again) maxRows = std::max(maxRows, jobs[i].n_rows);
		Rl.cap_cols = geo.capCols;
		Rl.trace_cap = maxRows * geo.traceMul + 4096;
		Rl.max_slices = std::max<uint32_t>(maxRows / 64, 1);
		Rl.arena_words = std::min<uint64_t>(64 + (uint64_t)(maxRows / 64) * (gak::kSliceHdrWords + geo.arenaWordsPerSlice) + geo.arenaWordsExtra, 0xfffffff0ull);
		Rl.sparse_bw = k.sparseNodes ? (uint32_t)std::max(std::max(L.initial_bw, L.ramp_bw), 1) : 0u;
		SlotLayout lay = slotLayout(Rl.cap_cols, Rl.max_slices, Rl.arena_words, Rl.trace_cap, Rl.sparse_bw, k.stateBytes, k.maxN);
		const uint64_t sparseBytes = k.sparseNodes > 256 ? gak::sparse_mem_bytes<kWideNodes>(Rl.sparse_bw) : k.sparseNodes ? gak::sparse_mem_bytes<256>(Rl.sparse_bw) : 0;
		Rl.slot_bytes = lay.bytes;
		const uint64_t fit = scratchBudget() / lay.bytes;
		uint32_t rslots = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>((uint64_t)g->cus * geo.wavesPerCu, fit), again.size()));
		if (geo.slotCap) rslots = std::min(rslots, geo.slotCap);
		if (knobs.waveSlots) rslots = std::min(rslots, knobs.waveSlots);
		bool fromPool = false;
		uint8_t* scratch = takeScratch((size_t)rslots * lay.bytes, fromPool);
		if (!scratch) return 0;                            // the affected jobs keep their capacity status
		Rl.scratch = scratch;
		if (passNo == 1) { st.slots = rslots; st.waves_per_cu = geo.wavesPerCu; st.scratch_bytes = (uint64_t)rslots * lay.bytes; }
		Rl.job_list = dList;
		Rl.n_jobs = (uint32_t)again.size();
		int rc = uploadList(again);
		if (!rc)
		{
			hipMemsetAsync(Rl.next_job, 0, 16, stream);
			if (k.clearSlotBySlot)
			{
				for (uint32_t s = 0; s < rslots && !rc; s++)
					if (hipMemsetAsync(scratch + (uint64_t)s * lay.bytes + lay.sparse, 0, sparseBytes, stream) != hipSuccess) rc = GA_E_DEVICE;
			}
			else if (k.sparseNodes) hipMemset2DAsync(scratch + lay.sparse, lay.bytes, 0, sparseBytes, rslots, stream);
		}
		if (!rc)
		{
			hipEventRecord(evA, stream);
			hipLaunchKernelGGL(k.kernel, dim3(rslots), dim3(64), 0, stream, Rl);
			float ms = 0;
			rc = afterPass(ms);
			if (knobs.debugPasses)
			{
				size_t capNodes = 0;
				for (uint32_t i : again) if (outs[i].status == GA_CAP_NODES) capNodes++;
				fprintf(stderr, "graphaligner_amd: wave-per-read pass <%d,%d%s>: %zu jobs on %u slots, %.2f ms, %zu left with GA_CAP_NODES\n", k.maxN, (int)k.general, k.sparseNodes ? ",sparse" : "", again.size(), rslots, ms, capNodes);
			}
		}
		if (fromPool) g->givePool();
		return rc;
	}

	// gald::climb's back end: the one place that names the kernels' template arguments
#ifndef GA_FIRST_N
#define GA_FIRST_N 32
#endif
	int launch(gald::Variant v, const std::vector<uint32_t>& list, bool first)
	{
		constexpr uint64_t kWideState = sizeof(gak::WaveState<kWideNodes>);
		static_assert(gak::Limits<kWideNodes>::kStateInHbm && !gak::Limits<256>::kStateInHbm, "two variants keep their state in HBM: <4096,true> and <4096,true,true>");
		const WaveGeom& geo = kWaveGeom[gald::isLanes(v) ? 0 : v - gald::kLean32];
		switch (v)
		{
		case gald::kLanes10: return lanesPass<10, 64>(list, kLanesRowsPerSlice[0], first);
		case gald::kLanes24: return lanesPass<24, 32>(list, kLanesRowsPerSlice[1], first);
		case gald::kLanes56: return lanesPass<56, 16>(list, kLanesRowsPerSlice[2], first);
		case gald::kLean32:
		{
			if (int rc = wavePass({ga_extend_kernel<GA_FIRST_N, false>, GA_FIRST_N, false, 0, 0, false}, geo, list)) return rc;
			st.main_ms = st.kernel_ms;
			st.main_variant = -GA_FIRST_N;                 // (negative: the wave-per-read kernel with that many band nodes in LDS)
			return 0;
		}
		case gald::kLean64: return wavePass({ga_extend_kernel<64, false>, 64, false, 0, 0, false}, geo, list);
		case gald::kGeneral64: return wavePass({ga_extend_kernel<64, true>, 64, true, 0, 0, false}, geo, list);
		case gald::kGeneral256: return wavePass({ga_extend_kernel<256, true>, 256, true, 0, 0, false}, geo, list);
		case gald::kWide: return wavePass({ga_wide_kernel, kWideNodes, true, kWideState, 0, false}, geo, list);
		case gald::kSparse256: return wavePass({ga_extend_kernel<256, true, true>, 256, true, 0, 256, false}, geo, list);
		case gald::kWideSparse: return wavePass({ga_wide_sparse_kernel, kWideNodes, true, kWideState, kWideNodes, true}, geo, list);
		default: return GA_E_INVALID;
		}
	}

	// ---- GA_F_OPS (ga_ops.h): after the last pass, every finished job's moves coded as runs where they lie -------------------------
	const uint8_t* resSeq = nullptr;   // the batch's resident copy of the reads and, per job, where its rows come from in it
	size_t resSeqBytes = 0;
	const GaEqFill* resFills = nullptr;
	uint8_t opsLut[256];               // the row codes of the read characters
	hipEvent_t evO[4] = {nullptr, nullptr, nullptr, nullptr};
	uint64_t* dOpsOffsets = nullptr;   // device copies, until fetch has brought them down
	uint32_t* dOpsRuns = nullptr;
	uint64_t opsTotal = 0, opsJobs = 0, opsMoves = 0;
	float opsCountMs = 0, opsWriteMs = 0;
	std::vector<uint64_t> opsOffsetsHost;
	std::unique_ptr<uint32_t[]> opsRunsHost;
	void releaseOps()
	{
		if (dOpsOffsets) release(dOpsOffsets);
		if (dOpsRuns) release(dOpsRuns);
		dOpsOffsets = nullptr; dOpsRuns = nullptr;
	}
	int runOps()
	{
		if (!resSeq || !resFills) return GA_E_INVALID;
		const size_t n = jobs.size();
		uint64_t* dCounts; uint8_t *dLut, *dTmp;
		if (alloc(&dCounts, n + 1) || alloc(&dOpsOffsets, n + 1) || alloc(&dLut, 256)) return GA_E_DEVICE;
		size_t tmpBytes = 0;
		HIP_OK(rocprim::exclusive_scan(nullptr, tmpBytes, dCounts, dOpsOffsets, (uint64_t)0, n + 1, rocprim::plus<uint64_t>(), stream));
		if (alloc(&dTmp, tmpBytes + 16)) return GA_E_DEVICE;
		for (hipEvent_t& e : evO) if (!e) HIP_OK(hipEventCreate(&e));
		HIP_OK(hipMemcpyAsync(dLut, opsLut, 256, hipMemcpyHostToDevice, stream));
		HIP_OK(hipMemsetAsync(dCounts, 0, (n + 1) * 8, stream));
		if (uploadList(orderHost)) return GA_E_DEVICE;           // longest first, dealt statically: wave w takes entries w, w + waves, ...
		gao::OpsLaunch O;
		memset(&O, 0, sizeof(O));
		O.graph = L.graph; O.jobs = L.jobs; O.outs = L.outs; O.fills = resFills;
		O.traces = L.traces; O.trace_bytes = L.trace_pool_cap;
		O.seq = resSeq; O.seq_bytes = resSeqBytes; O.row_code = dLut;
		{
			std::lock_guard<std::mutex> guard(g->twinLock);
			O.twin = g->dTwin ? g->dTwin : g->dOpsTwin;
		}
		if (!O.twin) return GA_E_INVALID;
		O.job_list = dList; O.n_jobs = (uint32_t)n;
		O.counts = dCounts; O.offsets = dOpsOffsets;
		uint32_t waves = (uint32_t)std::min<size_t>(n, (size_t)g->cus * 16);
		if (knobs.waveSlots) waves = std::min(waves, knobs.waveSlots);
		HIP_OK(hipEventRecord(evO[0], stream));
		hipLaunchKernelGGL(ga_ops_count_kernel, dim3(waves), dim3(64), 0, stream, O);
		HIP_OK(hipGetLastError());
		HIP_OK(hipEventRecord(evO[1], stream));
		HIP_OK(rocprim::exclusive_scan(dTmp, tmpBytes, dCounts, dOpsOffsets, (uint64_t)0, n + 1, rocprim::plus<uint64_t>(), stream));
		HIP_OK(hipMemcpyAsync(&opsTotal, dOpsOffsets + n, 8, hipMemcpyDeviceToHost, stream));
		HIP_OK(hipStreamSynchronize(stream));
		if (alloc(&dOpsRuns, opsTotal + 1)) return GA_E_DEVICE;
		O.runs = dOpsRuns;
		HIP_OK(hipEventRecord(evO[2], stream));
		hipLaunchKernelGGL(ga_ops_write_kernel, dim3(waves), dim3(64), 0, stream, O);
		HIP_OK(hipGetLastError());
		HIP_OK(hipEventRecord(evO[3], stream));
		HIP_OK(hipStreamSynchronize(stream));
		HIP_OK(hipEventElapsedTime(&opsCountMs, evO[0], evO[1]));
		HIP_OK(hipEventElapsedTime(&opsWriteMs, evO[2], evO[3]));
		release(dCounts); release(dTmp); release(dLut);
		opsJobs = opsMoves = 0;
		for (const GaJobOut& o : outs) if (o.status == GA_OK && o.n_valid > 0 && o.reserved3 != 1) { opsJobs++; opsMoves += o.trace_len; }
		if (knobs.debugPasses) fprintf(stderr, "graphaligner_amd: operations: %llu jobs, %llu moves, %llu runs on %u waves, count %.2f ms, write %.2f ms\n",
		                               (unsigned long long)opsJobs, (unsigned long long)opsMoves, (unsigned long long)opsTotal, waves, opsCountMs, opsWriteMs);
		return 0;
	}
	int fetchOps(GaOpsOut& out) override
	{
		if (!cfg.emit_ops) return GA_E_INVALID;
		out.runs = opsRunsHost.get(); out.offsets = opsOffsetsHost.empty() ? nullptr : opsOffsetsHost.data();
		out.n_runs = opsTotal; out.count_ms = opsCountMs; out.write_ms = opsWriteMs; out.jobs = opsJobs; out.moves = opsMoves;
		return 0;
	}

	// ---- GA_F_PILEUP (ga_pileup.h): the winning jobs' moves, still in the trace pool after the collect, added to a pileup -----------
	hipEvent_t evU[2] = {nullptr, nullptr};
	int addToPileup(GaBackendPileup* to, const GaPileupAdd& add, GaPileupAddOut& out) override
	{
		DevPileup* p = static_cast<DevPileup*>(to);
		if (!cfg.emit_pileup || !p || p->device != g->device || p->entries != ga_pileup_entries((int)p->kind, g->totalBp, g->edgeSlots)) return GA_E_INVALID;
		out = GaPileupAddOut();
		const bool edges = p->kind == (uint32_t)GA_KIND_EDGES;
		if (!add.nList && !(edges ? add.nSlots : add.nPairs)) return 0;
		// everything that can refuse the add is looked at before a block is taken or anything is put on the stream
		const uint32_t* twin = nullptr;
		if (add.nList)
		{
			if (!resSeq || !resFills) return GA_E_INVALID;
			std::lock_guard<std::mutex> guard(g->twinLock);
			twin = g->dTwin ? g->dTwin : g->dOpsTwin;
			if (!twin) return GA_E_INVALID;
		}
		HIP_OK(hipSetDevice(g->device));
		for (hipEvent_t& e : evU) if (!e) HIP_OK(hipEventCreate(&e));
		AddBlocks blocks;
		const int rc = addWith(p, add, twin, out, blocks);
		// the blocks go back to the graph's list whether or not the add went through (after an error, once the stream is idle)
		if (rc) (void)hipStreamSynchronize(stream);
		if (blocks.added) release(blocks.added);
		if (blocks.jobList) release(blocks.jobList);
		if (blocks.lut) release(blocks.lut);
		if (blocks.pairs) release(blocks.pairs);
		if (blocks.slots) release(blocks.slots);
		return rc;
	}
	struct AddBlocks { uint32_t* jobList = nullptr; uint64_t* pairs = nullptr; uint32_t* slots = nullptr; uint8_t* lut = nullptr; unsigned long long* added = nullptr; };
	int addWith(DevPileup* p, const GaPileupAdd& add, const uint32_t* twin, GaPileupAddOut& out, AddBlocks& blocks)
	{
		uint32_t*& dJobList = blocks.jobList; uint64_t*& dPairs = blocks.pairs; uint8_t*& dLut = blocks.lut; unsigned long long*& dAdded = blocks.added;
		// the EDGES kind takes the host's crossings (slot indices) where the other kinds take its items (plane, column)
		const bool edges = p->kind == (uint32_t)GA_KIND_EDGES;
		const size_t nPairs = edges ? 0 : add.nPairs, nSlots = edges ? add.nSlots : 0;
		if (alloc(&dAdded, 1)) return GA_E_DEVICE;
		HIP_OK(hipMemsetAsync(dAdded, 0, 8, stream));
		if (add.nList)
		{
			if (alloc(&dJobList, add.nList) || alloc(&dLut, 256)) return GA_E_DEVICE;
			HIP_OK(hipMemcpyAsync(dJobList, add.list, add.nList * 4, hipMemcpyHostToDevice, stream));
			HIP_OK(hipMemcpyAsync(dLut, opsLut, 256, hipMemcpyHostToDevice, stream));
		}
		if (nPairs)
		{
			if (alloc(&dPairs, nPairs)) return GA_E_DEVICE;
			HIP_OK(hipMemcpyAsync(dPairs, add.pairs, nPairs * 8, hipMemcpyHostToDevice, stream));
		}
		if (nSlots)
		{
			if (alloc(&blocks.slots, nSlots)) return GA_E_DEVICE;
			HIP_OK(hipMemcpyAsync(blocks.slots, add.slots, nSlots * 4, hipMemcpyHostToDevice, stream));
		}
		HIP_OK(hipEventRecord(evU[0], stream));
		if (add.nList && edges)
		{
			gaed::EdgesLaunch P;
			memset(&P, 0, sizeof(P));
			gao::OpsLaunch& O = P.walk;
			O.graph = L.graph; O.jobs = L.jobs; O.outs = L.outs; O.fills = resFills;
			O.traces = L.traces; O.trace_bytes = L.trace_pool_cap;
			O.seq = resSeq; O.seq_bytes = resSeqBytes; O.row_code = dLut;
			O.twin = twin;
			O.n_jobs = (uint32_t)jobs.size();
			P.counts = p->planes; P.mirror = p->mirror; P.entries = p->entries;
			P.list = dJobList; P.n_list = (uint32_t)add.nList; P.added = dAdded;
			uint32_t waves = (uint32_t)std::min<size_t>(add.nList, (size_t)g->cus * 16);
			if (knobs.waveSlots) waves = std::min(waves, knobs.waveSlots);
			hipLaunchKernelGGL(ga_pileup_edges_kernel, dim3(waves), dim3(64), 0, stream, P);
			HIP_OK(hipGetLastError());
		}
		else if (add.nList)
		{
			gapl::PileupLaunch P;
			memset(&P, 0, sizeof(P));
			gao::OpsLaunch& O = P.walk;
			O.graph = L.graph; O.jobs = L.jobs; O.outs = L.outs; O.fills = resFills;
			O.traces = L.traces; O.trace_bytes = L.trace_pool_cap;
			O.seq = resSeq; O.seq_bytes = resSeqBytes; O.row_code = dLut;
			O.twin = twin;
			O.n_jobs = (uint32_t)jobs.size();
			P.planes = p->planes; P.columns = p->entries; P.kind = p->kind;
			P.list = dJobList; P.n_list = (uint32_t)add.nList; P.added = dAdded;
			uint32_t waves = (uint32_t)std::min<size_t>(add.nList, (size_t)g->cus * 16);
			if (knobs.waveSlots) waves = std::min(waves, knobs.waveSlots);
			if (p->kind == gapl::KIND_BASES) hipLaunchKernelGGL(ga_pileup_bases_kernel, dim3(waves), dim3(64), 0, stream, P);
			else hipLaunchKernelGGL(ga_pileup_depth_kernel, dim3(waves), dim3(64), 0, stream, P);
			HIP_OK(hipGetLastError());
		}
		if (nPairs)
		{
			hipLaunchKernelGGL(ga_pileup_pairs_kernel, dim3((uint32_t)((nPairs + 255) / 256)), dim3(256), 0, stream, dPairs, (uint64_t)nPairs, p->planes, p->entries, p->kind);
			HIP_OK(hipGetLastError());
		}
		if (nSlots)
		{
			hipLaunchKernelGGL(ga_pileup_slots_kernel, dim3((uint32_t)((nSlots + 255) / 256)), dim3(256), 0, stream, blocks.slots, (uint64_t)nSlots, p->planes, p->entries);
			HIP_OK(hipGetLastError());
		}
		HIP_OK(hipEventRecord(evU[1], stream));
		unsigned long long added = 0;
		HIP_OK(hipMemcpyAsync(&added, dAdded, 8, hipMemcpyDeviceToHost, stream));
		HIP_OK(hipStreamSynchronize(stream));
		float ms = 0;
		HIP_OK(hipEventElapsedTime(&ms, evU[0], evU[1]));
		out.kernel_ms = ms; out.items = added;
		for (size_t k = 0; k < add.nList; k++)
		{
			const uint32_t job = add.list[k] & ~gapl::kCounts;
			if (!(add.list[k] & gapl::kCounts) || job >= outs.size()) continue;
			const GaJobOut& o = outs[job];
			if (o.status == GA_OK && o.n_valid > 0 && o.reserved3 != 1) { out.jobs++; out.moves += o.trace_len; }
		}
		for (size_t k = 0; k < nPairs; k++)
			if (ga_pileup_plane_in_kind(p->kind, (uint32_t)(add.pairs[k] >> 56)) < p->nPlanes && (add.pairs[k] & 0x00ffffffffffffffull) < p->entries) out.items++;
		for (size_t k = 0; k < nSlots; k++) if (add.slots[k] < p->entries) out.items++;
		if (knobs.debugPasses) fprintf(stderr, "graphaligner_amd: pileup: %llu jobs, %llu moves, %llu items (%zu from the host), %.2f ms\n",
		                               (unsigned long long)out.jobs, (unsigned long long)out.moves, (unsigned long long)out.items, nPairs + nSlots, ms);
		return 0;
	}

	int run() override
	{
		int rc = runLadder();
		if (rc || !cfg.emit_ops) return rc;
		releaseOps();
		opsTotal = opsJobs = opsMoves = 0; opsCountMs = opsWriteMs = 0;
		opsOffsetsHost.clear(); opsRunsHost.reset();
		if (jobs.empty()) { opsOffsetsHost.assign(1, 0); opsRunsHost.reset(new uint32_t[1]); return 0; }
		return runOps();
	}

	int runLadder()
	{
		HIP_OK(hipSetDevice(g->device));
		st = GaRunStats();
		passOf.assign(jobs.size(), 0);
		passNo = 0;
		if (jobs.empty()) return 0;
		// (the records are initialised on the device and come back whole after every pass: nothing to upload here; the host copy's
		// statuses are what the passes select their jobs by, so a batch that is run again starts from "not run" here too)
		for (auto& o : outs) o.status = GA_NOT_RUN;
		hipLaunchKernelGGL(ga_outs_init_kernel, dim3((uint32_t)((jobs.size() + 255) / 256)), dim3(256), 0, stream, L.outs, (uint32_t)jobs.size());
		HIP_OK(hipGetLastError());
		HIP_OK(hipMemsetAsync(L.trace_top, 0, 16, stream));
		// ---- the passes (ga_ladder.h): first the lanes = reads kernel, one job per lane, where the graph's shape makes its lockstep pay
		// -- its LDS tables hold 10, 24 or 56 band nodes per lane, the starting size follows the graph's mean node length, and jobs a
		// size cannot hold move to the next -- or the lean wave-per-read kernel; what is left climbs the wave-per-read rungs.
		// GA_LANES=1 / 0 forces which kernel goes first. ----
		const double meanNode = g->g.n_nodes > 2 ? (double)g->totalBp / (double)(g->g.n_nodes - 2) : 64.0;
		const int rc = gald::climb(orderHost, outs, passOf, passNo, st.jobs_retried, gald::firstPassFor(meanNode, knobs.lanes),
		                           [&](gald::Variant v, const std::vector<uint32_t>& list, bool first) { return launch(v, list, first); });
		for (int k = 0; k < 8; k++) { st.stamps[k] = 0; for (auto& o : outs) st.stamps[k] += o.stamps[k]; }
		return rc;
	}

	uint8_t* hostTraces = nullptr;       // the graph's pinned buffer (hostFromPool) or a private one
	bool hostFromPool = false;
	std::unique_ptr<uint8_t[]> hostPrivate;
	size_t hostPrivateBytes = 0;
	int fetch(std::vector<GaJobOut>& o, const uint8_t** traces, uint64_t* nBytes) override
	{
		HIP_OK(hipSetDevice(g->device));
		fetchDone();
		o = outs;
		for (size_t i = 0; i < o.size(); i++) o[i].reserved2 = passOf[i];      // 0 = finished by the first pass
		uint64_t top = 0;
		// (on the batch's own stream: the null stream would make this wait for whatever kernel another batch is running)
		HIP_OK(hipMemcpyAsync(&top, L.trace_top, 8, hipMemcpyDeviceToHost, stream));
		HIP_OK(hipStreamSynchronize(stream));
		top = std::min<uint64_t>(top, L.trace_pool_cap);
		hostTraces = g->takeHost(top + 64);
		hostFromPool = hostTraces != nullptr;
		if (!hostTraces)
		{
			// another batch of this graph is being assembled from the pinned buffer: pageable memory, not initialised first
			if (hostPrivateBytes < top + 64) { hostPrivate.reset(new uint8_t[top + 64]); hostPrivateBytes = top + 64; }
			hostTraces = hostPrivate.get();
		}
		if (top)
		{
			HIP_OK(hipMemcpyAsync(hostTraces, L.traces, top, hipMemcpyDeviceToHost, stream));
			HIP_OK(hipStreamSynchronize(stream));
		}
		*traces = hostTraces;
		*nBytes = top;
		if (cfg.emit_ops && dOpsOffsets)
		{
			// the runs and their places come down with the records; their buffers go back to the graph's block list
			opsOffsetsHost.resize(jobs.size() + 1);
			opsRunsHost.reset(new uint32_t[opsTotal + 1]);
			HIP_OK(hipMemcpyAsync(opsOffsetsHost.data(), dOpsOffsets, opsOffsetsHost.size() * 8, hipMemcpyDeviceToHost, stream));
			if (opsTotal) HIP_OK(hipMemcpyAsync(opsRunsHost.get(), dOpsRuns, opsTotal * 4, hipMemcpyDeviceToHost, stream));
			HIP_OK(hipStreamSynchronize(stream));
			releaseOps();
		}
		return 0;
	}
	void fetchDone() override
	{
		if (hostFromPool) g->giveHost();
		hostFromPool = false;
		hostTraces = nullptr;
	}
	GaRunStats stats() const override { return st; }
};

}  // namespace

GaBackendGraph* ga_backend_upload_graph(const GaFlatGraph& flat, const GaHmmTables& hmm, int device, int* status)
{
	int count = 0;
	if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count) { *status = GA_E_NO_DEVICE; return nullptr; }
	if (hipSetDevice(device) != hipSuccess) { *status = GA_E_NO_DEVICE; return nullptr; }
	hipDeviceProp_t prop;
	if (hipGetDeviceProperties(&prop, device) != hipSuccess) { *status = GA_E_NO_DEVICE; return nullptr; }
	if (flat.node_start.size() - 1 >= 0xfffffff0ull) { *status = GA_E_INVALID; return nullptr; }      // node indices are 32-bit
	DevGraph* g = new DevGraph();
	g->device = device;
	g->cus = prop.multiProcessorCount;
	g->g.n_nodes = (uint32_t)(flat.node_start.size() - 1);
	g->g.reserved = 0;
	g->totalBp = flat.node_start.back();
	g->edgeSlots = ga_edge_slot_count(flat);
	int bad = 0;
	bad |= g->put(flat.node_start, &g->g.node_start);
	bad |= g->put(flat.seq2, &g->g.seq2);
	bad |= g->put(flat.in_off, &g->g.in_off);
	bad |= g->put(flat.in_nbr, &g->g.in_nbr);
	bad |= g->put(flat.out_off, &g->g.out_off);
	bad |= g->put(flat.out_nbr, &g->g.out_nbr);
	bad |= g->put(ga_build_node_records(flat), &g->g.node_rec);
	std::vector<GaHmmTables> h(1, hmm);
	const GaHmmTables* dh = nullptr;
	bad |= g->put(h, &dh);
	g->hmm = const_cast<GaHmmTables*>(dh);
	if (bad) { delete g; *status = GA_E_DEVICE; return nullptr; }
	g->seed = std::make_unique<gasd::DevSeedEngine>(g, device, g->cus, g->g);
	*status = 0;
	return g;
}

GaBackendBatch* DevGraph::beginSeededBatch(const GaSeededRequest& req, GaSeededPlan& plan, int* status)
{
	DevBatch* b = new DevBatch();
	b->g = this;
	int s = b->beginSeeded(req, plan);
	if (s) { delete b; *status = s; return nullptr; }
	*status = 0;
	return b;
}

GaBackendBatch* ga_backend_create_batch(GaBackendGraph* graph, GaRowsProvider rows, const uint64_t* eq, const GaEqSource* src, size_t eqWords, const std::vector<GaJob>& jobs,
                                        const GaRunConfig& cfg, int* status)
{
	DevBatch* b = new DevBatch();
	b->g = static_cast<DevGraph*>(graph);
	b->cfg = cfg;
	b->rowsProvider = rows;
	int s = b->init(eq, src, eqWords, jobs);
	if (s) { delete b; *status = s; return nullptr; }
	*status = 0;
	return b;
}
