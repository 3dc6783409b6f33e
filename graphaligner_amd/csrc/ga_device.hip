// ga_device.hip -- the gfx950 back end (ga_backend.h), one translation unit.  This file holds the kernels: a __global__ wrapper around
// each device program -- the extension program one wave per read (ga_kernel.h, which brings ga_sparse.h and ga_job.h with run_job;
// the three wrappers build their Slot with makeSlot; state in LDS, or in HBM for bands of up to 4 096 nodes,
// with or without the sparse method) and one lane per read (ga_lanes.h), the match words, the job plan of seeded batches (ga_plan.h),
// the walk over finished jobs' moves as operations, pileups, edge support and path sequences (ga_ops.h, ga_pileup.h, ga_edges.h,
// ga_pathseq.h) and the site queries (ga_sites.h); seeding brings its own (ga_seed_dev.h).  The extension kernels are persistent launches: a wave per scratch slot in HBM,
// pulling jobs from a device-side queue; waves share nothing but the queue counter and the trace pool's bump counter.
// Below the kernels the host side is included in parts, and the entry points of ga_backend.h end the file:
//   ga_dev.h          the graph resident in HBM with its pools and block list, the pileup, the owners of events, streams, blocks and
//                     single device allocations, and what every stage of a batch uses (BatchCore)
//   ga_dev_seed.h     the seed engine: the index and the topology coordinate built as named stages, the launches of the seeding kernels
//                     (included by ga_dev.h between its owners, which the engine uses, and the graph, which holds the engine)
//   ga_dev_prepare.h  a batch's prepare: reads, jobs and match words into device memory; the seeded prepare (BatchPrepared)
//   ga_dev_ladder.h   a batch's run: the scratch geometry and the passes of the ladder, ga_ladder.h (BatchLadder)
//   ga_dev_post.h     after the ladder: operations, path sequences, pileup add, the results' way back (DevBatch); a pileup's site queries
// A batch is built in these layers, each derived from the one before with its state next to its functions.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <chrono>
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
#include "ga_pathseq.h"
#include "ga_sites.h"

namespace {

// the sparse method's tables (ga_sparse.h) for a variant of `bandNodes` band nodes: they are sized per variant, gak::SparseLimits
__host__ __device__ inline uint64_t sparseTableBytes(int bandNodes, uint32_t maxBw) { return bandNodes > 256 ? gak::sparse_mem_bytes<4096>(maxBw) : gak::sparse_mem_bytes<256>(maxBw); }

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
	l.sparse = at; if (sparseBw) at = up(at + sparseTableBytes(sparseNodes, sparseBw));
	l.ovr = at; if (sparseBw) at = up(at + 8ull * (maxSlices + 2));
	// the variant whose band tables do not fit in LDS: its WaveState (0 bytes for every other variant)
	l.state = at; if (stateBytes) at = up(at + stateBytes);
	l.bytes = at;
	return l;
}

// a wave's views of its scratch slot (sparse: the variant carries the sparse method, so its tables and override windows are laid out)
__device__ __forceinline__ gak::Slot makeSlot(const GaLaunch& L, uint8_t* base, const SlotLayout& lay, bool sparse)
{
	gak::Slot slot;
	slot.end_prev = (uint32_t*)(base + lay.endPrev);
	slot.end_cur = (uint32_t*)(base + lay.endCur);
	slot.slice_off = (uint32_t*)(base + lay.sliceOff);
	slot.arena = (uint32_t*)(base + lay.arena);
	slot.trace = base + lay.trace;
	slot.slice_flags = base + lay.flags;
	slot.ckpt = (uint32_t*)(base + lay.ckpt);
	slot.below_off = (uint32_t*)(base + lay.belowOff);
	slot.sparse = sparse ? base + lay.sparse : nullptr;
	slot.ovr = sparse ? (uint32_t*)(base + lay.ovr) : nullptr;
	slot.sparse_max_bw = sparse ? L.sparse_bw : 0u;
	return slot;
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
	const gak::Slot slot = makeSlot(L, base, lay, SPARSE);
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
	const gak::Slot slot = makeSlot(L, base, lay, false);
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
	const gak::Slot slot = makeSlot(L, base, lay, true);
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

// ---- path sequences (ga_pathseq.h): the same walk leaving the graph's base per visited column, counting and writing ---------------
__global__ void __launch_bounds__(64) ga_pathseq_count_kernel(gaps::PathLaunch P)
{
	__shared__ gao::OpsLds lds;
	gaps::run_wave<false>(P, lds, blockIdx.x, gridDim.x);
}
__global__ void __launch_bounds__(64) ga_pathseq_write_kernel(gaps::PathLaunch P)
{
	__shared__ gao::OpsLds lds;
	gaps::run_wave<true>(P, lds, blockIdx.x, gridDim.x);
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

}  // namespace

// ---- the host side, in parts (each opens the unnamed namespace again): what they share, then the batch's stages in the order they run ----
#define GA_DEVICE_PARTS
#include "ga_dev.h"
#include "ga_dev_prepare.h"
#include "ga_dev_ladder.h"
#include "ga_dev_post.h"
#undef GA_DEVICE_PARTS

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
	DevBatch* b = new DevBatch(this);
	int s = b->beginSeeded(req, plan);
	if (s) { delete b; *status = s; return nullptr; }
	*status = 0;
	return b;
}

GaBackendBatch* ga_backend_create_batch(GaBackendGraph* graph, GaRowsProvider rows, const uint64_t* eq, const GaEqSource* src, size_t eqWords, const std::vector<GaJob>& jobs,
                                        const GaRunConfig& cfg, int* status)
{
	DevBatch* b = new DevBatch(static_cast<DevGraph*>(graph));
	b->cfg = cfg;
	b->rowsProvider = rows;
	int s = b->init(eq, src, eqWords, jobs);
	if (s) { delete b; *status = s; return nullptr; }
	*status = 0;
	return b;
}
