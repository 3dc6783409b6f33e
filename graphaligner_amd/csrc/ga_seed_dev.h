// ga_seed_dev.h -- the gfx950 side of seeding: the kernels around the program of ga_seed.h, and how many waves per CU the two seeding
// kernels are launched with.  The engine that launches them and owns the index in HBM is a part of the host side, ga_dev_seed.h.
// Included by ga_device.hip only.
#pragma once
#include <hip/hip_runtime.h>

#include "ga_backend.h"
#include "ga_seed.h"

namespace gasd {

// index build, once per graph: one lane per node (a node's k-mers must leave in offset order, and the key rolls along the node)
__global__ void __launch_bounds__(256) ga_seed_count_kernel(GaDevGraph g, uint32_t k, uint32_t sampleShift, uint64_t* counts)
{
	const uint32_t node = blockIdx.x * 256u + threadIdx.x;
	if (node < g.n_nodes) gas::index_count(g, node, k, sampleShift, counts);
	else if (node == g.n_nodes) counts[node] = 0;                         // (the scan's last element = the total)
}
__global__ void __launch_bounds__(256) ga_seed_write_kernel(GaDevGraph g, uint32_t k, uint32_t sampleShift, const uint64_t* firstEntry, uint64_t* keys, uint64_t* vals)
{
	const uint32_t node = blockIdx.x * 256u + threadIdx.x;
	if (node < g.n_nodes) gas::index_write(g, node, k, sampleShift, firstEntry, keys, vals);
}
__global__ void __launch_bounds__(256) ga_seed_dir_kernel(const uint64_t* keys, uint32_t n, uint32_t dirShift, uint32_t buckets, uint32_t* dir, unsigned long long* distinct)
{
	const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
	if (i > n) return;
	gas::index_dir(keys, n, dirShift, buckets, dir, (uint32_t)i);
	const bool isNew = i < n && (i == 0 || keys[i] != keys[i - 1]);
	const uint64_t m = __ballot(isNew);
	if (m != 0 && (threadIdx.x & 63) == (uint32_t)__builtin_ctzll(m)) atomicAdd(distinct, (unsigned long long)__builtin_popcountll(m));
}
// index build with walks: one lane per node as above, one wave per block: the block's LDS is the 64 lanes' walk stacks
__global__ void __launch_bounds__(64) ga_seed_walk_count_kernel(GaDevGraph g, uint32_t k, uint32_t sampleShift, uint32_t maxWalks, uint64_t* counts, unsigned long long* tally)
{
	__shared__ gas::WalkStack st;
	const uint32_t node = blockIdx.x * 64u + threadIdx.x;
	gas::WalkTally t{0, 0, 0};
	if (node < g.n_nodes) gas::walk_index_count(g, node, k, sampleShift, maxWalks, st, (int)threadIdx.x, t, counts);
	else if (node == g.n_nodes) counts[node] = 0;
	unsigned long long v[3] = {t.tail_starts, t.skipped, t.walks};
#pragma unroll
	for (int q = 0; q < 3; q++)
	{
		for (int d = 32; d >= 1; d >>= 1) v[q] += __shfl_down(v[q], d, 64);
		if (threadIdx.x == 0 && v[q] != 0) atomicAdd(tally + q, v[q]);
	}
}
__global__ void __launch_bounds__(64) ga_seed_walk_write_kernel(GaDevGraph g, uint32_t k, uint32_t sampleShift, uint32_t maxWalks, const uint64_t* firstEntry, uint64_t* keys, uint64_t* vals)
{
	__shared__ gas::WalkStack st;
	const uint32_t node = blockIdx.x * 64u + threadIdx.x;
	if (node < g.n_nodes) gas::walk_index_write(g, node, k, sampleShift, maxWalks, st, (int)threadIdx.x, firstEntry, keys, vals);
}
// equal (key, node, offset) triples are neighbours after the sort: flag the first of each, scan, move the flagged ones
__global__ void __launch_bounds__(256) ga_seed_flag_kernel(const uint64_t* keys, const uint64_t* vals, uint32_t n, uint32_t* flags)
{
	const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
	if (i < n) flags[i] = gas::index_first_of_its_kind(keys, vals, (uint32_t)i);
	else if (i == n) flags[i] = 0;                                          // (the scan's last element = the number kept)
}
__global__ void __launch_bounds__(256) ga_seed_compact_kernel(const uint64_t* keys, const uint64_t* vals, uint32_t n, const uint32_t* pos, uint64_t* outKeys, uint64_t* outVals)
{
	const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
	if (i >= n) return;
	const uint32_t at = pos[i];
	if (pos[i + 1] != at) { outKeys[at] = keys[i]; outVals[at] = vals[i]; }
}
// the topology coordinate (ga_seed.h): one lane per node, one launch per step; a launch ors "still moving" into a word of its own, which
// the host reads before it decides on the next launch, and the two counting launches add the wave's count to a counter
__device__ __forceinline__ void coord_flag(bool moving, uint32_t* flag)
{
	if (__ballot(moving) != 0 && (threadIdx.x & 63) == 0) *flag = 1;       // (every wave that writes writes 1)
}
__device__ __forceinline__ void coord_count(bool one, uint32_t* counter)
{
	const uint64_t m = __ballot(one);
	if (m != 0 && (threadIdx.x & 63) == 0) atomicAdd(counter, (uint32_t)__builtin_popcountll(m));
}
__global__ void __launch_bounds__(256) ga_coord_parent_kernel(GaDevGraph g, uint32_t* par, uint32_t* parLen, gas::CoordCyc* cyc, uint32_t* flag)
{
	const uint32_t v = blockIdx.x * 256u + threadIdx.x;
	bool mv = false;
	if (v < g.n_nodes) { gas::coord_parent(g, v, par, parLen); mv = gas::coord_cyc_init(par, v, cyc); }
	coord_flag(mv, flag);
}
__global__ void __launch_bounds__(256) ga_coord_cyc_round_kernel(uint32_t n, const gas::CoordCyc* a, gas::CoordCyc* o, uint32_t* flag)
{
	const uint32_t v = blockIdx.x * 256u + threadIdx.x;
	coord_flag(v < n && gas::coord_cyc_round(a, o, v), flag);
}
__global__ void __launch_bounds__(256) ga_coord_mark_kernel(uint32_t n, const gas::CoordCyc* a, uint32_t* mark)
{
	const uint32_t v = blockIdx.x * 256u + threadIdx.x;
	if (v < n) gas::coord_mark(a, mark, v);
}
__global__ void __launch_bounds__(256) ga_coord_cut_kernel(uint32_t n, const gas::CoordCyc* a, const uint32_t* mark, uint32_t* par, uint32_t* cuts)
{
	const uint32_t v = blockIdx.x * 256u + threadIdx.x;
	coord_count(v < n && gas::coord_cut(a, mark, par, v), cuts);
}
__global__ void __launch_bounds__(256) ga_coord_depth_init_kernel(uint32_t n, const uint32_t* par, const uint32_t* parLen, gas::CoordDepth* o, uint32_t* flag)
{
	const uint32_t v = blockIdx.x * 256u + threadIdx.x;
	coord_flag(v < n && gas::coord_depth_init(par, parLen, v, o), flag);
}
__global__ void __launch_bounds__(256) ga_coord_depth_round_kernel(uint32_t n, const gas::CoordDepth* a, gas::CoordDepth* o, uint32_t* flag)
{
	const uint32_t v = blockIdx.x * 256u + threadIdx.x;
	coord_flag(v < n && gas::coord_depth_round(a, o, v), flag);
}
// one max per wave and root: the lanes that share the root of the first lane still left take their max by butterfly, that lane sends
// it, and they leave; a counted loop whose exit is the wave's own ballot (one pass on a chain, at most 64 when every lane has another root)
__global__ void __launch_bounds__(256) ga_coord_extent_kernel(GaDevGraph g, const gas::CoordDepth* a, uint64_t* ext)
{
	const uint32_t v = blockIdx.x * 256u + threadIdx.x;
	const int lane = (int)(threadIdx.x & 63);
	uint32_t root = 0;
	uint64_t end = 0;
	bool have = v < g.n_nodes && gas::coord_extent_of(g, a, v, root, end);
	uint64_t left = __ballot(have);
	for (int pass = 0; pass < 64 && left != 0; pass++)
	{
		const int first = __builtin_ctzll(left);
		const uint32_t r = (uint32_t)__shfl((int)root, first, 64);
		const bool mine = have && root == r;
		unsigned long long m = mine ? end : 0ull;
		for (int d = 32; d >= 1; d >>= 1) { const unsigned long long o = __shfl_xor(m, d, 64); m = o > m ? o : m; }
		if (lane == first) gas::acc_max(ext + r, (uint64_t)m);
		have = have && !mine;
		left = __ballot(have);
	}
}
__global__ void __launch_bounds__(256) ga_coord_contrib_kernel(GaDevGraph g, const gas::CoordDepth* a, const uint64_t* ext, uint64_t* contrib, uint32_t* trees)
{
	const uint32_t v = blockIdx.x * 256u + threadIdx.x;
	bool root = false;
	if (v < g.n_nodes) root = gas::coord_contrib(g, a, ext, contrib, v);
	else if (v == g.n_nodes) contrib[v] = 0;                              // (the scan's last element = the sum over the trees)
	coord_count(root, trees);
}
__global__ void __launch_bounds__(256) ga_coord_write_kernel(GaDevGraph g, const gas::CoordDepth* a, const uint64_t* base, int64_t* linx)
{
	const uint32_t v = blockIdx.x * 256u + threadIdx.x;
	if (v < g.n_nodes) gas::coord_write(g, a, base, linx, v);
}
// the hot path: one wave per read at a time
__global__ void __launch_bounds__(64) ga_seed_find_kernel(gas::SeedLaunch L)
{
	__shared__ gas::SeedLds lds;
	gas::seed_wave(L, lds, blockIdx.x, gridDim.x);
}
// the same with one seed per locus (ga_find_seeds_loci)
__global__ void __launch_bounds__(64) ga_seed_find_loci_kernel(gas::SeedLaunch L)
{
	__shared__ gas::SeedLdsLoci lds;
	gas::seed_wave_loci(L, lds, blockIdx.x, gridDim.x);
}

constexpr size_t kWavesPerCu = 16;
// seeds per locus: its passes over the hits wait on loads more than the lookup does, and 24 waves per CU hide that better (the linear
// benchmark's batch: 16.2 ms with 16, 13.8 with 20, 12.2 with 24, 16.9 with 28, the most its 67 VGPRs allow: profiles/seed_loci_waves_per_cu.txt)
constexpr size_t kLociWavesPerCu = 24;

}  // namespace gasd
