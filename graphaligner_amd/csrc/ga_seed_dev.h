// ga_seed_dev.h -- the gfx950 side of seeding: the kernels around the program of ga_seed.h and the engine that owns the index in HBM.
// Included by ga_device.hip only.
#pragma once
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <vector>

#include "ga_backend.h"
#include "ga_seed.h"

namespace gasd {

#define GAS_HIP_OK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { fprintf(stderr, "graphaligner_amd: %s failed: %s\n", #call, hipGetErrorString(e_)); return 102; } } while (0)

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

struct DevSeedEngine : GaSeedEngine
{
	GaBackendGraph* owner;
	int device;
	int cus;
	GaDevGraph g;
	std::mutex lock;                           // one build or find at a time per graph
	gas::SeedIndex ix{};
	GaSeedIndexInfo inf;
	GaSeedWalkInfo winf;
	bool have = false;
	std::vector<int64_t> linxFile;             // the file-order coordinate build() was given: what kind 0 puts back
	GaSeedCoordInfo cinf;
	void* dKeys = nullptr; void* dVals = nullptr; void* dDir = nullptr; void* dLinx = nullptr;
	// buffers of find(), kept between calls
	void* work = nullptr; size_t workBytes = 0;
	void* hits = nullptr; size_t hitsBytes = 0;
	void* loci = nullptr; size_t lociBytes = 0;    // the per-hit buffers of findLoci: allocated at its first call
	hipEvent_t evA = nullptr, evB = nullptr;

	DevSeedEngine(GaBackendGraph* o, int dev, int nCus, const GaDevGraph& graph) : owner(o), device(dev), cus(nCus), g(graph) {}
	void dropIndex()
	{
		for (void** p : {&dKeys, &dVals, &dDir, &dLinx}) { if (*p) hipFree(*p); *p = nullptr; }
		have = false;
	}
	~DevSeedEngine() override
	{
		hipSetDevice(device);
		dropIndex();
		if (work) hipFree(work);
		if (hits) hipFree(hits);
		if (loci) hipFree(loci);
		if (evA) hipEventDestroy(evA);
		if (evB) hipEventDestroy(evB);
	}
	bool built() const override { return have; }
	GaSeedIndexInfo info() const override { return inf; }

	GaSeedWalkInfo walkInfo() const override { return winf; }
	int build(uint32_t k, uint32_t sampleShift, const std::vector<int64_t>& linx) override { return buildIndex(k, sampleShift, 0, linx); }
	int buildWalks(uint32_t k, uint32_t sampleShift, uint32_t maxWalks, const std::vector<int64_t>& linx) override
	{
		if (maxWalks < 1 || maxWalks > 256 || k - 1 > gas::kWalkLevels) return 100;
		return buildIndex(k, sampleShift, maxWalks, linx);
	}

	// maxWalks = 0: the in-node index
	int buildIndex(uint32_t k, uint32_t sampleShift, uint32_t maxWalks, const std::vector<int64_t>& linx)
	{
		std::lock_guard<std::mutex> guard(lock);
		GAS_HIP_OK(hipSetDevice(device));
		dropIndex();
		const auto t0 = std::chrono::steady_clock::now();
		const uint32_t nNodes = g.n_nodes;
		const uint32_t blocks = (nNodes + 1 + 255) / 256;
		const uint32_t walkBlocks = (nNodes + 1 + 63) / 64;
		uint64_t* counts = nullptr; uint64_t* firstEntry = nullptr;
		void* tmp = nullptr; uint64_t* keysIn = nullptr; uint64_t* valsIn = nullptr;
		uint64_t* keysSorted = nullptr; uint64_t* valsSorted = nullptr; uint32_t* flags = nullptr; uint32_t* pos = nullptr; unsigned long long* dTally = nullptr;
		auto cleanup = [&]() { for (void* p : {(void*)counts, (void*)firstEntry, tmp, (void*)keysIn, (void*)valsIn, (void*)keysSorted, (void*)valsSorted, (void*)flags, (void*)pos, (void*)dTally}) if (p) hipFree(p); };
		GaSeedWalkInfo w;
		w.max_walks = maxWalks;
#define GAS_TRY(call) do { if ((call) != hipSuccess) { fprintf(stderr, "graphaligner_amd: %s failed\n", #call); cleanup(); dropIndex(); return 102; } } while (0)
		GAS_TRY(hipMalloc((void**)&counts, ((size_t)nNodes + 1) * 8));
		GAS_TRY(hipMalloc((void**)&firstEntry, ((size_t)nNodes + 1) * 8));
		if (maxWalks)
		{
			GAS_TRY(hipMalloc((void**)&dTally, 3 * 8));
			GAS_TRY(hipMemset(dTally, 0, 3 * 8));
			hipLaunchKernelGGL(ga_seed_walk_count_kernel, dim3(walkBlocks), dim3(64), 0, 0, g, k, sampleShift, maxWalks, counts, dTally);
		}
		else hipLaunchKernelGGL(ga_seed_count_kernel, dim3(blocks), dim3(256), 0, 0, g, k, sampleShift, counts);
		size_t tmpBytes = 0;
		GAS_TRY(rocprim::exclusive_scan(nullptr, tmpBytes, counts, firstEntry, (uint64_t)0, (size_t)nNodes + 1, rocprim::plus<uint64_t>()));
		GAS_TRY(hipMalloc(&tmp, std::max<size_t>(tmpBytes, 16)));
		GAS_TRY(rocprim::exclusive_scan(tmp, tmpBytes, counts, firstEntry, (uint64_t)0, (size_t)nNodes + 1, rocprim::plus<uint64_t>()));
		uint64_t total = 0;
		GAS_TRY(hipMemcpy(&total, firstEntry + nNodes, 8, hipMemcpyDeviceToHost));
		hipFree(tmp); tmp = nullptr;
		if (total >= 0xfffffff0ull) { cleanup(); return 100; }             // entry numbers are 32-bit
		uint32_t n = (uint32_t)total;
		const size_t cap = std::max<size_t>(n, 2);
		GAS_TRY(hipMalloc((void**)&keysIn, cap * 8));
		GAS_TRY(hipMalloc((void**)&valsIn, cap * 8));
		if (maxWalks)
		{
			GAS_TRY(hipMalloc((void**)&keysSorted, cap * 8));
			GAS_TRY(hipMalloc((void**)&valsSorted, cap * 8));
			hipLaunchKernelGGL(ga_seed_walk_write_kernel, dim3(walkBlocks), dim3(64), 0, 0, g, k, sampleShift, maxWalks, firstEntry, keysIn, valsIn);
		}
		else
		{
			GAS_TRY(hipMalloc(&dKeys, cap * 8));
			GAS_TRY(hipMalloc(&dVals, cap * 8));
			hipLaunchKernelGGL(ga_seed_write_kernel, dim3(blocks), dim3(256), 0, 0, g, k, sampleShift, firstEntry, keysIn, valsIn);
		}
		// by key, stable: equal keys keep the (node, offset) order they were written in
		uint64_t* sortedK = maxWalks ? keysSorted : (uint64_t*)dKeys;
		uint64_t* sortedV = maxWalks ? valsSorted : (uint64_t*)dVals;
		if (n > 0)
		{
			tmpBytes = 0;
			GAS_TRY(rocprim::radix_sort_pairs(nullptr, tmpBytes, keysIn, sortedK, valsIn, sortedV, (size_t)n, 0u, 2u * k));
			GAS_TRY(hipMalloc(&tmp, std::max<size_t>(tmpBytes, 16)));
			GAS_TRY(rocprim::radix_sort_pairs(tmp, tmpBytes, keysIn, sortedK, valsIn, sortedV, (size_t)n, 0u, 2u * k));
		}
		if (maxWalks)
		{
			if (tmp) { hipFree(tmp); tmp = nullptr; }
			// two walks of one start with equal text wrote the same triple twice: one stays
			unsigned long long tally[3] = {0, 0, 0};
			GAS_TRY(hipMemcpy(tally, dTally, 3 * 8, hipMemcpyDeviceToHost));
			w.tail_starts = tally[0]; w.tail_starts_skipped = tally[1]; w.walk_kmers = tally[2];
			hipFree(keysIn); keysIn = nullptr;
			hipFree(valsIn); valsIn = nullptr;
			const uint32_t entryBlocks = (uint32_t)(((uint64_t)n + 1 + 255) / 256);
			GAS_TRY(hipMalloc((void**)&flags, ((size_t)n + 1) * 4));
			GAS_TRY(hipMalloc((void**)&pos, ((size_t)n + 1) * 4));
			hipLaunchKernelGGL(ga_seed_flag_kernel, dim3(entryBlocks), dim3(256), 0, 0, keysSorted, valsSorted, n, flags);
			tmpBytes = 0;
			GAS_TRY(rocprim::exclusive_scan(nullptr, tmpBytes, flags, pos, 0u, (size_t)n + 1, rocprim::plus<uint32_t>()));
			GAS_TRY(hipMalloc(&tmp, std::max<size_t>(tmpBytes, 16)));
			GAS_TRY(rocprim::exclusive_scan(tmp, tmpBytes, flags, pos, 0u, (size_t)n + 1, rocprim::plus<uint32_t>()));
			uint32_t unique = 0;
			GAS_TRY(hipMemcpy(&unique, pos + n, 4, hipMemcpyDeviceToHost));
			hipFree(tmp); tmp = nullptr;
			if (unique > n) { cleanup(); return 102; }
			const size_t ucap = std::max<size_t>(unique, 2);
			GAS_TRY(hipMalloc(&dKeys, ucap * 8));
			GAS_TRY(hipMalloc(&dVals, ucap * 8));
			hipLaunchKernelGGL(ga_seed_compact_kernel, dim3(entryBlocks), dim3(256), 0, 0, keysSorted, valsSorted, n, pos, (uint64_t*)dKeys, (uint64_t*)dVals);
			w.duplicates_dropped = n - unique;
			n = unique;
		}
		// the directory: top bits of the key -> first entry; about one entry per bucket
		uint32_t bits = 1;
		while (bits < 2 * k && bits < 28 && (1ull << bits) < n) bits++;
		const uint32_t buckets = 1u << bits;
		unsigned long long* dDistinct = nullptr;
		GAS_TRY(hipMalloc(&dDir, ((size_t)buckets + 2) * 4));
		GAS_TRY(hipMalloc(&dLinx, std::max<size_t>(linx.size(), 1) * 8));
		GAS_TRY(hipMemcpy(dLinx, linx.data(), linx.size() * 8, hipMemcpyHostToDevice));
		dDistinct = (unsigned long long*)counts;                            // (reused: the counts are no longer needed)
		GAS_TRY(hipMemset(dDistinct, 0, 8));
		hipLaunchKernelGGL(ga_seed_dir_kernel, dim3((uint32_t)(((uint64_t)n + 1 + 255) / 256)), dim3(256), 0, 0, (const uint64_t*)dKeys, n, 2 * k - bits, buckets, (uint32_t*)dDir, dDistinct);
		unsigned long long distinct = 0;
		GAS_TRY(hipMemcpy(&distinct, dDistinct, 8, hipMemcpyDeviceToHost));
		GAS_TRY(hipDeviceSynchronize());
#undef GAS_TRY
		cleanup();
		ix.k = k; ix.sample_shift = sampleShift; ix.dir_shift = 2 * k - bits; ix.n_entries = n;
		ix.keys = (const uint64_t*)dKeys; ix.vals = (const uint64_t*)dVals; ix.dir = (const uint32_t*)dDir; ix.linx = (const int64_t*)dLinx;
		inf = GaSeedIndexInfo();
		inf.entries = n; inf.distinct_keys = distinct; inf.k = k; inf.sample_shift = sampleShift; inf.dir_bits = bits;
		inf.bytes = (uint64_t)n * 16 + ((uint64_t)buckets + 1) * 4 + (uint64_t)linx.size() * 8;
		inf.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
		winf = w;
		linxFile = linx;
		cinf = GaSeedCoordInfo();
		have = true;
		return 0;
	}

	GaSeedCoordInfo coordInfo() const override { return cinf; }
	int copyLin(int64_t* lin, size_t capacity) const override
	{
		if (!have) return 100;
		const size_t n = std::min<size_t>(capacity, g.n_nodes);
		if (n == 0) return 0;
		GAS_HIP_OK(hipSetDevice(device));
		GAS_HIP_OK(hipMemcpy(lin, dLinx, n * 8, hipMemcpyDeviceToHost));
		for (size_t i = 0; i < n; i++) lin[i] >>= 1;
		return 0;
	}

	// kind 1: the passes of ga_seed.h ("topology coordinate"), the last of which writes dLinx; the index itself is not touched
	int setCoordinate(int kind, GaSeedCoordInfo& out) override
	{
		std::lock_guard<std::mutex> guard(lock);
		if (!have || (kind != 0 && kind != 1)) return 100;
		GAS_HIP_OK(hipSetDevice(device));
		if (kind == 0)
		{
			GAS_HIP_OK(hipMemcpy(dLinx, linxFile.data(), linxFile.size() * 8, hipMemcpyHostToDevice));
			cinf = GaSeedCoordInfo();
			out = cinf;
			return 0;
		}
		const auto t0 = std::chrono::steady_clock::now();
		const uint32_t n = g.n_nodes, blocks = (n + 255) / 256, blocks1 = (n + 1 + 255) / 256, R = gas::coord_rounds(n);
		// control words: "still moving" of the cycle pass' start and of each of its <= R rounds, of the depth pass' start and of each of
		// its <= R + 1 rounds, then the two counters
		const uint32_t fCyc = 0, fDepth = R + 1, cCuts = 2 * R + 3, cTrees = cCuts + 1, nCtl = cTrees + 1;
		void* stA = nullptr; void* stB = nullptr; uint32_t* par = nullptr; uint32_t* parLen = nullptr; uint32_t* mark = nullptr;
		uint64_t* ext = nullptr; uint64_t* contrib = nullptr; uint64_t* base = nullptr; uint32_t* ctl = nullptr; void* tmp = nullptr;
		auto cleanup = [&]() { for (void* p : {stA, stB, (void*)par, (void*)parLen, (void*)mark, (void*)ext, (void*)contrib, (void*)base, (void*)ctl, tmp}) if (p) hipFree(p); };
#define GAS_TRY(call) do { if ((call) != hipSuccess) { fprintf(stderr, "graphaligner_amd: %s failed\n", #call); cleanup(); return 102; } } while (0)
		GAS_TRY(hipMalloc(&stA, (size_t)n * 16));
		GAS_TRY(hipMalloc(&stB, (size_t)n * 16));
		GAS_TRY(hipMalloc((void**)&par, (size_t)n * 4));
		GAS_TRY(hipMalloc((void**)&parLen, (size_t)n * 4));
		GAS_TRY(hipMalloc((void**)&mark, (size_t)n * 4));
		GAS_TRY(hipMalloc((void**)&ext, (size_t)n * 8));
		GAS_TRY(hipMalloc((void**)&contrib, ((size_t)n + 1) * 8));
		GAS_TRY(hipMalloc((void**)&base, ((size_t)n + 1) * 8));
		GAS_TRY(hipMalloc((void**)&ctl, (size_t)nCtl * 4));
		GAS_TRY(hipMemsetAsync(ctl, 0, (size_t)nCtl * 4, 0));
		GAS_TRY(hipMemsetAsync(mark, 0, (size_t)n * 4, 0));
		GAS_TRY(hipMemsetAsync(ext, 0, (size_t)n * 8, 0));
		auto moving = [&](uint32_t word, bool& mv) { uint32_t w = 0; const hipError_t e = hipMemcpy(&w, ctl + word, 4, hipMemcpyDeviceToHost); mv = w != 0; return e; };
		GaSeedCoordInfo c;
		c.kind = 1;
		// parents, and the cycle pass over them
		gas::CoordCyc* ca = (gas::CoordCyc*)stA; gas::CoordCyc* co = (gas::CoordCyc*)stB;
		hipLaunchKernelGGL(ga_coord_parent_kernel, dim3(blocks), dim3(256), 0, 0, g, par, parLen, ca, ctl + fCyc);
		bool mv = false;
		GAS_TRY(moving(fCyc, mv));
		while (mv && c.cycle_rounds < R)
		{
			hipLaunchKernelGGL(ga_coord_cyc_round_kernel, dim3(blocks), dim3(256), 0, 0, n, (const gas::CoordCyc*)ca, co, ctl + fCyc + 1 + c.cycle_rounds);
			GAS_TRY(moving(fCyc + 1 + c.cycle_rounds, mv));
			c.cycle_rounds++;
			std::swap(ca, co);
		}
		if (mv)
		{
			// walks that never end: mark the cycles' nodes, cut every cycle at its smallest index
			hipLaunchKernelGGL(ga_coord_mark_kernel, dim3(blocks), dim3(256), 0, 0, n, (const gas::CoordCyc*)ca, mark);
			hipLaunchKernelGGL(ga_coord_cut_kernel, dim3(blocks), dim3(256), 0, 0, n, (const gas::CoordCyc*)ca, (const uint32_t*)mark, par, ctl + cCuts);
		}
		// depths in the forest
		gas::CoordDepth* da = (gas::CoordDepth*)stA; gas::CoordDepth* dd = (gas::CoordDepth*)stB;
		hipLaunchKernelGGL(ga_coord_depth_init_kernel, dim3(blocks), dim3(256), 0, 0, n, (const uint32_t*)par, (const uint32_t*)parLen, da, ctl + fDepth);
		GAS_TRY(moving(fDepth, mv));
		while (mv && c.depth_rounds < R + 1)
		{
			hipLaunchKernelGGL(ga_coord_depth_round_kernel, dim3(blocks), dim3(256), 0, 0, n, (const gas::CoordDepth*)da, dd, ctl + fDepth + 1 + c.depth_rounds);
			GAS_TRY(moving(fDepth + 1 + c.depth_rounds, mv));
			c.depth_rounds++;
			std::swap(da, dd);
		}
		if (mv) { cleanup(); return 102; }                                  // (never: a forest's walks are at their roots after R rounds)
		// extents at the roots, bases by a scan in node index order, the write
		hipLaunchKernelGGL(ga_coord_extent_kernel, dim3(blocks), dim3(256), 0, 0, g, (const gas::CoordDepth*)da, ext);
		hipLaunchKernelGGL(ga_coord_contrib_kernel, dim3(blocks1), dim3(256), 0, 0, g, (const gas::CoordDepth*)da, (const uint64_t*)ext, contrib, ctl + cTrees);
		size_t tmpBytes = 0;
		GAS_TRY(rocprim::exclusive_scan(nullptr, tmpBytes, contrib, base, (uint64_t)0, (size_t)n + 1, rocprim::plus<uint64_t>()));
		GAS_TRY(hipMalloc(&tmp, std::max<size_t>(tmpBytes, 16)));
		GAS_TRY(rocprim::exclusive_scan(tmp, tmpBytes, contrib, base, (uint64_t)0, (size_t)n + 1, rocprim::plus<uint64_t>()));
		hipLaunchKernelGGL(ga_coord_write_kernel, dim3(blocks), dim3(256), 0, 0, g, (const gas::CoordDepth*)da, (const uint64_t*)base, (int64_t*)dLinx);
		uint64_t total = 0;
		uint32_t counts[2] = {0, 0};
		GAS_TRY(hipMemcpy(&total, base + n, 8, hipMemcpyDeviceToHost));
		GAS_TRY(hipMemcpy(counts, ctl + cCuts, 8, hipMemcpyDeviceToHost));
		GAS_TRY(hipDeviceSynchronize());
#undef GAS_TRY
		cleanup();
		c.cycles_cut = counts[0]; c.trees = counts[1];
		c.extent_sum = total - (uint64_t)c.trees * (uint64_t)gas::kTreeGap;
		c.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
		cinf = c;
		out = c;
		return 0;
	}

	int copy(uint64_t* keys, uint32_t* nodes, uint32_t* offsets, size_t capacity) const override
	{
		if (!have) return 100;
		const size_t n = std::min<size_t>(capacity, ix.n_entries);
		if (n == 0) return 0;
		GAS_HIP_OK(hipSetDevice(device));
		std::vector<uint64_t> vals(n);
		GAS_HIP_OK(hipMemcpy(keys, dKeys, n * 8, hipMemcpyDeviceToHost));
		GAS_HIP_OK(hipMemcpy(vals.data(), dVals, n * 8, hipMemcpyDeviceToHost));
		for (size_t i = 0; i < n; i++) { nodes[i] = (uint32_t)(vals[i] >> 32); offsets[i] = (uint32_t)vals[i]; }
		return 0;
	}

	int find(const char* const* seqs, const size_t* lens, size_t nReads, const GaSeedParams& p, GaSeedOut& out) override { return run(seqs, lens, nReads, p, out, false); }
	int findLoci(const char* const* seqs, const size_t* lens, size_t nReads, const GaSeedParams& p, GaSeedOut& out) override { return run(seqs, lens, nReads, p, out, true); }

	// what every launch of the seeding kernels shares: the number of wave slots, the per-slot hit (and, by locus, label) buffers, grown
	// when needed, and the launch record but for the reads and the outputs.  Under `lock`.
	int prepareLaunch(gas::SeedLaunch& L, const GaSeedParams& p, size_t nReads, bool byLocus, uint32_t& slots)
	{
		// (the kernel waits on dependent loads: directory, keys, entry, coordinate; sixteen waves per CU hide them, and the kernel's
		// registers and LDS would allow more)
		slots = (uint32_t)std::min<size_t>(nReads, (size_t)std::max(cus, 1) * (byLocus ? kLociWavesPerCu : kWavesPerCu));
		const size_t needHits = (size_t)slots * p.max_hits * 20;
		if (needHits > hitsBytes)
		{
			if (hits) hipFree(hits);
			hits = nullptr; hitsBytes = 0;
			GAS_HIP_OK(hipMalloc(&hits, needHits));
			hitsBytes = needHits;
		}
		const size_t needLoci = byLocus ? (size_t)slots * p.max_hits * 28 : 0;
		if (needLoci > lociBytes)
		{
			if (loci) hipFree(loci);
			loci = nullptr; lociBytes = 0;
			GAS_HIP_OK(hipMalloc(&loci, needLoci));
			lociBytes = needLoci;
		}
		memset(&L, 0, sizeof(L));
		L.ix = ix; L.p = p;
		L.n_reads = (uint32_t)nReads;
		const size_t per = (size_t)slots * p.max_hits;
		L.hit_dx = (int64_t*)hits; L.hit_p = (uint32_t*)((uint8_t*)hits + per * 8); L.hit_node = L.hit_p + per; L.hit_sup = L.hit_node + per;
		if (byLocus) { L.loc_best = (uint64_t*)loci; L.loc_lab = (uint32_t*)((uint8_t*)loci + per * 8); L.loc_alt = L.loc_lab + per; L.loc_last = L.loc_alt + per; L.loc_run = L.loc_last + per; L.loc_nbr = L.loc_run + per; }
		return 0;
	}

	// The seeding kernel over reads that lie in device memory already (a seeded batch, ga_plan.h), on the caller's stream; the outputs stay in
	// device memory, where the caller's pointers say (cleared by the caller).  The caller holds `lock` from before this call until its
	// stream has finished the kernel: the hit and label buffers are per graph.
	int launchResident(const GaSeedParams& p, size_t nReads, bool byLocus, const uint8_t* seq, const gas::SeedRead* reads, const uint32_t* order,
	                   uint32_t* outN, uint32_t* outSeed, uint32_t* outLocus, uint32_t* outNLoci, hipStream_t stream)
	{
		if (!have) return 100;
		gas::SeedLaunch L;
		uint32_t slots = 0;
		if (int st = prepareLaunch(L, p, nReads, byLocus, slots)) return st;
		L.seq = seq; L.reads = reads; L.order = order;
		L.out_n = outN; L.out_seed = outSeed;
		if (byLocus) { L.out_locus = outLocus; L.out_nloci = outNLoci; }
		if (byLocus) hipLaunchKernelGGL(ga_seed_find_loci_kernel, dim3(slots), dim3(64), 0, stream, L);
		else hipLaunchKernelGGL(ga_seed_find_kernel, dim3(slots), dim3(64), 0, stream, L);
		GAS_HIP_OK(hipGetLastError());
		return 0;
	}

	// byLocus: one seed per locus (ga_seed_find_loci_kernel) instead of hit by hit
	int run(const char* const* seqs, const size_t* lens, size_t nReads, const GaSeedParams& p, GaSeedOut& out, bool byLocus)
	{
		std::lock_guard<std::mutex> guard(lock);
		if (!have) return 100;
		out.n_seeds.assign(nReads, 0); out.n_hits.assign(nReads, 0); out.truncated.assign(nReads, 0);
		out.node.assign(nReads * p.max_seeds, 0); out.pos.assign(nReads * p.max_seeds, 0); out.support.assign(nReads * p.max_seeds, 0);
		out.locus_hits.clear(); out.locus_first_p.clear(); out.locus_last_p.clear(); out.n_loci.clear();
		if (byLocus)
		{
			out.locus_hits.assign(nReads * p.max_seeds, 0); out.locus_first_p.assign(nReads * p.max_seeds, 0); out.locus_last_p.assign(nReads * p.max_seeds, 0);
			out.n_loci.assign(nReads, 0);
		}
		out.kernel_ms = 0;
		if (nReads == 0) return 0;
		GAS_HIP_OK(hipSetDevice(device));
		// the batch: characters (every read at a multiple of 16 with 16 bytes of padding behind it), read records, the hand-out order
		std::vector<gas::SeedRead> recs(nReads);
		uint64_t seqBytes = 0;
		for (size_t i = 0; i < nReads; i++)
		{
			if (lens[i] > 0xfffffff0ull) return 100;
			recs[i] = gas::SeedRead{seqBytes, (uint32_t)lens[i], 0};
			seqBytes += ((lens[i] + 15) & ~(size_t)15) + 16;
		}
		std::vector<uint32_t> order(nReads);
		for (size_t i = 0; i < nReads; i++) order[i] = (uint32_t)i;
		std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return lens[a] > lens[b]; });
		auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
		const size_t oSeq = 0, oRecs = up(seqBytes), oOrder = oRecs + up(nReads * sizeof(gas::SeedRead)), oNext = oOrder + up(nReads * 4);      // (oNext: end of the uploaded part)
		const size_t oOutN = oNext, oOutSeed = oOutN + up(nReads * 12), oOutLocus = oOutSeed + up(nReads * p.max_seeds * 12);
		const size_t oOutNLoci = oOutLocus + (byLocus ? up(nReads * p.max_seeds * 12) : 0), total = oOutNLoci + (byLocus ? up(nReads * 4) : 0);
		std::shared_ptr<char> host = owner->hostBlock(oNext);
		if (!host) return 102;
		memset(host.get(), 0, oNext);
		for (size_t i = 0; i < nReads; i++) memcpy(host.get() + recs[i].off, seqs[i], lens[i]);
		memcpy(host.get() + oRecs, recs.data(), nReads * sizeof(gas::SeedRead));
		memcpy(host.get() + oOrder, order.data(), nReads * 4);
		if (total > workBytes)
		{
			if (work) hipFree(work);
			work = nullptr; workBytes = 0;
			GAS_HIP_OK(hipMalloc(&work, total + total / 8));
			workBytes = total + total / 8;
		}
		gas::SeedLaunch L;
		uint32_t slots = 0;
		if (int st = prepareLaunch(L, p, nReads, byLocus, slots)) return st;
		if (!evA) { GAS_HIP_OK(hipEventCreate(&evA)); GAS_HIP_OK(hipEventCreate(&evB)); }
		uint8_t* w = (uint8_t*)work;
		GAS_HIP_OK(hipMemcpyAsync(w, host.get(), oNext, hipMemcpyHostToDevice, 0));
		GAS_HIP_OK(hipMemsetAsync(w + oNext, 0, total - oNext, 0));
		L.seq = w + oSeq; L.reads = (const gas::SeedRead*)(w + oRecs); L.order = (const uint32_t*)(w + oOrder);
		L.out_n = (uint32_t*)(w + oOutN); L.out_seed = (uint32_t*)(w + oOutSeed);
		if (byLocus) { L.out_locus = (uint32_t*)(w + oOutLocus); L.out_nloci = (uint32_t*)(w + oOutNLoci); }
		GAS_HIP_OK(hipEventRecord(evA, 0));
		if (byLocus) hipLaunchKernelGGL(ga_seed_find_loci_kernel, dim3(slots), dim3(64), 0, 0, L);
		else hipLaunchKernelGGL(ga_seed_find_kernel, dim3(slots), dim3(64), 0, 0, L);
		GAS_HIP_OK(hipEventRecord(evB, 0));
		std::vector<uint32_t> outN(nReads * 3), outSeed(nReads * p.max_seeds * 3);
		GAS_HIP_OK(hipMemcpy(outN.data(), w + oOutN, outN.size() * 4, hipMemcpyDeviceToHost));
		GAS_HIP_OK(hipMemcpy(outSeed.data(), w + oOutSeed, outSeed.size() * 4, hipMemcpyDeviceToHost));
		GAS_HIP_OK(hipEventSynchronize(evB));
		float ms = 0;
		GAS_HIP_OK(hipEventElapsedTime(&ms, evA, evB));
		out.kernel_ms = ms;
		for (size_t i = 0; i < nReads; i++) { out.n_seeds[i] = outN[i * 3]; out.n_hits[i] = outN[i * 3 + 1]; out.truncated[i] = outN[i * 3 + 2]; }
		for (size_t i = 0; i < nReads * p.max_seeds; i++) { out.node[i] = outSeed[i * 3]; out.pos[i] = outSeed[i * 3 + 1]; out.support[i] = outSeed[i * 3 + 2]; }
		if (byLocus)
		{
			std::vector<uint32_t> outLocus(nReads * p.max_seeds * 3);
			GAS_HIP_OK(hipMemcpy(outLocus.data(), w + oOutLocus, outLocus.size() * 4, hipMemcpyDeviceToHost));
			GAS_HIP_OK(hipMemcpy(out.n_loci.data(), w + oOutNLoci, nReads * 4, hipMemcpyDeviceToHost));
			for (size_t i = 0; i < nReads * p.max_seeds; i++) { out.locus_hits[i] = outLocus[i * 3]; out.locus_first_p[i] = outLocus[i * 3 + 1]; out.locus_last_p[i] = outLocus[i * 3 + 2]; }
		}
		return 0;
	}
};

}  // namespace gasd
