// ga_emul_hooks.cpp -- TEST-ONLY (ga_emul.h): component hooks for unit tests of pieces of graphaligner_amd/csrc/ga_kernel.h, ga_sparse.h
// and ga_lanes.h, each run on the host with the wave primitives of ga_wave_emul.h, and of the ladder's policy (ga_ladder.h).
#include <algorithm>
#include <cstring>
#include <memory>
#include <unordered_map>
#include <vector>

#include "../../graphaligner_amd/csrc/ga_backend.h"
#include "../../graphaligner_amd/csrc/ga_kernel.h"
#include "../../graphaligner_amd/csrc/ga_ladder.h"
#include "../../graphaligner_amd/csrc/ga_lanes.h"

// component hooks for unit tests of the order-emulation pieces
extern "C" int ga_emul_hash_order(const uint32_t* keys, int n, int32_t* out)
{
	auto ws = std::make_unique<gak::WaveState<256>>();
	if (n > 256) return -1;
	gak::hash_order(*ws, keys, n);
	for (int i = 0; i < n; i++) out[i] = ws->h_order[i];
	return n;
}

extern "C" int ga_emul_hash_order_lanes(const uint32_t* keys, int n, int32_t* out)
{
	auto ws = std::make_unique<gak::WaveState<64>>();
	if (n > 64) return -1;
	gak::hash_order_lanes(*ws, keys, n);
	for (int i = 0; i < n; i++) out[i] = ws->h_order[i];
	return n;
}

// the same through the lane-resident heap
extern "C" int ga_emul_heap_lanes(const uint32_t* nodes, const int32_t* prios, int nOps, uint32_t* popped)
{
	gak::LaneHeap<4> h;
	for (int i = 0; i < 4; i++) { h.node[i] = gaw::VI(0); h.prio[i] = gaw::VI(0); }
	int size = 0, k = 0;
	for (int i = 0; i < nOps; i++)
	{
		if (prios[i] >= 0) { if (!h.push(size, nodes[i], prios[i])) return -1; }
		else if (size > 0) { popped[k++] = (uint32_t)h.getNode(0); h.pop(size); }
	}
	while (size > 0) { popped[k++] = (uint32_t)h.getNode(0); h.pop(size); }
	return k;
}

// push (node, prio) pairs then pop everything; ops: prio >= 0 push, prio < 0 pop.  returns pop order
extern "C" int ga_emul_heap(const uint32_t* nodes, const int32_t* prios, int nOps, uint32_t* popped)
{
	auto ws = std::make_unique<gak::WaveState<256>>();
	int size = 0, k = 0;
	for (int i = 0; i < nOps; i++)
	{
		if (prios[i] >= 0) { if (!gak::heap_push(*ws, size, nodes[i], prios[i])) return -1; }
		else if (size > 0) { popped[k++] = ws->heap_node[0]; gak::heap_pop(*ws, size); }
	}
	while (size > 0) { popped[k++] = ws->heap_node[0]; gak::heap_pop(*ws, size); }
	return k;
}

// ---- component hooks for the lanes = reads program (graphaligner_amd/csrc/ga_lanes.h) ---------------------------------------
// column = {vp, vn, before}
extern "C" void ga_emul_lanes_merge(const uint64_t* a, const uint64_t* b, uint64_t* out)
{
	gal::Col x{a[0], a[1], (int)(int64_t)a[2]}, y{b[0], b[1], (int)(int64_t)b[2]};
	gal::column_merge(x, y);
	out[0] = x.vp; out[1] = x.vn; out[2] = (uint64_t)(int64_t)x.before;
}
// the vertical re-entry: cell-wise minimum with the run coming down from a cell d below the column's row j-1 score
extern "C" void ga_emul_lanes_reenter(const uint64_t* a, int d, uint64_t* out)
{
	gal::Col x{a[0], a[1], (int)(int64_t)a[2]};
	gal::column_reenter(x, d);
	out[0] = x.vp; out[1] = x.vn; out[2] = (uint64_t)(int64_t)x.before;
}
// one column step (Eq word, "no diagonal into row j", new row j-1 score)
extern "C" void ga_emul_lanes_step(const uint64_t* a, uint64_t eq, int noDiag, int calc, uint64_t* out)
{
	gal::Col x{a[0], a[1], (int)(int64_t)a[2]};
	gal::column_step(x, eq, noDiag != 0, calc);
	out[0] = x.vp; out[1] = x.vn; out[2] = (uint64_t)(int64_t)x.before;
}
// map iteration order and heap pop order of the per-lane tables (one lane, N = 56)
extern "C" int ga_emul_lanes_hash_order(const uint32_t* keys, int n, int32_t* out)
{
	typedef gal::Lay<56> LY;
	if (n > 56) return -1;
	std::vector<uint32_t> lds((size_t)LY::WORDS);
	gal::Lds l{lds.data(), 1};
	for (int i = 0; i < n; i++) l.wr(LY::P_NODE + i, keys[i]);
	gal::hash_order<56>(l, n);
	for (int i = 0; i < n; i++) out[i] = (int32_t)l.rdb(LY::X_HASH, LY::HB_ORDER + i);
	return n;
}
extern "C" int ga_emul_lanes_heap(const uint32_t* nodes, const int32_t* prios, int nOps, uint32_t* popped)
{
	typedef gal::Lay<56> LY;
	std::vector<uint32_t> lds((size_t)LY::WORDS);
	gal::Lds l{lds.data(), 1};
	int size = 0, k = 0;
	for (int i = 0; i < nOps; i++)
	{
		if (prios[i] >= 0) { if (!gal::heap_push<56>(l, size, nodes[i], prios[i])) return -1; }
		else if (size > 0) { popped[k++] = l.rd(LY::X_HEAPN); gal::heap_pop<56>(l, size); }
	}
	while (size > 0) { popped[k++] = l.rd(LY::X_HEAPN); gal::heap_pop<56>(l, size); }
	return k;
}

// ---- bands of up to 4 096 nodes ---------------------------------------------------------------------------------------------------
// component hook: the map iteration order for up to 4 096 keys (tests/test_wide_bands.py compares it with a real std::unordered_map)
extern "C" int ga_emul_wide_hash_order(const uint32_t* keys, int n, int32_t* out)
{
	auto ws = std::make_unique<gak::WaveState<4096>>();
	if (n > 4096) return -1;
	gak::hash_order(*ws, keys, n);
	for (int i = 0; i < n; i++) out[i] = ws->h_order[i];
	return n;
}

// sizeof(WaveState<4096>): what a slot of the device's wide pass sets aside for it
extern "C" uint64_t ga_emul_wide_state_bytes() { return sizeof(gak::WaveState<4096>); }

// what hash_order has to reproduce: the iteration order of a real std::unordered_map<size_t, ..> of this build's libstdc++ after the keys
// went in one by one (NodeSlice.h:728-738); `buckets` (may be null) receives the bucket count after each insertion
extern "C" int ga_emul_wide_unordered_map_order(const uint32_t* keys, int n, int64_t* out, int32_t* buckets)
{
	std::unordered_map<size_t, int> m;
	for (int i = 0; i < n; i++)
	{
		m[(size_t)keys[i]] = i;
		if (buckets) buckets[i] = (int32_t)m.bucket_count();
	}
	int k = 0;
	for (const auto& kv : m) out[k++] = (int64_t)kv.first;
	return k;
}

// ---- the sparse method with 4 096 band nodes (ga_sparse.h) --------------------------------------------------------------------------
// component hook: the hashed node -> slot table of ga_sparse.h as sparse_fill uses it.  touches[0..n) = the nodes in the order the
// queue meets them; slots[i] = the slot touch i resolves to, order[] = the nodes in slot order (first touch).  Run `rounds` times over
// one table, each round with the next stamp: a round must not see the entries of the round before.  Returns the number of slots.
extern "C" int ga_emul_wide_sparse_node_slots(const uint32_t* touches, int n, int rounds, int32_t* slots, uint32_t* order)
{
	constexpr uint32_t size = gak::SparseLimits<4096>::kNodeMap;
	std::vector<uint32_t> mem(3 * (size_t)gak::SparseLimits<4096>::kNodeTabs * size, 0);
	gak::SparseMem sm;
	memset(&sm, 0, sizeof(sm));
	sm.nodeKey = mem.data(); sm.nodeGen = sm.nodeKey + gak::SparseLimits<4096>::kNodeTabs * size; sm.nodeVal = sm.nodeGen + gak::SparseLimits<4096>::kNodeTabs * size;
	int cn = 0;
	for (int r = 0; r < rounds; r++)
	{
		const gak::NodeTab tab = gak::node_tab(sm, (uint32_t)r % gak::SparseLimits<4096>::kNodeTabs, size, (uint32_t)r / gak::SparseLimits<4096>::kNodeTabs + 1);
		cn = 0;
		for (int i = 0; i < n; i++)
		{
			int s = gak::node_tab_find(tab, touches[i]);
			if (s < 0)
			{
				if (cn >= 4096) return -1;
				s = cn++;
				order[s] = touches[i];
				gak::node_tab_put(tab, touches[i], (uint32_t)s);
			}
			slots[i] = s;
		}
	}
	return cn;
}
// the table's size and its hash, so that a test can build keys that collide
extern "C" uint32_t ga_emul_wide_sparse_node_map_size() { return gak::SparseLimits<4096>::kNodeMap; }
extern "C" uint32_t ga_emul_wide_sparse_node_hash(uint32_t node) { return gak::mix64(node) & (gak::SparseLimits<4096>::kNodeMap - 1); }
// the limits of the two sparse variants: [set, map, words, entries, node map] for 256 and for 4 096 band nodes
extern "C" void ga_emul_wide_sparse_limits(uint32_t* out)
{
	using A = gak::SparseLimits<256>; using B = gak::SparseLimits<4096>;
	const uint32_t v[10] = {A::kSetSize, A::kMapSize, A::kSparseWords, A::kSparseEntries, A::kNodeMap, B::kSetSize, B::kMapSize, B::kSparseWords, B::kSparseEntries, B::kNodeMap};
	for (int i = 0; i < 10; i++) out[i] = v[i];
}
// bytes of the 256 variant's sparse tables at a bandwidth (its layout is pinned: 256 + the six regions of DESIGN.md section 4b)
extern "C" uint64_t ga_emul_wide_sparse_mem_bytes(int nodes, uint32_t bw) { return nodes > 256 ? gak::sparse_mem_bytes<4096>(bw) : gak::sparse_mem_bytes<256>(bw); }

// ---- the ladder's policy (ga_ladder.h) over a scripted back end: n jobs in index order, and after[v * n + j] = the status job j has
// after variant v ran it.  Out: per launch [variant, first, list size], the lists one after the other (at most gald::kVariants * n
// entries), passOf per job, the retried count.  Returns the number of launches.
extern "C" int ga_emul_ladder_climb(int n, int lanesFirst, int startLanes, uint32_t minJobsLater, const int32_t* after, int32_t* launches, uint32_t* lists, uint8_t* passOf, uint64_t* retried)
{
	std::vector<uint32_t> order(n);
	for (int i = 0; i < n; i++) order[i] = (uint32_t)i;
	std::vector<GaJobOut> outs(n, GaJobOut{});
	for (auto& o : outs) o.status = GA_NOT_RUN;
	std::vector<uint8_t> of(n, 0);
	int passNo = 0, nLaunches = 0;
	size_t at = 0;
	gald::climb(order, outs, of, passNo, *retried, gald::FirstPass{lanesFirst != 0, (gald::Variant)startLanes, minJobsLater},
	            [&](gald::Variant v, const std::vector<uint32_t>& list, bool first) {
		launches[3 * nLaunches] = v; launches[3 * nLaunches + 1] = first; launches[3 * nLaunches + 2] = (int32_t)list.size();
		nLaunches++;
		for (uint32_t j : list) { lists[at++] = j; outs[j].status = after[(size_t)v * n + j]; }
		return 0;
	});
	std::copy(of.begin(), of.end(), passOf);
	return nLaunches == passNo ? nLaunches : -1;
}
// the product's first pass for a graph's mean node length and GA_LANES (1 / 0, negative: unset): [lanes first, starting size, minJobsLater]
extern "C" void ga_emul_ladder_first_pass(double meanNodeLength, int forced, int32_t* out)
{
	const gald::FirstPass fp = gald::firstPassFor(meanNodeLength, forced);
	out[0] = fp.lanesFirst; out[1] = fp.startLanes; out[2] = (int32_t)fp.minJobsLater;
}
