// ga_edges.h -- edge support summed on the device: the pileup kind GA_PILEUP_EDGES (include/graphaligner_amd.h states the rule under
// "pileups"; DESIGN.md section 13 argues it).  One plane of 32-bit counters, one entry per SLOT: the in-neighbour lists of the graph laid
// end to end in node-index order, so the edge that enters node `to` through its in-neighbour number k has slot in_off[to] + k -- the
// position the device graph already holds it at.  The program is the walk of ga_ops.h once more (same job list, same waves and same
// `added` total as the kinds of ga_pileup.h) with SINK_EDGES: the walk hands over the slot of every node crossing whose two cells both
// have an item, and the sink adds one there with one no-return 32-bit atomic.
//
// A forward job crosses from -> to and counts at that edge's own slot.  A backward job's cells are mirrored (reverseTrace), so its
// crossing is the other strand's edge twin(to) -> twin(from): its slot is read from the mirror-slot table, 4 bytes per slot, which the
// host builds with the twin table (mirror_slots below; 0xffffffff where the mirror node or the mirror edge does not exist, and then
// nothing is counted).  Crossings that the host derived from a TraceItem list (the two kinds of reads GA_F_OPS names) come as slot
// indices and are added by add_slot, one thread each.
#pragma once
#include "ga_pileup.h"

namespace gaed {

struct EdgesLaunch
{
	gao::OpsLaunch walk;                   // (twin, seq, counts, offsets, runs and job_list are not used)
	uint32_t* counts;                      // [entries]
	const uint32_t* mirror;                // [entries] the slot of the other strand's copy of the edge, or 0xffffffff
	uint64_t entries;                      // = in_off[n_nodes]
	uint32_t n_list, reserved;
	const uint32_t* list;
	unsigned long long* added;
};

// the sink of gao::walk_job<SINK_EDGES>: on the device one per lane, in the host build one per wave
struct EdgeSink
{
	uint32_t* counts;
	const uint32_t* mirror;
	uint64_t entries;
	uint64_t added;
	GAO_FN void item(uint32_t, uint64_t, uint32_t) {}      // (the walk's item code is not reached with SINK_EDGES; it still has to compile)
	GAO_FN void crossing(uint32_t slot, bool backward)
	{
		if (slot >= entries) return;
		if (backward) slot = mirror[slot];
		if (slot >= entries) return;
		gapl::add_one(counts + slot);
		added++;
	}
};

// one wave's share of a launch
GAO_FN void run_wave(const EdgesLaunch& P, gao::OpsLds& lds, uint32_t wave, uint32_t nWaves)
{
	EdgeSink sink{P.counts, P.mirror, P.entries, 0};
	const uint32_t per = nWaves ? (P.n_list + nWaves - 1) / nWaves : 0;
	for (uint32_t k = 0; k < per; k++)
	{
		const uint32_t at = wave + k * nWaves;
		if (at >= P.n_list) break;
		const uint32_t entry = P.list[at], job = entry & ~gapl::kCounts;
		if (!(entry & gapl::kCounts) || job >= P.walk.n_jobs) continue;
		gao::walk_job<gao::SINK_EDGES>(P.walk, lds, job, sink);
		gao::sync();
	}
#ifdef GA_EMULATE
	*P.added += sink.added;
#else
	if (sink.added) (void)__hip_atomic_fetch_add(P.added, (unsigned long long)sink.added, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
}

// crossing i of the host's list
GAO_FN void add_slot(const uint32_t* slots, uint64_t i, uint32_t* counts, uint64_t entries)
{
	const uint32_t slot = slots[i];
	if (slot < entries) gapl::add_one(counts + slot);
}

}  // namespace gaed
