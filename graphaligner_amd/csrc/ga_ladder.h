// ga_ladder.h -- the ladder: which kernel variants a batch climbs, in which order, and which job statuses each pass picks up.  Host only,
// no HIP.  The one place that knows this policy: the device back end (ga_device.hip) and the tests' host emulation of it
// (tests/emul/ga_emul_ladder.cpp) both call climb() below and only supply launch(): how a variant is run over a list of jobs.
#pragma once
#include <cstdint>
#include <vector>

#include "ga_types.h"

namespace gald {

// the ten kernel variants: lanes = reads <band nodes per lane, lanes per wave>, wave-per-read <band nodes, GENERAL[, SPARSE]>
enum Variant : int
{
	kLanes10,        // <10,64>
	kLanes24,        // <24,32>
	kLanes56,        // <56,16>
	kLean32,         // <32,false>  (the product builds it with GA_FIRST_N band nodes)
	kLean64,         // <64,false>
	kGeneral64,      // <64,true>
	kGeneral256,     // <256,true>
	kWide,           // <4096,true>: band tables in HBM
	kSparse256,      // <256,true,true>: the sparse method and the backtrace override
	kWideSparse,     // <4096,true,true>
	kVariants
};
constexpr bool isLanes(Variant v) { return v <= kLanes56; }

// a set of job statuses, one bit each
constexpr uint64_t bit(int status) { return status == GA_NOT_RUN ? 1ull << 63 : status >= 0 && status < 63 ? 1ull << status : 0; }
constexpr bool takes(uint64_t set, int status) { return (set & bit(status)) != 0; }

// what a lanes = reads variant with larger tables can still take: a capacity of the size before was too small
constexpr uint64_t kLanesMoveOn = bit(GA_CAP_NODES) | bit(GA_CAP_COLS) | bit(GA_CAP_ARENA) | bit(GA_CAP_TRACE) | bit(GA_CAP_HEAP);
// capacity misses, with what the lanes = reads kernel declined and what no kernel has run yet
constexpr uint64_t kCapacity = kLanesMoveOn | bit(GA_PUNT) | bit(GA_NOT_RUN);
// bands with cycles and ramp redos: only the general wave-per-read variants carry those paths
constexpr uint64_t kGeneral = bit(GA_UNSUPPORTED_CYCLE) | bit(GA_UNSUPPORTED_RAMP);

// the wave-per-read rungs in order.  Each selects from ALL jobs by their current status, in hand-out order.
struct Rung
{
	Variant variant;
	uint64_t takes;
	bool firstOnly;      // runs only in a batch whose first pass it is (the lanes = reads kernel did not go first)
};
constexpr Rung kRungs[] = {
	{kLean32, kCapacity, true},                                              // everything: all jobs are GA_NOT_RUN
	{kLean64, kCapacity, false},
	{kGeneral64, kGeneral, false},                                           // only what needs the extra paths: capacity misses go straight on
	{kGeneral256, kCapacity | kGeneral, false},
	{kWide, bit(GA_CAP_NODES) | bit(GA_CAP_HEAP), false},                    // the band tables or the projection heap of 256 nodes overflowed
	{kSparse256, kCapacity | kGeneral | bit(GA_UNSUPPORTED_BAND), false},    // bands of 200 000 cells and more, and the last resort for every miss before
	{kWideSparse, bit(GA_CAP_NODES), false},                                 // only what the pass above left with GA_CAP_NODES; its other misses keep their status
};

// how a batch starts
struct FirstPass
{
	bool lanesFirst;          // the lanes = reads kernel goes first; else kRungs[0]
	Variant startLanes;       // the lanes size that gets all jobs
	uint32_t minJobsLater;    // a later lanes size is only worth a launch of its own for this many jobs; stragglers take the wave-per-read rungs
};
// The lanes = reads kernel is the first pass where its lockstep pays: the lanes of a wave take their k-th band node together, so on
// graphs of long, equally long nodes (mean node length >= 40 bp: linear and sparsely branching graphs) every lane is busy; on graphs
// chopped into short uneven nodes the wave-per-read kernel is still the faster one and goes first.  `forced` (1 / 0, negative: by
// shape) overrides the choice.  The starting size follows the mean node length too: shorter nodes, more band nodes per lane.
inline FirstPass firstPassFor(double meanNodeLength, int forced)
{
	return {forced >= 0 ? forced != 0 : meanNodeLength >= 40, meanNodeLength >= 40 ? kLanes10 : meanNodeLength >= 14 ? kLanes24 : kLanes56, 512};
}

// One run of a batch.  `order` is the hand-out order of all jobs; `outs` is the back end's host copy of the job records, whose statuses
// launch() refreshes.  For every pass with a non-empty list: passOf of its jobs = passNo, passNo++, (wave-per-read) retried += its size,
// then launch(variant, list, first) -- `first`: the batch's first pass -- whose non-zero result ends the climb.  `retried` restarts at 0
// behind a wave-per-read first pass.
template <typename Launch>
int climb(const std::vector<uint32_t>& order, const std::vector<GaJobOut>& outs, std::vector<uint8_t>& passOf, int& passNo, uint64_t& retried, const FirstPass& fp,
          Launch&& launch)
{
	auto pass = [&](Variant v, const std::vector<uint32_t>& list, bool first) {
		for (uint32_t i : list) passOf[i] = (uint8_t)passNo;
		passNo++;
		if (!isLanes(v)) retried += list.size();
		return launch(v, list, first);
	};
	retried = 0;
	if (order.empty()) return 0;
	if (fp.lanesFirst)
	{
		// the first size gets all jobs; jobs a size cannot hold move to the next
		std::vector<uint32_t> list = order;
		bool first = true;
		for (int v = fp.startLanes; v <= kLanes56 && !list.empty(); v++)
		{
			if (!first && list.size() < fp.minJobsLater) break;
			if (int rc = pass((Variant)v, list, first)) return rc;
			first = false;
			std::vector<uint32_t> again;
			for (uint32_t i : list) if (takes(kLanesMoveOn, outs[i].status)) again.push_back(i);
			list.swap(again);
		}
	}
	for (const Rung& r : kRungs)
	{
		if (r.firstOnly && fp.lanesFirst) continue;
		std::vector<uint32_t> list;
		for (uint32_t i : order) if (takes(r.takes, outs[i].status)) list.push_back(i);
		if (!list.empty()) if (int rc = pass(r.variant, list, r.firstOnly)) return rc;
		if (r.firstOnly) retried = 0;
	}
	return 0;
}

}  // namespace gald
