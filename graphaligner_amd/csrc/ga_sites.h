// ga_sites.h -- site queries over a pileup (include/graphaligner_amd.h states the rule under "pileup sites"; DESIGN.md section 14 argues
// it).  The counters of a pileup stay in HBM; this program reads them once, folds the two strands' counters of every candidate entry
// into F[0..planes), tests the thresholds and leaves the entries that pass -- the sites -- as records in ascending entry order.
//
// Two launches with one exclusive scan between them, like ga_ops.h.  The entries of the query's range are cut into TILES of kTile
// consecutive entries, dealt statically (wave w takes tiles w, w + waves, ...); a wave (= one workgroup of 64 lanes) goes through its
// tile in rounds of 64 entries, lane l at entry l of the round.
//   mark:  every lane loads its entry's plane words (planar layout: one plane of a round is one 256-byte load of the wave) and, in fold
//          mode, the partner's, forms F, D, X and the flag; one ballot gives the round's 64-bit mask, which one lane stores (1 bit per
//          entry); the popcounts of a tile's masks are summed and stored once.
//   scan:  the tiles' counts become their places.
//   write: reads the masks; a round whose mask is zero is left without touching the planes; the lanes of set bits form F once more and
//          store their record at offsets[tile] + the sites before it in the tile (popcount of the lower lanes + a running sum).
// So the order of the records comes from the scan and never from an atomic: the same counters give the same bytes.
//
// The node of a column (fold mode of the columns kinds: the partner lies on the twin node, mirrored): one wave-uniform binary search
// in node_start at a round's first column, then a uniform loop over the nodes that meet the round -- at most 64, as nodes have at least
// one base -- in which the lanes inside a node take its fold word, start and length.  mark searches once per tile and carries the node
// from round to round; write searches at the rounds that have a site.
//
// Written in phases (GAO_LANES, sync, ballot, popc of ga_ops.h): on gfx950 a lane block is the lane's straight-line code, in the host
// build of the tests (tests/emul/sites.mk) a loop over the 64 lanes.
#pragma once
#include "ga_ops.h"

namespace gast {

constexpr uint32_t kTile = 1024;                 // entries per tile: 16 rounds
constexpr uint32_t kRounds = kTile / 64;
enum { KIND_COLUMNS1 = 1, KIND_BASES = 8, KIND_EDGES = 32 };

struct SitesLaunch
{
	const uint32_t* planes;                // [nPlanes][entries]
	uint64_t entries;
	uint32_t kind, nPlanes;                // (GA_KIND_*; 8 or 1)
	uint32_t fold, n_nodes;
	const uint64_t* node_start;            // [n_nodes + 1]   (fold over a columns kind)
	const uint32_t* fold_table;            // [n_nodes]       (the same: GA_FOLD_*)
	const uint32_t* mirror;                // [entries]       (fold over the EDGES kind)
	uint64_t first, n;                     // the range
	uint64_t min_depth, min_alt;
	uint32_t alt_num, alt_den;
	uint64_t n_tiles;
	uint64_t* mask;                        // [n_tiles * kRounds]
	uint64_t* counts;                      // [n_tiles + 1] mark: sites per tile (entry n_tiles stays 0)
	const uint64_t* offsets;               // [n_tiles + 1] write: the scanned counts
	GaSiteRec* recs;                       // write: [n_recs]
	uint64_t n_recs;                       // = min(sites, max_sites): a record whose place is not below it is dropped
};

struct SitesLds { uint8_t flag[64]; };

// the node whose columns hold `col` (col < node_start[n_nodes]); the same in every lane
GAO_FN uint32_t node_of(const SitesLaunch& L, uint64_t col)
{
	uint32_t lo = 0, hi = L.n_nodes;         // node_start[lo] <= col < node_start[hi]
	while (hi - lo > 1)
	{
		const uint32_t mid = lo + (hi - lo) / 2;
		if (L.node_start[mid] <= col) lo = mid; else hi = mid;
	}
	return lo;
}

// one lane: is `e` a candidate, and its folded counts.  node0 (fold over a columns kind) is the node of the round's first column r0
GAO_FN bool fold_entry(const SitesLaunch& L, uint64_t e, uint64_t r0, uint32_t node0, uint32_t F[8])
{
	for (int p = 0; p < 8; p++) F[p] = 0;
	if (e >= L.entries) return false;
	if (L.kind == KIND_EDGES)
	{
		F[0] = L.planes[e];
		if (!L.fold) return true;
		const uint64_t m = L.mirror[e];
		if (m >= L.entries) return true;       // (no mirror slot)
		if (m < e) return false;
		if (m != e) F[0] += L.planes[m];
		return true;
	}
	const uint32_t K = L.nPlanes;
	if (!L.fold)
	{
		F[0] = L.planes[e];
		if (K == 8) for (uint32_t p = 1; p < 8; p++) F[p] = L.planes[(uint64_t)p * L.entries + e];
		return true;
	}
	// the nodes that meet the round, in order, from node0 on
	const uint64_t rEnd = r0 + 64;
	uint32_t word = GA_FOLD_NONE;
	uint64_t start = 0, len = 0;
	for (uint32_t k = 0, nd = node0; k < 64 && nd < L.n_nodes; k++, nd++)
	{
		const uint64_t s = L.node_start[nd], t = L.node_start[nd + 1];
		if (s >= rEnd) break;
		if (e >= s && e < t) { word = L.fold_table[nd]; start = s; len = t - s; }
	}
	const uint32_t twin = word & GA_FOLD_NONE;
	if (!(word & GA_FOLD_FORWARD) || twin >= L.n_nodes) return false;
	const uint64_t c2 = L.node_start[twin] + (len - 1 - (e - start));
	if (c2 >= L.entries) return false;
	F[0] = L.planes[e] + L.planes[c2];
	if (K == 8)
	{
		for (uint32_t p = 1; p <= 4; p++) F[p] = L.planes[(uint64_t)p * L.entries + e] + L.planes[(uint64_t)(5 - p) * L.entries + c2];
		for (uint32_t p = 5; p < 8; p++) F[p] = L.planes[(uint64_t)p * L.entries + e] + L.planes[(uint64_t)p * L.entries + c2];
	}
	return true;
}

GAO_FN bool passes(const SitesLaunch& L, const uint32_t F[8])
{
	uint64_t D = F[0], X = 0;
	if (L.kind == KIND_BASES)
	{
		for (int p = 1; p < 7; p++) D += F[p];
		X = D - F[0];
		if (F[7] > X) X = F[7];
	}
	return D >= L.min_depth && X >= L.min_alt && X * L.alt_den >= (uint64_t)L.alt_num * D;
}

// the node of the next round's first column, from the node of this round's (at most 64 nodes start inside a round)
GAO_FN uint32_t advance(const SitesLaunch& L, uint32_t node, uint64_t rEnd)
{
	for (uint32_t k = 0; k < 64 && node + 1 < L.n_nodes && L.node_start[node + 1] <= rEnd; k++) node++;
	return node;
}

// one wave's share of the marking launch
GAO_FN void mark_wave(const SitesLaunch& L, SitesLds& lds, uint32_t wave, uint32_t nWaves)
{
	const bool nodes = L.fold && L.kind != KIND_EDGES;
	for (uint64_t tile = wave; tile < L.n_tiles; tile += nWaves)
	{
		const uint64_t t0 = L.first + tile * kTile, end = L.first + L.n;
		uint32_t node = nodes ? node_of(L, t0) : 0;
		uint32_t count = 0;
		for (uint32_t r = 0; r < kRounds; r++)
		{
			const uint64_t r0 = t0 + (uint64_t)r * 64;
			uint64_t m = 0;
			if (r0 < end)
			{
				GAO_LANES(l)
				{
					const uint64_t e = r0 + (uint64_t)l;
					uint32_t F[8];
					lds.flag[l] = e < end && fold_entry(L, e, r0, node, F) && passes(L, F) ? 1 : 0;
				}
				gao::sync();
				m = gao::ballot(lds.flag);
				gao::sync();                                         // (the flags are written again in the next round)
				if (nodes && r0 + 64 < end) node = advance(L, node, r0 + 64);
			}
			GAO_LANES(l) { if (l == 0) L.mask[tile * kRounds + r] = m; }
			count += gao::popc(m);
		}
		GAO_LANES(l) { if (l == 0) L.counts[tile] = count; }
	}
}

// one wave's share of the writing launch
GAO_FN void write_wave(const SitesLaunch& L, uint32_t wave, uint32_t nWaves)
{
	const bool nodes = L.fold && L.kind != KIND_EDGES;
	for (uint64_t tile = wave; tile < L.n_tiles; tile += nWaves)
	{
		const uint64_t t0 = L.first + tile * kTile;
		uint64_t at = L.offsets[tile];
		if (at >= L.n_recs) continue;                              // (the tile's places all lie behind the cap)
		for (uint32_t r = 0; r < kRounds; r++)
		{
			const uint64_t m = L.mask[tile * kRounds + r];
			if (!m) continue;
			const uint64_t r0 = t0 + (uint64_t)r * 64;
			const uint32_t node = nodes ? node_of(L, r0) : 0;
			GAO_LANES(l)
			{
				if ((m >> l) & 1)
				{
					const uint64_t idx = at + gao::popc(m & ((1ull << l) - 1));
					if (idx < L.n_recs)
					{
						const uint64_t e = r0 + (uint64_t)l;
						uint32_t F[8];
						(void)fold_entry(L, e, r0, node, F);
						GaSiteRec rec;
						rec.entry = e;
						for (int p = 0; p < 8; p++) rec.counts[p] = F[p];
						L.recs[idx] = rec;
					}
				}
			}
			at += gao::popc(m);
		}
	}
}

}  // namespace gast
