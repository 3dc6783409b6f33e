// ga_seed.h -- seeds found on the device: the k-mer index of the uploaded graph and, per read, the lookup of its k-mers and the
// ranking of the hits (include/graphaligner_amd.h states the rule; DESIGN.md section 10 argues it).
//
// One wave (= one workgroup of 64 lanes) works on one read at a time.  The program is written in PHASES: inside GAS_LANES(l) { ... }
// every lane runs the block for its own l, and lanes exchange values only through the SeedLds block (LDS) or the wave's hit buffer
// (HBM) with a wave_sync() between the phase that writes and the phase that reads; everything declared outside a lane block is the
// same in every lane (it is derived from such exchanged values), so the control flow around the blocks is uniform.  On gfx950 a lane
// block is straight-line code of the lane; in the host build of the tests (tests/emul) it is a loop over the 64 lanes, which is
// the same program because of that discipline.  The one wave primitive that is not a lane block is the exclusive scan of the tile's
// hit counts (cross-lane DPP/permute moves on the device, a running sum on the host).
//
// Two indexes: the in-node one (a k-mer lies inside one node; nodes shorter than k contribute nothing) and the walk index, which adds
// the k-mers of walks that leave a node through its out-edges ("index build with walks" below).  The lookup reads either.
#pragma once
#include "ga_types.h"
#ifndef GA_WAVE_HEADER
#define GA_WAVE_HEADER "ga_wave.h"
#endif
#include GA_WAVE_HEADER

namespace gas {

#ifdef GA_EMULATE
#define GAS_FN inline
#define GAS_HOST_FN inline
#define GAS_LANES(l) for (int l = 0; l < 64; l++)
#else
#define GAS_FN __device__ __forceinline__
#define GAS_HOST_FN __host__ __device__ inline                 // what the engine's host code calls too
#define GAS_LANES(l) if (const int l = (int)threadIdx.x; true)
#endif

constexpr uint32_t kMinArm = 193;          // a direction shorter than this asserts in the reference's engine (GraphAligner.h:906)
constexpr uint32_t kSeg = 4096;            // read positions whose bases are held 2 bits each in LDS at a time
constexpr uint32_t kSegWords = kSeg / 16 + 2;   // + the k - 1 <= 30 bases behind the segment's last position (a key spans up to three words)

struct SeedIndex
{
	uint32_t k, sample_shift;
	uint32_t dir_shift;                    // bucket of a key = key >> dir_shift (its top bits)
	uint32_t n_entries;
	const uint64_t* keys;                  // [n_entries] ascending; equal keys in (node, offset) order
	const uint64_t* vals;                  // [n_entries] node index << 32 | offset
	const uint32_t* dir;                   // [buckets + 1] first entry of each bucket
	const int64_t* linx;                   // [n_nodes] 2 * linear coordinate of the node's first base + strand flag
};

struct SeedRead { uint64_t off; uint32_t len, reserved; };      // off: multiple of 16; at least 16 bytes of padding follow the read

struct SeedLaunch
{
	SeedIndex ix;
	GaSeedParams p;
	const uint8_t* seq;
	const SeedRead* reads;
	const uint32_t* order;                 // read numbers, longest read first
	uint32_t n_reads, reserved;
	// per wave slot, max_hits entries each: read position, node index, 2 * diag + strand, support (0: not a candidate)
	uint32_t* hit_p; uint32_t* hit_node; int64_t* hit_dx; uint32_t* hit_sup;
	uint32_t* out_n;                       // [n_reads][3] seeds, hits used, truncated
	uint32_t* out_seed;                    // [n_reads][max_seeds][3] node index, read position, support
	// seeds per locus (seed_wave_loci) only; null for seed_wave.  Per wave slot, max_hits entries each: the hit's label (in the end the
	// smallest hit number of its locus), a second label buffer (in the end the locus' size, at its smallest hit), the locus' largest hit
	// number (there too), the ends of the hit's window run (first | last << 16) and the locus' best candidate (support << 32 | ~hit
	// number, there too; 0: none); how many hits the hit is linked to, itself included, 3 for more (<< 16), and for 2 the other one
	uint32_t* loc_lab; uint32_t* loc_alt; uint32_t* loc_last; uint32_t* loc_run; uint64_t* loc_best; uint32_t* loc_nbr;
	uint32_t* out_locus;                   // [n_reads][max_seeds][3] hits of the seed's locus, its smallest and its largest read position
	uint32_t* out_nloci;                   // [n_reads] loci that have a candidate
};

struct SeedLds
{
	uint32_t code[kSegWords + 1], inval[kSegWords + 1];    // 16 bases / 16 "not ACGT" flags per word, first base in the top bits
	uint32_t cnt[64], tot;
	uint32_t bestSup[64], bestIdx[64];
	int64_t taken[64];                                     // 2 * diag + strand of the seeds taken so far
};
struct SeedLdsLoci : SeedLds { uint64_t bestKey[64]; };   // seeds per locus: a lane's best locus of the round (its size goes to bestSup)

GAS_FN uint32_t mix64(uint64_t x) { x ^= x >> 29; x *= 0x9e3779b97f4a7c15ull; x ^= x >> 32; return (uint32_t)x; }
GAS_FN bool kept(uint64_t key, uint32_t sampleShift) { return (mix64(key) & ((1u << sampleShift) - 1u)) == 0; }
GAS_FN int64_t absdiff(int64_t a, int64_t b) { return a < b ? b - a : a - b; }

// ---- index build ---------------------------------------------------------------------------------------------------------------
// the kept k-mers of one node in offset order (the key rolls along the node: one base per step); returns their number
template <class F> GAS_FN uint64_t node_kmers(const GaDevGraph& g, uint32_t node, uint32_t k, uint32_t sampleShift, F emit)
{
	if (node == 0 || node + 1 >= g.n_nodes) return 0;                    // the two dummy nodes
	const uint64_t start = g.node_start[node], len = g.node_start[node + 1] - start;
	if (len < k) return 0;
	const uint64_t mask = (1ull << (2 * k)) - 1;
	uint64_t key = 0, n = 0;
	uint32_t w = g.seq2[start >> 4];
	for (uint64_t i = 0; i < len; i++)
	{
		const uint64_t col = start + i;
		if ((col & 15) == 0) w = g.seq2[col >> 4];
		key = ((key << 2) | ((w >> ((col & 15) * 2)) & 3u)) & mask;
		if (i + 1 >= k && kept(key, sampleShift)) { emit(key, (uint32_t)(i + 1 - k)); n++; }
	}
	return n;
}
GAS_FN void index_count(const GaDevGraph& g, uint32_t node, uint32_t k, uint32_t sampleShift, uint64_t* counts)
{
	counts[node] = node_kmers(g, node, k, sampleShift, [](uint64_t, uint32_t) {});
}
GAS_FN void index_write(const GaDevGraph& g, uint32_t node, uint32_t k, uint32_t sampleShift, const uint64_t* firstEntry, uint64_t* keys, uint64_t* vals)
{
	uint64_t at = firstEntry[node];
	node_kmers(g, node, k, sampleShift, [&](uint64_t key, uint32_t o) { keys[at] = key; vals[at] = ((uint64_t)node << 32) | o; at++; });
}
// ---- index build with walks: k-mers that leave a node through its out-edges -----------------------------------------------------
// A start (node, o) with o + k > len ("tail start") has one k-mer per walk that begins with the node's bases from o and goes on through
// out-neighbours until k bases are read; every one is attributed to (node, o).  The walks of one start are enumerated depth first.
// The stack of the enumeration (per level: next out-edge, end of the out-edges, bases read when the level was entered) is indexed by
// the depth at run time, so it lives in LDS, lane-minor (level d of lane l at [d][l]: the 64 lanes of a wave hit 64 banks); a level
// adds at least one base and the last node of a walk is not pushed, so k - 1 <= 30 levels are enough.
constexpr uint32_t kWalkLevels = 30;
struct WalkStack { uint32_t cur[kWalkLevels][64], end[kWalkLevels][64], have[kWalkLevels][64]; };
struct WalkTally { uint64_t tail_starts, skipped, walks; };       // of one lane: tail starts, those over max_walks, walks of the others

// `cnt` <= 31 bases from column `col` on, shifted into `key` (first base most significant)
GAS_FN uint64_t append_bases(const GaDevGraph& g, uint64_t key, uint64_t col, uint32_t cnt)
{
	for (uint32_t i = 0; i < cnt; i++, col++) key = (key << 2) | ((g.seq2[col >> 4] >> ((col & 15) * 2)) & 3u);
	return key;
}
// the walks of the tail start whose own `have` bases are `prefix`: emit(key) per walk in depth-first order; returns their number, or
// maxWalks + 1 as soon as there are more (what was emitted until then is not to be used: the caller counts first).  A walk does not
// enter a dummy node or a node of length 0, and one that cannot go on before k bases gives nothing.
template <class F> GAS_FN uint32_t start_walks(const GaDevGraph& g, uint32_t node, uint64_t prefix, uint32_t have, uint32_t k, uint32_t maxWalks, WalkStack& st, int lane, F emit)
{
	uint64_t key = prefix;
	uint32_t inKey = have, walks = 0;
	int d = 0;
	st.cur[0][lane] = g.out_off[node]; st.end[0][lane] = g.out_off[node + 1]; st.have[0][lane] = have;
	while (d >= 0)
	{
		const uint32_t e = st.cur[d][lane];
		if (e == st.end[d][lane]) { d--; continue; }
		st.cur[d][lane] = e + 1;
		const uint32_t m = g.out_nbr[e];
		if (m == 0 || m + 1 >= g.n_nodes) continue;
		const uint64_t mStart = g.node_start[m], mLen = g.node_start[m + 1] - mStart;
		if (mLen == 0) continue;
		const uint32_t h = st.have[d][lane], need = k - h;
		key >>= 2 * (inKey - h);                                           // back to the bases read when this level was entered
		inKey = h;
		if (mLen >= need)
		{
			if (++walks > maxWalks) return walks;
			emit(append_bases(g, key, mStart, need));
		}
		else
		{
			key = append_bases(g, key, mStart, (uint32_t)mLen);
			inKey = h + (uint32_t)mLen;
			d++;
			st.cur[d][lane] = g.out_off[m]; st.end[d][lane] = g.out_off[m + 1]; st.have[d][lane] = inKey;
		}
	}
	return walks;
}
// the kept k-mers of one node's starts in offset order: the in-node ones as node_kmers gives them, then the tail starts'; returns
// their number (equal (key, offset) pairs of one start's walks are all emitted: they are dropped after the sort)
template <class F> GAS_FN uint64_t node_walk_kmers(const GaDevGraph& g, uint32_t node, uint32_t k, uint32_t sampleShift, uint32_t maxWalks, WalkStack& st, int lane, WalkTally& tally, F emit)
{
	if (node == 0 || node + 1 >= g.n_nodes) return 0;
	uint64_t n = node_kmers(g, node, k, sampleShift, emit);
	const uint64_t start = g.node_start[node], len = g.node_start[node + 1] - start;
	const uint32_t tail = len < k ? (uint32_t)len : k - 1;                  // the last `tail` offsets are tail starts
	const uint64_t tkey = append_bases(g, 0, start + len - tail, tail);
	for (uint32_t have = tail; have >= 1; have--)
	{
		const uint32_t o = (uint32_t)(len - have);
		const uint64_t prefix = tkey & ((1ull << (2 * have)) - 1);
		tally.tail_starts++;
		const uint32_t walks = start_walks(g, node, prefix, have, k, maxWalks, st, lane, [](uint64_t) {});
		if (walks > maxWalks) { tally.skipped++; continue; }
		if (walks == 0) continue;
		tally.walks += walks;
		start_walks(g, node, prefix, have, k, maxWalks, st, lane, [&](uint64_t key) { if (kept(key, sampleShift)) { emit(key, o); n++; } });
	}
	return n;
}
GAS_FN void walk_index_count(const GaDevGraph& g, uint32_t node, uint32_t k, uint32_t sampleShift, uint32_t maxWalks, WalkStack& st, int lane, WalkTally& tally, uint64_t* counts)
{
	counts[node] = node_walk_kmers(g, node, k, sampleShift, maxWalks, st, lane, tally, [](uint64_t, uint32_t) {});
}
GAS_FN void walk_index_write(const GaDevGraph& g, uint32_t node, uint32_t k, uint32_t sampleShift, uint32_t maxWalks, WalkStack& st, int lane, const uint64_t* firstEntry, uint64_t* keys, uint64_t* vals)
{
	uint64_t at = firstEntry[node];
	WalkTally unused{0, 0, 0};
	node_walk_kmers(g, node, k, sampleShift, maxWalks, st, lane, unused, [&](uint64_t key, uint32_t o) { keys[at] = key; vals[at] = ((uint64_t)node << 32) | o; at++; });
}
// after the stable sort equal (key, node, offset) triples are neighbours: entry i stays when it differs from entry i - 1
GAS_FN uint32_t index_first_of_its_kind(const uint64_t* keys, const uint64_t* vals, uint32_t i)
{
	return (i == 0 || keys[i] != keys[i - 1] || vals[i] != vals[i - 1]) ? 1u : 0u;
}

// entry i (i = n: the end) names itself as the first entry of every bucket between its predecessor's and its own
GAS_FN void index_dir(const uint64_t* keys, uint32_t n, uint32_t dirShift, uint32_t buckets, uint32_t* dir, uint32_t i)
{
	const uint64_t lo = i == 0 ? 0 : (keys[i - 1] >> dirShift) + 1;
	const uint64_t hi = i == n ? buckets : (keys[i] >> dirShift);
	for (uint64_t b = lo; b <= hi; b++) dir[b] = i;
}

// ---- lookup --------------------------------------------------------------------------------------------------------------------
// entries of `key`: one directory load, a search inside the bucket (about one entry per bucket by the choice of dir_shift), then a
// walk over at most maxOcc + 1 equal keys
GAS_FN uint32_t lookup(const SeedIndex& ix, uint64_t key, uint32_t maxOcc, uint32_t& first)
{
	const uint64_t b = key >> ix.dir_shift;
	uint32_t lo = ix.dir[b];
	const uint32_t end = ix.dir[b + 1];
	first = lo;
	if (end > ix.n_entries || lo > end) return 0;                          // (never with a directory built by index_dir: keeps every loop here bounded)
	uint32_t hi = end;
	while (hi - lo > 4) { const uint32_t mid = lo + ((hi - lo) >> 1); if (ix.keys[mid] < key) lo = mid + 1; else hi = mid; }
	while (lo < end && ix.keys[lo] < key) lo++;
	uint32_t occ = 0;
	while (lo + occ < end && occ <= maxOcc && ix.keys[lo + occ] == key) occ++;
	first = lo;
	return occ;
}

// exclusive scan of lds.cnt over the lanes, total into lds.tot (the caller syncs before and after)
GAS_FN void scan_counts(SeedLds& lds)
{
#ifdef GA_EMULATE
	uint32_t run = 0;
	for (int l = 0; l < 64; l++) { const uint32_t c = lds.cnt[l]; lds.cnt[l] = run; run += c; }
	lds.tot = run;
#else
	const int l = (int)threadIdx.x;
	const uint32_t own = lds.cnt[l];
	uint32_t v = own;
	for (int d = 1; d < 64; d <<= 1) { const uint32_t o = (uint32_t)__shfl_up((int)v, d, 64); if (l >= d) v += o; }
	lds.cnt[l] = v - own;
	if (l == 63) lds.tot = v;
#endif
}

// sixteen characters -> their 2-bit codes and "not one of ACGT" flags, first character in the top bits
GAS_FN void pack16(const uint8_t* p, uint32_t nValid, uint32_t& code, uint32_t& inval)
{
	code = 0; inval = 0xffffu;
	if (nValid == 0) return;
	const uint32_t* q = (const uint32_t*)p;                                // (16-byte aligned, padded: SeedRead)
	const uint32_t w[4] = {q[0], q[1], q[2], q[3]};
#pragma unroll
	for (uint32_t i = 0; i < 16; i++)
	{
		const uint32_t c = (w[i >> 2] >> ((i & 3) * 8)) & 0xffu;
		const bool ok = i < nValid && (c == 'A' || c == 'C' || c == 'G' || c == 'T');
		if (ok) { code |= (((c >> 1) ^ (c >> 2)) & 3u) << (30 - 2 * i); inval &= ~(1u << (15 - i)); }
	}
}

// ---- one read, in three phases: its hits into the wave's hit buffer, their support, the choice ------------------------------------
// what the first phase leaves for the others: the slot's part of the hit buffer, the number of hits, the read's length
struct ReadHits { uint32_t* p; uint32_t* node; int64_t* dx; uint32_t* sup; uint32_t n, len; bool truncated; };
// the slot's part of the buffers of seeds per locus (SeedLaunch)
struct LociBuf { uint32_t* lab; uint32_t* alt; uint32_t* last; uint32_t* run; uint64_t* best; uint32_t* nbr; };

// Values that several lanes add to or raise in one phase (size, largest hit number and best candidate of a locus, kept at the locus'
// smallest hit): integer add and max, so the result does not depend on the order.  On gfx950 they are device-scope atomics, which
// are served by L2; they are set and read back by device-scope stores and loads, which do not stop at the CU's first-level cache (a
// plain load could find a line there from before the atomics).  On the host they are the plain operations.
// INVARIANT: between the acc_set of an entry and the end of the read, that entry of `size` (the second label buffer), `last` and `best`
// is touched by acc_* alone, never by a plain load or store.  The label buffers are used with plain stores and loads again by the
// next read of the slot; that is sound because every label entry below the read's hit count is written by a plain store (read_support,
// then every compress and hook step writes the whole buffer) before any plain load reads it, the order the hit buffer itself relies on.
#ifdef GA_EMULATE
template <class T> GAS_FN void acc_set(T* p, T v) { *p = v; }
template <class T> GAS_FN T acc_get(const T* p) { return *p; }
template <class T> GAS_FN void acc_add(T* p, T v) { *p += v; }
template <class T> GAS_FN void acc_max(T* p, T v) { if (v > *p) *p = v; }
#else
template <class T> GAS_FN void acc_set(T* p, T v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <class T> GAS_FN T acc_get(const T* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <class T> GAS_FN void acc_add(T* p, T v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <class T> GAS_FN void acc_max(T* p, T v) { __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
#endif

// phase 1: the hits of the read, in (p, index order) order, into the slot's hit buffer (p, node, 2 * diag + strand)
GAS_FN ReadHits read_hits(const SeedLaunch& L, SeedLds& lds, uint32_t slot, uint32_t read)
{
	const SeedIndex& ix = L.ix;
	const GaSeedParams& P = L.p;
	const SeedRead rd = L.reads[read];
	const uint8_t* seq = L.seq + rd.off;
	const uint32_t len = rd.len, k = ix.k;
	uint32_t* hitP = L.hit_p + (uint64_t)slot * P.max_hits;
	uint32_t* hitNode = L.hit_node + (uint64_t)slot * P.max_hits;
	int64_t* hitDx = L.hit_dx + (uint64_t)slot * P.max_hits;
	uint32_t* hitSup = L.hit_sup + (uint64_t)slot * P.max_hits;
	const uint32_t nPos = len >= k ? len - k + 1 : 0;                      // read positions that start a k-mer
	uint32_t total = 0;
	bool truncated = false;

	for (uint32_t s0 = 0; s0 < nPos && !truncated; s0 += kSeg)
	{
		gaw::wave_sync();                                                    // (the previous segment's words are no longer read)
		GAS_LANES(l)
		{
			for (uint32_t w = (uint32_t)l; w < kSegWords + 1; w += 64)
			{
				const uint64_t at = (uint64_t)s0 + 16ull * w;
				uint32_t c, iv;
				pack16(seq + at, at < len ? (len - at < 16 ? (uint32_t)(len - at) : 16u) : 0u, c, iv);
				lds.code[w] = c; lds.inval[w] = iv;
			}
		}
		gaw::wave_sync();
		for (uint32_t t0 = 0; t0 < kSeg && s0 + t0 < nPos && !truncated; t0 += 64)
		{
			GAS_LANES(l)
			{
				const uint32_t q = t0 + (uint32_t)l, p = s0 + q;
				uint32_t c = 0;
				if (p < nPos)
				{
					const uint32_t j = q >> 4, sh = q & 15;
					const uint64_t iv = ((uint64_t)lds.inval[j] << 32) | ((uint64_t)lds.inval[j + 1] << 16) | lds.inval[j + 2];
					const bool bad = (((iv << sh) & 0xffffffffffffull) >> (48 - k)) != 0;
					const uint64_t hi = ((uint64_t)lds.code[j] << 32) | lds.code[j + 1];
					const uint64_t x = sh ? (hi << (2 * sh)) | ((uint64_t)lds.code[j + 2] >> (32 - 2 * sh)) : hi;
					const uint64_t key = x >> (64 - 2 * k);
					if (!bad && kept(key, ix.sample_shift))                      // (the kept test comes before any index access)
					{
						uint32_t first;
						const uint32_t occ = lookup(ix, key, P.max_occ, first);
						if (occ >= 1 && occ <= P.max_occ) { c = occ; lds.bestIdx[l] = first; }
					}
				}
				lds.cnt[l] = c;
			}
			gaw::wave_sync();
			scan_counts(lds);
			gaw::wave_sync();
			GAS_LANES(l)
			{
				// hits leave in (p, index order) order: lane order is position order, a lane's entries are in index order
				const uint32_t p = s0 + t0 + (uint32_t)l;
				const uint32_t n = (l == 63 ? lds.tot : lds.cnt[l + 1]) - lds.cnt[l];
				const uint32_t first = lds.bestIdx[l];
				for (uint32_t e = 0; e < n; e++)
				{
					const uint32_t at = total + lds.cnt[l] + e;
					if (at >= P.max_hits) break;
					const uint64_t v = ix.vals[first + e];
					const uint32_t node = (uint32_t)(v >> 32);
					const int64_t lx = ix.linx[node];
					const int64_t diag = (lx >> 1) + (int64_t)(uint32_t)v - (int64_t)p;
					hitP[at] = p; hitNode[at] = node; hitDx[at] = diag * 2 + (lx & 1);
				}
			}
			total += lds.tot;
			if (total > P.max_hits) { total = P.max_hits; truncated = true; }
			gaw::wave_sync();                                                // (lds.tot is read before the next tile writes it)
		}
	}
	gaw::wave_sync();                                                        // the hit buffer is complete and visible to every lane
	return ReadHits{hitP, hitNode, hitDx, hitSup, total, len, truncated};
}

// phase 2: support of every hit (0 when it is no candidate).  kLoci: also the hit's first label, the smallest hit number among the
// hits it is linked to (the relation support counts; itself included), the ends of its run, for the later passes over it, and how
// many hits it is linked to: the relation does not change, so a hit linked to none but itself keeps its label for good, and one linked
// to a single other hit needs that hit's label and no pass over the run (chance hits are of these two kinds)
template <bool kLoci> GAS_FN void read_support(const GaSeedParams& P, const ReadHits& h, const LociBuf& b)
{
	const uint32_t* hitP = h.p;
	const int64_t* hitDx = h.dx;
	uint32_t* hitSup = h.sup;
	const uint32_t len = h.len;
	// support: hits are in p order, so the hits within `window` of one are a run around it.  Its two ends come from binary searches;
	// the count over the run then has no exit that depends on a loaded value, so its loads are in flight together (a walk outwards
	// that stops at the first hit outside the window waits for every load in turn: 18.1 ms against 13.6 ms for the benchmark's batch)
	const uint32_t H = h.n;
	GAS_LANES(l)
	{
		for (uint32_t i = (uint32_t)l; i < H; i += 64)
		{
			const uint32_t p = hitP[i];
			const int64_t dx = hitDx[i];
			uint32_t lo = 0, hi = i;
			while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (p - hitP[mid] > P.window) lo = mid + 1; else hi = mid; }
			const uint32_t from = lo;
			lo = i + 1; hi = H;
			while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (hitP[mid] - p <= P.window) lo = mid + 1; else hi = mid; }
			uint32_t sup = 0, first = i, last = i;
#pragma unroll 4
			for (uint32_t j = from; j < lo; j++)
			{
				const int64_t o = hitDx[j];
				const bool linked = ((o ^ dx) & 1) == 0 && absdiff(o >> 1, dx >> 1) <= (int64_t)P.diag_tol;
				sup += linked ? 1u : 0u;                                         // (j = i counts: the hit itself)
				if constexpr (kLoci) { first = linked && j < first ? j : first; last = linked ? j : last; }
			}
			const bool cand = p >= kMinArm && len - p >= kMinArm && sup >= P.min_support;
			hitSup[i] = cand ? sup : 0u;
			if constexpr (kLoci)
			{
				b.lab[i] = first; b.run[i] = from | ((lo - 1) << 16);              // (hit numbers are below 65 536 = the largest max_hits)
				b.nbr[i] = (first < i ? first : last) | ((sup < 3 ? sup : 3u) << 16);
			}
		}
	}
	gaw::wave_sync();
}

// phase 3, hit by hit: per round every lane names its best remaining candidate (highest support, then lowest hit number = (p, node,
// offset) order), the wave takes the best of those
GAS_FN void read_choice(const SeedLaunch& L, SeedLds& lds, const ReadHits& h, uint32_t read)
{
	const GaSeedParams& P = L.p;
	const uint32_t* hitP = h.p;
	const uint32_t* hitNode = h.node;
	const int64_t* hitDx = h.dx;
	const uint32_t* hitSup = h.sup;
	const uint32_t H = h.n;
	const bool truncated = h.truncated;
	uint32_t nSeeds = 0;
	for (uint32_t r = 0; r < P.max_seeds; r++)
	{
		GAS_LANES(l)
		{
			uint32_t bs = 0, bi = 0xffffffffu;
			for (uint32_t i = (uint32_t)l; i < H; i += 64)
			{
				const uint32_t s = hitSup[i];
				if (s <= bs) continue;
				const int64_t dx = hitDx[i];
				bool same = false;
				for (uint32_t t = 0; t < r; t++)
				{
					const int64_t o = lds.taken[t];
					if (((o ^ dx) & 1) == 0 && absdiff(o >> 1, dx >> 1) <= (int64_t)P.diag_tol) same = true;
				}
				if (!same) { bs = s; bi = i; }
			}
			lds.bestSup[l] = bs; lds.bestIdx[l] = bi;
		}
		gaw::wave_sync();
		uint32_t bs = 0, bi = 0xffffffffu;
		for (int l = 0; l < 64; l++)
		{
			const uint32_t s = lds.bestSup[l], i = lds.bestIdx[l];
			if (s > bs || (s == bs && s != 0 && i < bi)) { bs = s; bi = i; }
		}
		gaw::wave_sync();                                                    // (everyone has read the round's table)
		if (bs == 0) break;
		GAS_LANES(l)
		{
			if (l == 0)
			{
				lds.taken[r] = hitDx[bi];
				uint32_t* o = L.out_seed + ((uint64_t)read * P.max_seeds + r) * 3;
				o[0] = hitNode[bi]; o[1] = hitP[bi]; o[2] = bs;
			}
		}
		nSeeds++;
		gaw::wave_sync();
	}
	GAS_LANES(l)
	{
		if (l == 0) { uint32_t* o = L.out_n + (uint64_t)read * 3; o[0] = nSeeds; o[1] = H; o[2] = truncated ? 1u : 0u; }
	}
}

// one read: its hits into the wave's hit buffer, their support, the greedy choice
GAS_FN void seed_read(const SeedLaunch& L, SeedLds& lds, uint32_t slot, uint32_t read)
{
	const ReadHits h = read_hits(L, lds, slot, read);
	read_support<false>(L.p, h, LociBuf{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr});
	read_choice(L, lds, h, read);
}

// ---- seeds per locus -----------------------------------------------------------------------------------------------------------
// A locus is a connected component of the link relation over the read's hits (include/graphaligner_amd.h has the rule).  Labels: every
// hit ends up with the smallest hit number of its component.  Two kinds of step, each reading one label buffer and writing the other
// with a wave_sync between (so a step is a function of the labels before it, on the device as on the host):
//   hook      label'[i] = the smallest label among the hits linked to i (itself included); the first hook, over label[i] = i, is done by
//             read_support<true> inside the support scan
//   compress  label'[i] = the end of the chain label[i], label[label[i]], ... (a label is a hit number of the same component and <= i,
//             so the labels are pointers towards the component's smallest hit), followed for at most 16 steps; repeated while some
//             chain was longer (4 passes follow any chain of 65 536 hits; after the first hook a chain has about one step per
//             `window` of read, so one pass is the rule)
// until a hook changes nothing: then linked hits have equal labels, so a component has one label, which is one of its hit numbers and
// <= its smallest.  Labels only fall and every hook carries the smallest number one link further, so H hooks always suffice: both
// loops have a count as their bound, and their other exit is read by every lane from LDS after a wave_sync.
GAS_FN bool any_lane(const SeedLds& lds)
{
	uint32_t v = 0;
	for (int l = 0; l < 64; l++) v |= lds.cnt[l];
	return v != 0;
}

GAS_FN void seed_read_loci(const SeedLaunch& L, SeedLdsLoci& lds, uint32_t slot, uint32_t read)
{
	const GaSeedParams& P = L.p;
	const ReadHits h = read_hits(L, lds, slot, read);
	const uint64_t base = (uint64_t)slot * P.max_hits;
	const LociBuf b{L.loc_lab + base, L.loc_alt + base, L.loc_last + base, L.loc_run + base, L.loc_best + base, L.loc_nbr + base};
	read_support<true>(P, h, b);
	const uint32_t H = h.n;
	uint32_t* a = b.lab;                                                     // the labels as they stand
	uint32_t* o = b.alt;                                                     // where the next step writes
	bool changed = true;
	for (uint32_t round = 0; round < H && changed; round++)
	{
		bool moving = true;
		for (uint32_t c = 0; c < 5 && moving; c++)
		{
			GAS_LANES(l)
			{
				uint32_t mv = 0;
				for (uint32_t i = (uint32_t)l; i < H; i += 64)
				{
					uint32_t v = a[i], w = a[v];
					for (uint32_t t = 0; t < 16 && w != v; t++) { v = w; w = a[v]; }
					o[i] = w;
					mv |= v ^ w;                                                   // (not at the chain's end yet)
				}
				lds.cnt[l] = mv;
			}
			gaw::wave_sync();
			moving = any_lane(lds);
			gaw::wave_sync();
			uint32_t* t = a; a = o; o = t;
		}
		GAS_LANES(l)
		{
			uint32_t ch = 0;
			for (uint32_t i = (uint32_t)l; i < H; i += 64)
			{
				const uint32_t own = a[i], nbr = b.nbr[i], links = nbr >> 16;
				uint32_t m = own;
				if (links == 2)
				{
					const uint32_t v = a[nbr & 0xffffu];
					m = v < own ? v : own;
				}
				else if (links > 2)
				{
					// the smallest label in the run, linked or not: labels are equal all over a locus once it is compressed, so it
					// is rarely lower than the hit's own, and only then are the diagonals looked at
					const uint32_t run = b.run[i], from = run & 0xffffu, to = run >> 16;
					uint32_t low = own;
#pragma unroll 8
					for (uint32_t j = from; j <= to; j++) { const uint32_t v = a[j]; low = v < low ? v : low; }
					if (low < own)
					{
						const int64_t dx = h.dx[i];
#pragma unroll 4
						for (uint32_t j = from; j <= to; j++)
						{
							const uint32_t v = a[j];
							const int64_t x = h.dx[j];
							if (v < m && ((x ^ dx) & 1) == 0 && absdiff(x >> 1, dx >> 1) <= (int64_t)P.diag_tol) m = v;
						}
					}
				}
				o[i] = m;
				ch |= m ^ own;
			}
			lds.cnt[l] = ch;
		}
		gaw::wave_sync();
		changed = any_lane(lds);
		gaw::wave_sync();
		uint32_t* t = a; a = o; o = t;
	}

	// (the sums below rely on changed == false here: `a` is then a compressed buffer that the last hook left as it was, so a[r] == r
	// names one hit per locus; leaving through round == H cannot happen before that, by the argument above)
	// per locus, at its smallest hit r (a[r] == r): size, largest hit number (= largest p: hits are in p order) and best candidate
	// (support << 32 | ~hit number: the larger value is the earlier one in the order of the choice).  A lane sums what its own hits
	// give to one locus before it adds it there.
	uint32_t* size = o;
	GAS_LANES(l)
	{
		for (uint32_t i = (uint32_t)l; i < H; i += 64)
			if (a[i] == i) { acc_set(size + i, 0u); acc_set(b.last + i, 0u); acc_set(b.best + i, (uint64_t)0); }
	}
	gaw::wave_sync();
	GAS_LANES(l)
	{
		uint32_t r0 = 0, n = 0, mx = 0;
		uint64_t bk = 0;
		for (uint32_t i = (uint32_t)l; i < H; i += 64)
		{
			const uint32_t r = a[i];
			if (n != 0 && r != r0)
			{
				acc_add(size + r0, n); acc_max(b.last + r0, mx);
				if (bk != 0) acc_max(b.best + r0, bk);
				n = 0; bk = 0;
			}
			r0 = r; n++; mx = i;
			const uint32_t s = h.sup[i];
			const uint64_t key = ((uint64_t)s << 32) | (0xffffffffu - i);
			if (s != 0 && key > bk) bk = key;
		}
		if (n != 0)
		{
			acc_add(size + r0, n); acc_max(b.last + r0, mx);
			if (bk != 0) acc_max(b.best + r0, bk);
		}
	}
	gaw::wave_sync();

	// the choice, locus by locus: per round every lane names its best remaining locus (most hits, then the earlier seed hit), the wave
	// takes the best of those; a locus whose seed hit lies within diag_tol of a taken seed hit (itself, once taken) is passed over
	uint32_t nSeeds = 0, nLoci = 0;
	for (uint32_t r = 0; r < P.max_seeds; r++)
	{
		GAS_LANES(l)
		{
			uint32_t bz = 0, roots = 0;
			uint64_t bk = 0;
			for (uint32_t i = (uint32_t)l; i < H; i += 64)
			{
				if (a[i] != i) continue;
				const uint64_t key = acc_get(b.best + i);
				if (key == 0) continue;
				roots++;
				const uint32_t z = acc_get(size + i);
				if (z < bz || (z == bz && key <= bk)) continue;
				const int64_t dx = h.dx[0xffffffffu - (uint32_t)key];
				bool same = false;
				for (uint32_t t = 0; t < r; t++)
				{
					const int64_t x = lds.taken[t];
					if (((x ^ dx) & 1) == 0 && absdiff(x >> 1, dx >> 1) <= (int64_t)P.diag_tol) same = true;
				}
				if (!same) { bz = z; bk = key; }
			}
			lds.bestSup[l] = bz; lds.bestKey[l] = bk; lds.cnt[l] = roots;
		}
		gaw::wave_sync();
		uint32_t bz = 0;
		uint64_t bk = 0;
		for (int l = 0; l < 64; l++)
		{
			const uint32_t z = lds.bestSup[l];
			const uint64_t key = lds.bestKey[l];
			if (z > bz || (z == bz && key > bk)) { bz = z; bk = key; }
			if (r == 0) nLoci += lds.cnt[l];
		}
		gaw::wave_sync();                                                    // (everyone has read the round's table)
		if (bz == 0) break;
		GAS_LANES(l)
		{
			if (l == 0)
			{
				const uint32_t bi = 0xffffffffu - (uint32_t)bk, root = a[bi];
				lds.taken[r] = h.dx[bi];
				uint32_t* s = L.out_seed + ((uint64_t)read * P.max_seeds + r) * 3;
				s[0] = h.node[bi]; s[1] = h.p[bi]; s[2] = (uint32_t)(bk >> 32);
				uint32_t* q = L.out_locus + ((uint64_t)read * P.max_seeds + r) * 3;
				q[0] = bz; q[1] = h.p[root]; q[2] = h.p[acc_get(b.last + root)];
			}
		}
		nSeeds++;
		gaw::wave_sync();
	}
	GAS_LANES(l)
	{
		if (l == 0)
		{
			uint32_t* q = L.out_n + (uint64_t)read * 3;
			q[0] = nSeeds; q[1] = H; q[2] = h.truncated ? 1u : 0u;
			L.out_nloci[read] = nLoci;
		}
	}
}

// a wave: the reads are dealt longest first, round-robin over the waves (read number slot, slot + slots, ... of that order), so every
// wave gets the same mix of lengths and the hand-out needs no counter: the loop is the same in every lane by construction
GAS_FN void seed_wave(const SeedLaunch& L, SeedLds& lds, uint32_t slot, uint32_t slots)
{
	for (uint32_t at = slot; at < L.n_reads; at += slots) seed_read(L, lds, slot, L.order[at]);
}
GAS_FN void seed_wave_loci(const SeedLaunch& L, SeedLdsLoci& lds, uint32_t slot, uint32_t slots)
{
	for (uint32_t at = slot; at < L.n_reads; at += slots) seed_read_loci(L, lds, slot, L.order[at]);
}

// ---- topology coordinate ---------------------------------------------------------------------------------------------------------
// The linear coordinate from the graph's edges instead of the order of the file (include/graphaligner_amd.h, "topology coordinate",
// has the rule; DESIGN.md section 10b argues it): every node hangs under the first usable entry of its in-list, the cycles of that
// relation are cut at their smallest node index, lin = the tree's base + the summed length of the node's ancestors.  One lane per
// node.  Every function below is one node's part of one launch: it reads the launch's input buffers, writes the node's own entry of
// the output buffer (coord_mark and coord_extent: an entry of another node, by a store of the constant 1 and by an integer max, so
// the order of the lanes does not show), and returns what the launch counts or ors together.  The loops over rounds are the host's.
// Work buffers, freed when the call ends, 68 bytes per node: two state buffers of 16 bytes (the cycle pass uses 8 of each), parent
// and its length 4 + 4, marks 4, extents 8, the scan's input and output 8 + 8.
constexpr uint32_t kCoordRoot = 0xffffffffu;       // "no parent": what the cycle pass calls the ancestor of a walk that has left its tree
constexpr int64_t kTreeGap = 1 << 20;              // GA_SEED_TREE_GAP
struct alignas(8) CoordCyc { uint32_t anc, low; };                  // ancestor 2^r steps up, smallest index among the 2^r nodes before it
struct alignas(16) CoordDepth { int64_t dist; uint32_t anc, reserved; };   // ancestor min(2^r, all) steps up (a root: itself), columns from its first to the node's first

GAS_FN bool coord_dummy(const GaDevGraph& g, uint32_t v) { return v == 0 || v + 1 >= g.n_nodes; }
GAS_HOST_FN uint32_t coord_rounds(uint32_t nNodes) { uint32_t r = 0; while ((1ull << r) < nNodes) r++; return r; }   // smallest R with 2^R >= n_nodes

// the parent: the first entry of the in-list that is neither the node itself nor a dummy node.  The node's record holds the first
// four entries and their lengths; a longer list is read itself
GAS_FN void coord_parent(const GaDevGraph& g, uint32_t v, uint32_t* par, uint32_t* parLen)
{
	uint32_t p = kCoordRoot, pl = 0;
	if (!coord_dummy(g, v))
	{
		const uint32_t* r = g.node_rec + (uint64_t)v * GA_NODE_REC_WORDS;
		const uint32_t inDeg = r[3] & 0xffffu;
		bool found = false;
		if (inDeg <= 4)
		{
#pragma unroll
			for (uint32_t k = 0; k < 4; k++)
			{
				const uint32_t u = r[8 + k], ul = r[12 + k];
				if (k < inDeg && !found && u != v && !coord_dummy(g, u)) { p = u; pl = ul; found = true; }
			}
		}
		else
		{
			const uint32_t end = g.in_off[v + 1];
			for (uint32_t e = g.in_off[v]; e < end && !found; e++)
			{
				const uint32_t u = g.in_nbr[e];
				if (u != v && !coord_dummy(g, u)) { p = u; pl = (uint32_t)(g.node_start[u + 1] - g.node_start[u]); found = true; }
			}
		}
	}
	par[v] = p; parLen[v] = pl;
}
// cycle pass.  After r rounds: anc = the node r' = 2^r parent steps up (kCoordRoot once the walk has passed a root), low = the smallest
// index among the node and the walk's nodes before anc.  Returns whether the node's walk is still inside the graph.
GAS_FN bool coord_cyc_init(const uint32_t* par, uint32_t v, CoordCyc* o)
{
	const uint32_t p = par[v];
	o[v] = CoordCyc{p, v};
	return p != kCoordRoot;
}
GAS_FN bool coord_cyc_round(const CoordCyc* a, CoordCyc* o, uint32_t v)
{
	CoordCyc s = a[v];
	if (s.anc != kCoordRoot)
	{
		const CoordCyc t = a[s.anc];
		s.anc = t.anc; s.low = t.low < s.low ? t.low : s.low;
	}
	o[v] = s;
	return s.anc != kCoordRoot;
}
// after R rounds with 2^R >= n_nodes a walk that is still inside the graph never ends: its node 2^R steps up lies on a cycle, and
// from the nodes of a cycle those are all its nodes (2^R steps turn the cycle onto itself).  For a node ON a cycle the 2^R nodes
// of its walk are the cycle's, so there `low` is the cycle's smallest index; for a node that leads into one, `low` may be its own
GAS_FN void coord_mark(const CoordCyc* a, uint32_t* mark, uint32_t v)
{
	const uint32_t t = a[v].anc;
	if (t != kCoordRoot) mark[t] = 1;
}
GAS_FN bool coord_cut(const CoordCyc* a, const uint32_t* mark, uint32_t* par, uint32_t v)
{
	const bool cut = mark[v] != 0 && a[v].low == v;
	if (cut) par[v] = kCoordRoot;
	return cut;
}
// depth pass over the forest that is left: a root is its own ancestor at distance 0, so a walk stays at its root.  Returns whether
// the node's ancestor changed
GAS_FN bool coord_depth_init(const uint32_t* par, const uint32_t* parLen, uint32_t v, CoordDepth* o)
{
	const uint32_t p = par[v];
	o[v] = p == kCoordRoot ? CoordDepth{0, v, 0} : CoordDepth{(int64_t)parLen[v], p, 0};
	return p != kCoordRoot;
}
GAS_FN bool coord_depth_round(const CoordDepth* a, CoordDepth* o, uint32_t v)
{
	const CoordDepth s = a[v], t = a[s.anc];
	o[v] = CoordDepth{s.dist + t.dist, t.anc, 0};                         // (s.anc a root: t = {0, s.anc})
	return t.anc != s.anc;
}
// the tree's extent, at its root's entry (zeroed before the launch, then touched by acc_* alone until the next launch has read it).
// coord_extent_of: what one node gives, its root and depth + length (false: a dummy node); coord_extent: the integer max there.  On
// gfx950 the launch first takes the max over the lanes of a wave that share a root (ga_seed_dev.h) and sends one value per wave and
// root, so that the nodes of a long chain do not queue at one address; the maximum is the same
GAS_FN bool coord_extent_of(const GaDevGraph& g, const CoordDepth* a, uint32_t v, uint32_t& root, uint64_t& end)
{
	if (coord_dummy(g, v)) return false;
	const CoordDepth s = a[v];
	root = s.anc;
	end = (uint64_t)s.dist + (g.node_start[v + 1] - g.node_start[v]);
	return true;
}
GAS_FN void coord_extent(const GaDevGraph& g, const CoordDepth* a, uint64_t* ext, uint32_t v)
{
	uint32_t root = 0;
	uint64_t end = 0;
	if (coord_extent_of(g, a, v, root, end)) acc_max(ext + root, end);
}
// what the scan sums: extent + gap at a root (the exclusive scan in node index order then gives every root its tree's base)
GAS_FN bool coord_contrib(const GaDevGraph& g, const CoordDepth* a, const uint64_t* ext, uint64_t* contrib, uint32_t v)
{
	const bool root = !coord_dummy(g, v) && a[v].anc == v;
	contrib[v] = root ? acc_get(ext + v) + (uint64_t)kTreeGap : 0;
	return root;
}
// 2 * lin + the strand flag the entry holds already (digraph id & 1 in either coordinate); the dummy nodes stay at 0
GAS_FN void coord_write(const GaDevGraph& g, const CoordDepth* a, const uint64_t* base, int64_t* linx, uint32_t v)
{
	if (coord_dummy(g, v)) { linx[v] = 0; return; }
	const CoordDepth s = a[v];
	linx[v] = ((int64_t)base[s.anc] + s.dist) * 2 + (linx[v] & 1);
}

}  // namespace gas
