// ga_emul_seed.cpp -- TEST-ONLY (ga_emul.h): the seed engine of the host emulation, the seeding program of graphaligner_amd/csrc/ga_seed.h
// with both index builds (build, buildWalks), both lookups (find, findLoci) and the topology coordinate (setCoordinate): the per-node and
// per-wave functions of ga_seed.h run for every item in turn, launch by launch, with the two buffers, the "still moving" words and the
// bounds on the rounds that ga_seed_dev.h uses.  What replaces device-library calls here: the stable radix sort of the index entries
// (std::stable_sort by key) and the three scans (per-node counts, "first of its kind" flags, the trees' extents).  A wave slot's
// buffers and the coordinate's work buffers are filled with a pattern before use.
// GA_EMUL_WITHOUT=walks,loci,topology: the withheld entry points answer as GaSeedEngine's defaults do.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <memory>
#include <numeric>

#include "ga_emul.h"
#include "../../graphaligner_amd/csrc/ga_seed.h"

namespace {

struct EmulSeedEngine : GaSeedEngine
{
	const GaDevGraph* g;
	std::vector<uint64_t> keys, vals;
	std::vector<uint32_t> dir;
	std::vector<int64_t> linx, linxFile;
	GaSeedCoordInfo cinf;
	gas::SeedIndex ix{};
	GaSeedIndexInfo inf;
	GaSeedWalkInfo winf;
	bool have = false;
	const uint32_t without;
	EmulSeedEngine(const GaDevGraph* graph, uint32_t withheld) : g(graph), without(withheld) {}
	bool built() const override { return have; }
	GaSeedIndexInfo info() const override { return inf; }

	GaSeedWalkInfo walkInfo() const override { return (without & gae::NO_WALKS) ? GaSeedEngine::walkInfo() : winf; }
	int build(uint32_t k, uint32_t sampleShift, const std::vector<int64_t>& lx) override { return buildIndex(k, sampleShift, 0, lx); }
	int buildWalks(uint32_t k, uint32_t sampleShift, uint32_t maxWalks, const std::vector<int64_t>& lx) override
	{
		if (without & gae::NO_WALKS) return GaSeedEngine::buildWalks(k, sampleShift, maxWalks, lx);
		if (maxWalks < 1 || maxWalks > 256 || k - 1 > gas::kWalkLevels) return 100;
		return buildIndex(k, sampleShift, maxWalks, lx);
	}

	int buildIndex(uint32_t k, uint32_t sampleShift, uint32_t maxWalks, const std::vector<int64_t>& lx)
	{
		const auto t0 = std::chrono::steady_clock::now();
		const uint32_t nNodes = g->n_nodes;
		std::vector<uint64_t> counts(nNodes + 1, 0), firstEntry(nNodes + 1, 0);
		auto st = std::make_unique<gas::WalkStack>();
		memset(st.get(), 0xa5, sizeof(gas::WalkStack));
		gas::WalkTally tally{0, 0, 0};
		for (uint32_t node = 0; node < nNodes; node++)
		{
			if (maxWalks) gas::walk_index_count(*g, node, k, sampleShift, maxWalks, *st, (int)(node % 64), tally, counts.data());
			else gas::index_count(*g, node, k, sampleShift, counts.data());
		}
		for (uint32_t node = 0; node < nNodes; node++) firstEntry[node + 1] = firstEntry[node] + counts[node];
		const uint64_t total = firstEntry[nNodes];
		if (total >= 0xfffffff0ull) return 100;
		uint32_t n = (uint32_t)total;
		std::vector<uint64_t> keysIn(n + 1), valsIn(n + 1);
		for (uint32_t node = 0; node < nNodes; node++)
		{
			if (maxWalks) gas::walk_index_write(*g, node, k, sampleShift, maxWalks, *st, (int)(node % 64), firstEntry.data(), keysIn.data(), valsIn.data());
			else gas::index_write(*g, node, k, sampleShift, firstEntry.data(), keysIn.data(), valsIn.data());
		}
		std::vector<uint32_t> perm(n);
		std::iota(perm.begin(), perm.end(), 0u);
		std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return keysIn[a] < keysIn[b]; });
		keys.assign(n + 1, 0); vals.assign(n + 1, 0);
		for (uint32_t i = 0; i < n; i++) { keys[i] = keysIn[perm[i]]; vals[i] = valsIn[perm[i]]; }
		GaSeedWalkInfo w;
		w.max_walks = maxWalks;
		if (maxWalks)
		{
			// flag, scan, move: as the device does it
			std::vector<uint32_t> pos(n + 1, 0);
			for (uint32_t i = 0; i < n; i++) pos[i + 1] = pos[i] + gas::index_first_of_its_kind(keys.data(), vals.data(), i);
			for (uint32_t i = 0; i < n; i++) if (pos[i + 1] != pos[i]) { keys[pos[i]] = keys[i]; vals[pos[i]] = vals[i]; }
			w.tail_starts = tally.tail_starts; w.tail_starts_skipped = tally.skipped; w.walk_kmers = tally.walks;
			w.duplicates_dropped = n - pos[n];
			n = pos[n];
			keys.resize(n + 1); vals.resize(n + 1);
			keys[n] = 0; vals[n] = 0;
		}
		uint32_t bits = 1;
		while (bits < 2 * k && bits < 28 && (1ull << bits) < n) bits++;
		const uint32_t buckets = 1u << bits;
		dir.assign((size_t)buckets + 2, 0);
		uint64_t distinct = 0;
		for (uint64_t i = 0; i <= n; i++)
		{
			gas::index_dir(keys.data(), n, 2 * k - bits, buckets, dir.data(), (uint32_t)i);
			if (i < n && (i == 0 || keys[i] != keys[i - 1])) distinct++;
		}
		linx = lx;
		linxFile = lx;
		cinf = GaSeedCoordInfo();
		ix.k = k; ix.sample_shift = sampleShift; ix.dir_shift = 2 * k - bits; ix.n_entries = n;
		ix.keys = keys.data(); ix.vals = vals.data(); ix.dir = dir.data(); ix.linx = linx.data();
		inf = GaSeedIndexInfo();
		inf.entries = n; inf.distinct_keys = distinct; inf.k = k; inf.sample_shift = sampleShift; inf.dir_bits = bits;
		inf.bytes = (uint64_t)n * 16 + ((uint64_t)buckets + 1) * 4 + (uint64_t)linx.size() * 8;
		inf.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
		winf = w;
		have = true;
		return 0;
	}

	GaSeedCoordInfo coordInfo() const override { return (without & gae::NO_TOPOLOGY) ? GaSeedEngine::coordInfo() : cinf; }
	int copyLin(int64_t* lin, size_t capacity) const override
	{
		if (without & gae::NO_TOPOLOGY) return GaSeedEngine::copyLin(lin, capacity);
		if (!have) return 100;
		const size_t n = std::min<size_t>(capacity, linx.size());
		for (size_t i = 0; i < n; i++) lin[i] = linx[i] >> 1;
		return 0;
	}

	// the launches of DevSeedEngine::setCoordinate, a launch = a loop over the nodes
	int setCoordinate(int kind, GaSeedCoordInfo& out) override
	{
		if (without & gae::NO_TOPOLOGY) return GaSeedEngine::setCoordinate(kind, out);
		if (!have || (kind != 0 && kind != 1)) return 100;
		if (kind == 0)
		{
			std::copy(linxFile.begin(), linxFile.end(), linx.begin());         // (in place: ix.linx points at it)
			cinf = GaSeedCoordInfo();
			out = cinf;
			return 0;
		}
		const auto t0 = std::chrono::steady_clock::now();
		const uint32_t n = g->n_nodes, R = gas::coord_rounds(n);
		std::vector<gas::CoordDepth> stA(n), stB(n);
		memset(stA.data(), 0xa5, (size_t)n * sizeof(gas::CoordDepth));
		memset(stB.data(), 0xa5, (size_t)n * sizeof(gas::CoordDepth));
		std::vector<uint32_t> par(n, 0xa5a5a5a5u), parLen(n, 0xa5a5a5a5u), mark(n, 0);
		std::vector<uint64_t> ext(n, 0), contrib((size_t)n + 1, 0xa5a5a5a5a5a5a5a5ull), base((size_t)n + 1, 0xa5a5a5a5a5a5a5a5ull);
		GaSeedCoordInfo c;
		c.kind = 1;
		std::vector<gas::CoordCyc> cyA(n), cyB(n);                           // (the device keeps these in the first half of the two state buffers)
		memset(cyA.data(), 0xa5, (size_t)n * sizeof(gas::CoordCyc));
		memset(cyB.data(), 0xa5, (size_t)n * sizeof(gas::CoordCyc));
		gas::CoordCyc* ca = cyA.data(); gas::CoordCyc* co = cyB.data();
		bool mv = false;
		for (uint32_t v = 0; v < n; v++) { gas::coord_parent(*g, v, par.data(), parLen.data()); mv |= gas::coord_cyc_init(par.data(), v, ca); }
		while (mv && c.cycle_rounds < R)
		{
			mv = false;
			for (uint32_t v = 0; v < n; v++) mv |= gas::coord_cyc_round(ca, co, v);
			c.cycle_rounds++;
			std::swap(ca, co);
		}
		if (mv)
		{
			for (uint32_t v = 0; v < n; v++) gas::coord_mark(ca, mark.data(), v);
			for (uint32_t v = 0; v < n; v++) c.cycles_cut += gas::coord_cut(ca, mark.data(), par.data(), v) ? 1u : 0u;
		}
		gas::CoordDepth* da = stA.data(); gas::CoordDepth* dd = stB.data();
		mv = false;
		for (uint32_t v = 0; v < n; v++) mv |= gas::coord_depth_init(par.data(), parLen.data(), v, da);
		while (mv && c.depth_rounds < R + 1)
		{
			mv = false;
			for (uint32_t v = 0; v < n; v++) mv |= gas::coord_depth_round(da, dd, v);
			c.depth_rounds++;
			std::swap(da, dd);
		}
		if (mv) return 102;
		for (uint32_t v = 0; v < n; v++) gas::coord_extent(*g, da, ext.data(), v);
		for (uint32_t v = 0; v < n; v++) c.trees += gas::coord_contrib(*g, da, ext.data(), contrib.data(), v) ? 1u : 0u;
		contrib[n] = 0;
		uint64_t run = 0;
		for (uint32_t v = 0; v <= n; v++) { base[v] = run; run += contrib[v]; }
		for (uint32_t v = 0; v < n; v++) gas::coord_write(*g, da, base.data(), linx.data(), v);
		c.extent_sum = base[n] - (uint64_t)c.trees * (uint64_t)gas::kTreeGap;
		c.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
		cinf = c;
		out = c;
		return 0;
	}

	int copy(uint64_t* k, uint32_t* nodes, uint32_t* offsets, size_t capacity) const override
	{
		if (!have) return 100;
		const size_t n = std::min<size_t>(capacity, ix.n_entries);
		for (size_t i = 0; i < n; i++) { k[i] = keys[i]; nodes[i] = (uint32_t)(vals[i] >> 32); offsets[i] = (uint32_t)vals[i]; }
		return 0;
	}

	int find(const char* const* seqs, const size_t* lens, size_t nReads, const GaSeedParams& p, GaSeedOut& out) override { return run(seqs, lens, nReads, p, out, false); }
	int findLoci(const char* const* seqs, const size_t* lens, size_t nReads, const GaSeedParams& p, GaSeedOut& out) override
	{
		return (without & gae::NO_LOCI) ? GaSeedEngine::findLoci(seqs, lens, nReads, p, out) : run(seqs, lens, nReads, p, out, true);
	}

	int run(const char* const* seqs, const size_t* lens, size_t nReads, const GaSeedParams& p, GaSeedOut& out, bool byLocus)
	{
		if (!have) return 100;
		out.locus_hits.clear(); out.locus_first_p.clear(); out.locus_last_p.clear(); out.n_loci.clear();
		if (byLocus)
		{
			out.locus_hits.assign(nReads * p.max_seeds, 0); out.locus_first_p.assign(nReads * p.max_seeds, 0); out.locus_last_p.assign(nReads * p.max_seeds, 0);
			out.n_loci.assign(nReads, 0);
		}
		out.n_seeds.assign(nReads, 0); out.n_hits.assign(nReads, 0); out.truncated.assign(nReads, 0);
		out.node.assign(nReads * p.max_seeds, 0); out.pos.assign(nReads * p.max_seeds, 0); out.support.assign(nReads * p.max_seeds, 0);
		out.kernel_ms = 0;
		if (nReads == 0) return 0;
		std::vector<gas::SeedRead> recs(nReads);
		uint64_t seqBytes = 0;
		for (size_t i = 0; i < nReads; i++)
		{
			if (lens[i] > 0xfffffff0ull) return 100;
			recs[i] = gas::SeedRead{seqBytes, (uint32_t)lens[i], 0};
			seqBytes += ((lens[i] + 15) & ~(size_t)15) + 16;
		}
		// (16-byte aligned like the device buffer: pack16 reads words)
		std::vector<uint64_t> seqStore(seqBytes / 8 + 2, 0);
		uint8_t* seq = (uint8_t*)seqStore.data();
		for (size_t i = 0; i < nReads; i++) memcpy(seq + recs[i].off, seqs[i], lens[i]);
		std::vector<uint32_t> order(nReads);
		std::iota(order.begin(), order.end(), 0u);
		std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return lens[a] > lens[b]; });
		// a few wave slots, one after the other: a slot's hit buffer and the LDS block are reused with whatever the read before left in them
		const uint32_t slots = 3;
		std::vector<uint32_t> hitP((size_t)slots * p.max_hits, 0xdeadbeefu), hitNode(hitP), hitSup(hitP);
		std::vector<int64_t> hitDx((size_t)slots * p.max_hits, -12345);
		std::vector<uint32_t> outN(nReads * 3, 0), outSeed(nReads * p.max_seeds * 3, 0);
		gas::SeedLaunch L;
		memset(&L, 0, sizeof(L));
		L.ix = ix; L.p = p; L.seq = seq; L.reads = recs.data(); L.order = order.data(); L.n_reads = (uint32_t)nReads;
		L.hit_p = hitP.data(); L.hit_node = hitNode.data(); L.hit_dx = hitDx.data(); L.hit_sup = hitSup.data();
		L.out_n = outN.data(); L.out_seed = outSeed.data();
		std::vector<uint32_t> locLab, locAlt, locLast, locRun, locNbr, outLocus(nReads * p.max_seeds * 3, 0);
		std::vector<uint64_t> locBest;
		if (byLocus)
		{
			locLab = hitP; locAlt = hitP; locLast = hitP; locRun = hitP; locNbr = hitP;
			locBest.assign((size_t)slots * p.max_hits, 0xdeadbeefdeadbeefull);
			L.loc_lab = locLab.data(); L.loc_alt = locAlt.data(); L.loc_last = locLast.data(); L.loc_run = locRun.data(); L.loc_best = locBest.data(); L.loc_nbr = locNbr.data();
			L.out_locus = outLocus.data(); L.out_nloci = out.n_loci.data();
		}
		auto lds = std::make_unique<gas::SeedLdsLoci>();
		memset(lds.get(), 0xa5, sizeof(gas::SeedLdsLoci));
		const auto t0 = std::chrono::steady_clock::now();
		for (uint32_t slot = 0; slot < slots; slot++)
		{
			if (byLocus) gas::seed_wave_loci(L, *lds, slot, slots);
			else gas::seed_wave(L, *lds, slot, slots);
		}
		out.kernel_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
		for (size_t i = 0; i < nReads; i++) { out.n_seeds[i] = outN[i * 3]; out.n_hits[i] = outN[i * 3 + 1]; out.truncated[i] = outN[i * 3 + 2]; }
		for (size_t i = 0; i < nReads * p.max_seeds; i++) { out.node[i] = outSeed[i * 3]; out.pos[i] = outSeed[i * 3 + 1]; out.support[i] = outSeed[i * 3 + 2]; }
		if (byLocus)
			for (size_t i = 0; i < nReads * p.max_seeds; i++) { out.locus_hits[i] = outLocus[i * 3]; out.locus_first_p[i] = outLocus[i * 3 + 1]; out.locus_last_p[i] = outLocus[i * 3 + 2]; }
		return 0;
	}
};

}  // namespace

GaSeedEngine* gae::newSeedEngine(const GaDevGraph* g, uint32_t without) { return new EmulSeedEngine(g, without); }
