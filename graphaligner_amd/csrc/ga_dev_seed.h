// ga_dev_seed.h -- the seed engine of the device back end: the host side of the seeding kernels (ga_seed_dev.h).  It owns the k-mer index
// of a graph in HBM and the buffers of the finds, builds the index and the topology coordinate as named stages over the owners of
// ga_dev.h (DevBuf, GrownBuf, Events, Scan, SortPairs), and launches the seeding kernels: for ga_find_seeds over reads it uploads, and
// for a seeded batch (ga_dev_prepare.h) over reads that lie in device memory already.
// Not a header for others: a part of ga_device.hip's translation unit, included by ga_dev.h below its owners and above the graph.
#ifndef GA_DEVICE_PARTS
#error "ga_dev_seed.h is a part of ga_device.hip"
#endif

namespace gasd {

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
	uint64_t* dKeys = nullptr; uint64_t* dVals = nullptr; uint32_t* dDir = nullptr; int64_t* dLinx = nullptr;      // the index: IndexBuild hands them over
	// buffers of find(), kept between calls
	GrownBuf work;                             // the reads and the outputs of run()
	GrownBuf hits;                             // the per-slot hit buffers
	GrownBuf loci;                             // the per-hit buffers of findLoci: allocated at its first call
	Events<2> ev;                              // around the kernel of run()

	DevSeedEngine(GaBackendGraph* o, int dev, int nCus, const GaDevGraph& graph) : owner(o), device(dev), cus(nCus), g(graph) {}
	void dropIndex()
	{
		for (void* p : {(void*)dKeys, (void*)dVals, (void*)dDir, (void*)dLinx}) if (p) hipFree(p);
		dKeys = dVals = nullptr; dDir = nullptr; dLinx = nullptr;
		have = false;
	}
	~DevSeedEngine() override { hipSetDevice(device); dropIndex(); }          // (then the buffers and the events)
	bool built() const override { return have; }
	GaSeedIndexInfo info() const override { return inf; }
	GaSeedWalkInfo walkInfo() const override { return winf; }
	GaSeedCoordInfo coordInfo() const override { return cinf; }

	// ---- the index ----------------------------------------------------------------------------------------------------------------
	int build(uint32_t k, uint32_t sampleShift, const std::vector<int64_t>& linx) override { return buildIndex(k, sampleShift, 0, linx); }
	int buildWalks(uint32_t k, uint32_t sampleShift, uint32_t maxWalks, const std::vector<int64_t>& linx) override
	{
		if (maxWalks < 1 || maxWalks > 256 || k - 1 > gas::kWalkLevels) return GA_E_INVALID;
		return buildIndex(k, sampleShift, maxWalks, linx);
	}

	// one build: what its stages allocate and hand to each other.  Whatever publish() has not handed to the engine is freed with it, after
	// the build's last wait for the device; a stage releases sooner (reset()) only what the promised peak of device memory requires, so
	// the order of launches, copies, waits and releases is what it always was.  That is why sortTmp, flags and pos are members although
	// one stage alone uses each: as locals of their stage they would be released while its last kernel runs (hipFree waits for it):
	// another order of waits and releases.  Whoever moves them checks the peak that include/graphaligner_amd.h promises and measures.
	struct IndexBuild
	{
		uint32_t k, sampleShift, maxWalks;                // maxWalks = 0: the in-node index
		DevBuf<uint64_t> counts, firstEntry;              // per node and one more: its entries, the number of the first of them
		DevBuf<unsigned long long> tally;                 // walk index: tail starts, skipped ones, walks
		DevBuf<uint64_t> keysIn, valsIn;                  // the entries as written, node by node
		DevBuf<uint8_t> sortTmp;
		DevBuf<uint64_t> keysSorted, valsSorted;          // walk index: the sorted entries, equal triples still among them
		DevBuf<uint32_t> flags, pos;                      // walk index: first of its kind, and where it goes
		DevBuf<uint64_t> keys, vals;                      // the index's four arrays
		DevBuf<uint32_t> dir;
		DevBuf<int64_t> linx;
		uint32_t n = 0;                                   // entries
		uint32_t bits = 0, buckets = 0;                   // of the directory
		unsigned long long distinct = 0;
		GaSeedWalkInfo w;
		IndexBuild(uint32_t k, uint32_t sampleShift, uint32_t maxWalks) : k(k), sampleShift(sampleShift), maxWalks(maxWalks) { w.max_walks = maxWalks; }
	};

	int buildIndex(uint32_t k, uint32_t sampleShift, uint32_t maxWalks, const std::vector<int64_t>& linx)
	{
		std::lock_guard<std::mutex> guard(lock);
		HIP_OK(hipSetDevice(device));
		dropIndex();
		const auto t0 = std::chrono::steady_clock::now();
		{
			IndexBuild b(k, sampleShift, maxWalks);
			int st = countAndPlace(b);
			if (!st) st = writeAndSort(b);
			if (!st && maxWalks) st = dropEqualTriples(b);
			if (!st) st = makeDirectory(b, linx);
			if (st) return st;
			publish(b, linx);
		}
		// (the build's temporaries are gone: their release is part of the build's time)
		inf.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
		linxFile = linx;                                                    // (the host's copy for kind 0 is not part of the build's time)
		have = true;
		return 0;
	}

	// stage 1: every node's number of entries, and by a scan its first entry and the total; an index of 2^32 entries is refused
	int countAndPlace(IndexBuild& b)
	{
		const uint32_t nNodes = g.n_nodes;
		if (b.counts.alloc((size_t)nNodes + 1) || b.firstEntry.alloc((size_t)nNodes + 1)) return GA_E_DEVICE;
		if (b.maxWalks)
		{
			if (b.tally.alloc(3)) return GA_E_DEVICE;
			HIP_OK(hipMemset(b.tally.p, 0, 3 * 8));
			hipLaunchKernelGGL(ga_seed_walk_count_kernel, dim3((nNodes + 1 + 63) / 64), dim3(64), 0, 0, g, b.k, b.sampleShift, b.maxWalks, b.counts.p, b.tally.p);
		}
		else hipLaunchKernelGGL(ga_seed_count_kernel, dim3((nNodes + 1 + 255) / 256), dim3(256), 0, 0, g, b.k, b.sampleShift, b.counts.p);
		Scan<uint64_t> place{b.counts.p, b.firstEntry.p, (size_t)nNodes + 1};
		DevBuf<uint8_t> tmp;
		if (place.size(0) || tmp.alloc(std::max<size_t>(place.tmpBytes, 16)) || place.run(tmp.p, 0)) return GA_E_DEVICE;
		uint64_t total = 0;
		HIP_OK(hipMemcpy(&total, b.firstEntry.p + nNodes, 8, hipMemcpyDeviceToHost));
		if (total >= 0xfffffff0ull) return GA_E_INVALID;                       // entry numbers are 32-bit
		b.n = (uint32_t)total;
		return 0;
	}

	// stage 2: the entries node by node, then by key, stable: equal keys keep the (node, offset) order they were written in.  The in-node
	// index is sorted straight into its arrays, the walk index into keysSorted / valsSorted, out of which stage 3 moves what stays.
	int writeAndSort(IndexBuild& b)
	{
		const uint32_t nNodes = g.n_nodes;
		const size_t cap = std::max<size_t>(b.n, 2);
		DevBuf<uint64_t>& sortedK = b.maxWalks ? b.keysSorted : b.keys;
		DevBuf<uint64_t>& sortedV = b.maxWalks ? b.valsSorted : b.vals;
		if (b.keysIn.alloc(cap) || b.valsIn.alloc(cap) || sortedK.alloc(cap) || sortedV.alloc(cap)) return GA_E_DEVICE;
		if (b.maxWalks) hipLaunchKernelGGL(ga_seed_walk_write_kernel, dim3((nNodes + 1 + 63) / 64), dim3(64), 0, 0, g, b.k, b.sampleShift, b.maxWalks, (const uint64_t*)b.firstEntry.p, b.keysIn.p, b.valsIn.p);
		else hipLaunchKernelGGL(ga_seed_write_kernel, dim3((nNodes + 1 + 255) / 256), dim3(256), 0, 0, g, b.k, b.sampleShift, (const uint64_t*)b.firstEntry.p, b.keysIn.p, b.valsIn.p);
		if (b.n > 0)
		{
			SortPairs<uint64_t, uint64_t> sort{b.keysIn.p, sortedK.p, b.valsIn.p, sortedV.p, (size_t)b.n, 2u * b.k};
			if (sort.size(0) || b.sortTmp.alloc(std::max<size_t>(sort.tmpBytes, 16)) || sort.run(b.sortTmp.p, 0)) return GA_E_DEVICE;
		}
		return 0;
	}

	// stage 3, walk index only: two walks of one start with equal text wrote the same triple twice, and one stays.  Equal (key, node,
	// offset) triples are neighbours after the sort: flag the first of each, scan, move the flagged ones into the index's arrays.
	// (The sort's storage and the unsorted entries go first: the walk index's peak is two arrays of 16 bytes per entry and 8 more.)
	int dropEqualTriples(IndexBuild& b)
	{
		b.sortTmp.reset();
		unsigned long long tally[3] = {0, 0, 0};
		HIP_OK(hipMemcpy(tally, b.tally.p, 3 * 8, hipMemcpyDeviceToHost));
		b.w.tail_starts = tally[0]; b.w.tail_starts_skipped = tally[1]; b.w.walk_kmers = tally[2];
		b.keysIn.reset();
		b.valsIn.reset();
		const uint32_t n = b.n, entryBlocks = (uint32_t)(((uint64_t)n + 1 + 255) / 256);
		DevBuf<uint32_t>& flags = b.flags; DevBuf<uint32_t>& pos = b.pos;
		if (flags.alloc((size_t)n + 1) || pos.alloc((size_t)n + 1)) return GA_E_DEVICE;
		hipLaunchKernelGGL(ga_seed_flag_kernel, dim3(entryBlocks), dim3(256), 0, 0, (const uint64_t*)b.keysSorted.p, (const uint64_t*)b.valsSorted.p, n, flags.p);
		Scan<uint32_t> place{flags.p, pos.p, (size_t)n + 1};
		DevBuf<uint8_t> tmp;
		if (place.size(0) || tmp.alloc(std::max<size_t>(place.tmpBytes, 16)) || place.run(tmp.p, 0)) return GA_E_DEVICE;
		uint32_t unique = 0;
		HIP_OK(hipMemcpy(&unique, pos.p + n, 4, hipMemcpyDeviceToHost));
		tmp.reset();
		if (unique > n) return GA_E_DEVICE;
		const size_t ucap = std::max<size_t>(unique, 2);
		if (b.keys.alloc(ucap) || b.vals.alloc(ucap)) return GA_E_DEVICE;
		hipLaunchKernelGGL(ga_seed_compact_kernel, dim3(entryBlocks), dim3(256), 0, 0, (const uint64_t*)b.keysSorted.p, (const uint64_t*)b.valsSorted.p, n, (const uint32_t*)pos.p, b.keys.p, b.vals.p);
		b.w.duplicates_dropped = n - unique;
		b.n = unique;
		return 0;
	}

	// stage 4: the directory (top bits of the key -> first entry; about one entry per bucket) with the number of distinct keys, and the
	// coordinate's upload
	int makeDirectory(IndexBuild& b, const std::vector<int64_t>& linx)
	{
		const uint32_t n = b.n;
		b.bits = 1;
		while (b.bits < 2 * b.k && b.bits < 28 && (1ull << b.bits) < n) b.bits++;
		b.buckets = 1u << b.bits;
		if (b.dir.alloc((size_t)b.buckets + 2) || b.linx.alloc(std::max<size_t>(linx.size(), 1))) return GA_E_DEVICE;
		HIP_OK(hipMemcpy(b.linx.p, linx.data(), linx.size() * 8, hipMemcpyHostToDevice));
		unsigned long long* dDistinct = (unsigned long long*)b.counts.p;     // (reused: the counts are no longer needed)
		HIP_OK(hipMemset(dDistinct, 0, 8));
		hipLaunchKernelGGL(ga_seed_dir_kernel, dim3((uint32_t)(((uint64_t)n + 1 + 255) / 256)), dim3(256), 0, 0, (const uint64_t*)b.keys.p, n, 2 * b.k - b.bits, b.buckets, b.dir.p, dDistinct);
		HIP_OK(hipMemcpy(&b.distinct, dDistinct, 8, hipMemcpyDeviceToHost));
		HIP_OK(hipDeviceSynchronize());
		return 0;
	}

	// stage 5: the index is the engine's (buildIndex adds build_ms and sets `have`)
	void publish(IndexBuild& b, const std::vector<int64_t>& linx)
	{
		dKeys = b.keys.release(); dVals = b.vals.release(); dDir = b.dir.release(); dLinx = b.linx.release();
		ix.k = b.k; ix.sample_shift = b.sampleShift; ix.dir_shift = 2 * b.k - b.bits; ix.n_entries = b.n;
		ix.keys = dKeys; ix.vals = dVals; ix.dir = dDir; ix.linx = dLinx;
		inf = GaSeedIndexInfo();
		inf.entries = b.n; inf.distinct_keys = b.distinct; inf.k = b.k; inf.sample_shift = b.sampleShift; inf.dir_bits = b.bits;
		inf.bytes = (uint64_t)b.n * 16 + ((uint64_t)b.buckets + 1) * 4 + (uint64_t)linx.size() * 8;
		winf = b.w;
		cinf = GaSeedCoordInfo();
	}

	int copy(uint64_t* keys, uint32_t* nodes, uint32_t* offsets, size_t capacity) const override
	{
		if (!have) return GA_E_INVALID;
		const size_t n = std::min<size_t>(capacity, ix.n_entries);
		if (n == 0) return 0;
		HIP_OK(hipSetDevice(device));
		std::vector<uint64_t> vals(n);
		HIP_OK(hipMemcpy(keys, dKeys, n * 8, hipMemcpyDeviceToHost));
		HIP_OK(hipMemcpy(vals.data(), dVals, n * 8, hipMemcpyDeviceToHost));
		for (size_t i = 0; i < n; i++) { nodes[i] = (uint32_t)(vals[i] >> 32); offsets[i] = (uint32_t)vals[i]; }
		return 0;
	}

	// ---- the coordinate -----------------------------------------------------------------------------------------------------------
	int copyLin(int64_t* lin, size_t capacity) const override
	{
		if (!have) return GA_E_INVALID;
		const size_t n = std::min<size_t>(capacity, g.n_nodes);
		if (n == 0) return 0;
		HIP_OK(hipSetDevice(device));
		HIP_OK(hipMemcpy(lin, dLinx, n * 8, hipMemcpyDeviceToHost));
		for (size_t i = 0; i < n; i++) lin[i] >>= 1;
		return 0;
	}

	// one build of the topology coordinate: the passes' arrays, one element per node, and their control words
	struct CoordBuild
	{
		uint32_t n, blocks, R;
		// control words: "still moving" of the cycle pass' start and of each of its <= R rounds, of the depth pass' start and of each of
		// its <= R + 1 rounds, then the two counters
		uint32_t fCyc, fDepth, cCuts, cTrees, nCtl;
		DevBuf<uint8_t> stA, stB;                  // the two sides of a pass' rounds, 16 bytes per node: CoordCyc, then CoordDepth
		DevBuf<uint32_t> par, parLen, mark, ctl;
		DevBuf<uint64_t> ext, contrib, base;
		DevBuf<uint8_t> scanTmp;                   // (writeCoordinate's alone, and a member: released with the rest, after the last wait)
		gas::CoordDepth* depth = nullptr;          // the side that holds the depth pass' result
		GaSeedCoordInfo c;
		explicit CoordBuild(uint32_t nNodes) : n(nNodes), blocks((nNodes + 255) / 256), R(gas::coord_rounds(nNodes)), fCyc(0), fDepth(R + 1), cCuts(2 * R + 3), cTrees(cCuts + 1), nCtl(cTrees + 1) { c.kind = 1; }
		int open()
		{
			if (stA.alloc((size_t)n * 16) || stB.alloc((size_t)n * 16) || par.alloc(n) || parLen.alloc(n) || mark.alloc(n) || ext.alloc(n) || contrib.alloc((size_t)n + 1) ||
			    base.alloc((size_t)n + 1) || ctl.alloc(nCtl)) return GA_E_DEVICE;
			HIP_OK(hipMemsetAsync(ctl.p, 0, (size_t)nCtl * 4, 0));
			HIP_OK(hipMemsetAsync(mark.p, 0, (size_t)n * 4, 0));
			HIP_OK(hipMemsetAsync(ext.p, 0, (size_t)n * 8, 0));
			return 0;
		}
		// the host reads a launch's word before it decides on the next launch
		int moving(uint32_t word, bool& mv)
		{
			uint32_t w = 0;
			HIP_OK(hipMemcpy(&w, ctl.p + word, 4, hipMemcpyDeviceToHost));
			mv = w != 0;
			return 0;
		}
	};

	// kind 1: the passes of ga_seed.h ("topology coordinate"), the last of which writes dLinx; the index itself is not touched
	int setCoordinate(int kind, GaSeedCoordInfo& out) override
	{
		std::lock_guard<std::mutex> guard(lock);
		if (!have || (kind != 0 && kind != 1)) return GA_E_INVALID;
		HIP_OK(hipSetDevice(device));
		if (kind == 0) return restoreFileOrder(out);
		const auto t0 = std::chrono::steady_clock::now();
		GaSeedCoordInfo c;
		{
			CoordBuild b(g.n_nodes);
			int st = b.open();
			if (!st) st = cutCycles(b);
			if (!st) st = forestDepths(b);
			if (!st) st = writeCoordinate(b);
			if (!st) st = coordStatistics(b);
			if (st) return st;
			c = b.c;
		}
		c.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
		cinf = c;
		out = c;
		return 0;
	}

	// kind 0: the array build() was given goes back
	int restoreFileOrder(GaSeedCoordInfo& out)
	{
		HIP_OK(hipMemcpy(dLinx, linxFile.data(), linxFile.size() * 8, hipMemcpyHostToDevice));
		cinf = GaSeedCoordInfo();
		out = cinf;
		return 0;
	}

	// parents, and the cycle pass over them; walks that never end: mark the cycles' nodes, cut every cycle at its smallest index
	int cutCycles(CoordBuild& b)
	{
		gas::CoordCyc* ca = (gas::CoordCyc*)b.stA.p; gas::CoordCyc* co = (gas::CoordCyc*)b.stB.p;
		hipLaunchKernelGGL(ga_coord_parent_kernel, dim3(b.blocks), dim3(256), 0, 0, g, b.par.p, b.parLen.p, ca, b.ctl.p + b.fCyc);
		bool mv = false;
		if (b.moving(b.fCyc, mv)) return GA_E_DEVICE;
		while (mv && b.c.cycle_rounds < b.R)
		{
			hipLaunchKernelGGL(ga_coord_cyc_round_kernel, dim3(b.blocks), dim3(256), 0, 0, b.n, (const gas::CoordCyc*)ca, co, b.ctl.p + b.fCyc + 1 + b.c.cycle_rounds);
			if (b.moving(b.fCyc + 1 + b.c.cycle_rounds, mv)) return GA_E_DEVICE;
			b.c.cycle_rounds++;
			std::swap(ca, co);
		}
		if (mv)
		{
			hipLaunchKernelGGL(ga_coord_mark_kernel, dim3(b.blocks), dim3(256), 0, 0, b.n, (const gas::CoordCyc*)ca, b.mark.p);
			hipLaunchKernelGGL(ga_coord_cut_kernel, dim3(b.blocks), dim3(256), 0, 0, b.n, (const gas::CoordCyc*)ca, (const uint32_t*)b.mark.p, b.par.p, b.ctl.p + b.cCuts);
		}
		return 0;
	}

	// depths in the forest
	int forestDepths(CoordBuild& b)
	{
		gas::CoordDepth* da = (gas::CoordDepth*)b.stA.p; gas::CoordDepth* dd = (gas::CoordDepth*)b.stB.p;
		hipLaunchKernelGGL(ga_coord_depth_init_kernel, dim3(b.blocks), dim3(256), 0, 0, b.n, (const uint32_t*)b.par.p, (const uint32_t*)b.parLen.p, da, b.ctl.p + b.fDepth);
		bool mv = false;
		if (b.moving(b.fDepth, mv)) return GA_E_DEVICE;
		while (mv && b.c.depth_rounds < b.R + 1)
		{
			hipLaunchKernelGGL(ga_coord_depth_round_kernel, dim3(b.blocks), dim3(256), 0, 0, b.n, (const gas::CoordDepth*)da, dd, b.ctl.p + b.fDepth + 1 + b.c.depth_rounds);
			if (b.moving(b.fDepth + 1 + b.c.depth_rounds, mv)) return GA_E_DEVICE;
			b.c.depth_rounds++;
			std::swap(da, dd);
		}
		if (mv) return GA_E_DEVICE;                                            // (never: a forest's walks are at their roots after R rounds)
		b.depth = da;
		return 0;
	}

	// extents at the roots, bases by a scan in node index order, the write
	int writeCoordinate(CoordBuild& b)
	{
		const gas::CoordDepth* da = b.depth;
		hipLaunchKernelGGL(ga_coord_extent_kernel, dim3(b.blocks), dim3(256), 0, 0, g, da, b.ext.p);
		hipLaunchKernelGGL(ga_coord_contrib_kernel, dim3((b.n + 1 + 255) / 256), dim3(256), 0, 0, g, da, (const uint64_t*)b.ext.p, b.contrib.p, b.ctl.p + b.cTrees);
		Scan<uint64_t> place{b.contrib.p, b.base.p, (size_t)b.n + 1};
		if (place.size(0) || b.scanTmp.alloc(std::max<size_t>(place.tmpBytes, 16)) || place.run(b.scanTmp.p, 0)) return GA_E_DEVICE;
		hipLaunchKernelGGL(ga_coord_write_kernel, dim3(b.blocks), dim3(256), 0, 0, g, da, (const uint64_t*)b.base.p, dLinx);
		return 0;
	}

	// the scan's last element and the two counters
	int coordStatistics(CoordBuild& b)
	{
		uint64_t total = 0;
		uint32_t counts[2] = {0, 0};
		HIP_OK(hipMemcpy(&total, b.base.p + b.n, 8, hipMemcpyDeviceToHost));
		HIP_OK(hipMemcpy(counts, b.ctl.p + b.cCuts, 8, hipMemcpyDeviceToHost));
		HIP_OK(hipDeviceSynchronize());
		b.c.cycles_cut = counts[0]; b.c.trees = counts[1];
		b.c.extent_sum = total - (uint64_t)b.c.trees * (uint64_t)gas::kTreeGap;
		return 0;
	}

	// ---- the finds ----------------------------------------------------------------------------------------------------------------
	int find(const char* const* seqs, const size_t* lens, size_t nReads, const GaSeedParams& p, GaSeedOut& out) override { return run(seqs, lens, nReads, p, out, false); }
	int findLoci(const char* const* seqs, const size_t* lens, size_t nReads, const GaSeedParams& p, GaSeedOut& out) override { return run(seqs, lens, nReads, p, out, true); }

	// where a launch's reads lie in device memory, and where its outputs go (the last two: by locus only)
	struct SeedIo
	{
		const uint8_t* seq; const gas::SeedRead* reads; const uint32_t* order;
		uint32_t* outN; uint32_t* outSeed; uint32_t* outLocus; uint32_t* outNLoci;
	};

	// The launch record and the number of wave slots of a launch of the seeding kernels, with the per-slot hit (and, by locus, label)
	// buffers grown when needed.  Under `lock`.  (Two functions and not one with launch() below: run() grows the buffers before it queues
	// its upload and records its first event, and launches behind them; a release inside one function would come to lie behind the
	// upload and inside the timed span.)
	int prepareLaunch(gas::SeedLaunch& L, uint32_t& slots, const GaSeedParams& p, size_t nReads, bool byLocus, const SeedIo& io)
	{
		// (the kernel waits on dependent loads: directory, keys, entry, coordinate; sixteen waves per CU hide them, and the kernel's
		// registers and LDS would allow more)
		slots = (uint32_t)std::min<size_t>(nReads, (size_t)std::max(cus, 1) * (byLocus ? kLociWavesPerCu : kWavesPerCu));
		const size_t per = (size_t)slots * p.max_hits;
		if (hits.ensure(per * 20) || loci.ensure(byLocus ? per * 28 : 0)) return GA_E_DEVICE;
		memset(&L, 0, sizeof(L));
		L.ix = ix; L.p = p;
		L.n_reads = (uint32_t)nReads;
		L.hit_dx = (int64_t*)hits.p; L.hit_p = (uint32_t*)((uint8_t*)hits.p + per * 8); L.hit_node = L.hit_p + per; L.hit_sup = L.hit_node + per;
		if (byLocus) { L.loc_best = (uint64_t*)loci.p; L.loc_lab = (uint32_t*)((uint8_t*)loci.p + per * 8); L.loc_alt = L.loc_lab + per; L.loc_last = L.loc_alt + per; L.loc_run = L.loc_last + per; L.loc_nbr = L.loc_run + per; }
		L.seq = io.seq; L.reads = io.reads; L.order = io.order;
		L.out_n = io.outN; L.out_seed = io.outSeed;
		if (byLocus) { L.out_locus = io.outLocus; L.out_nloci = io.outNLoci; }
		return 0;
	}
	// byLocus: one seed per locus (ga_seed_find_loci_kernel) instead of hit by hit
	void launch(const gas::SeedLaunch& L, uint32_t slots, bool byLocus, hipStream_t stream)
	{
		if (byLocus) hipLaunchKernelGGL(ga_seed_find_loci_kernel, dim3(slots), dim3(64), 0, stream, L);
		else hipLaunchKernelGGL(ga_seed_find_kernel, dim3(slots), dim3(64), 0, stream, L);
	}

	// The seeding kernel over reads that lie in device memory already (a seeded batch, ga_plan.h), on the caller's stream; the outputs stay in
	// device memory, where the caller's pointers say (cleared by the caller).  The caller holds `lock` from before this call until its
	// stream has finished the kernel: the hit and label buffers are per graph.
	int launchResident(const GaSeedParams& p, size_t nReads, bool byLocus, const uint8_t* seq, const gas::SeedRead* reads, const uint32_t* order,
	                   uint32_t* outN, uint32_t* outSeed, uint32_t* outLocus, uint32_t* outNLoci, hipStream_t stream)
	{
		if (!have) return GA_E_INVALID;
		gas::SeedLaunch L;
		uint32_t slots = 0;
		if (int st = prepareLaunch(L, slots, p, nReads, byLocus, SeedIo{seq, reads, order, outN, outSeed, outLocus, outNLoci})) return st;
		launch(L, slots, byLocus, stream);
		HIP_OK(hipGetLastError());
		return 0;
	}

	// records of three words, as the kernels write them, apart into three arrays (of a.size() elements each)
	static void unpack3(const std::vector<uint32_t>& rec, std::vector<uint32_t>& a, std::vector<uint32_t>& b, std::vector<uint32_t>& c)
	{
		for (size_t i = 0; i < a.size(); i++) { a[i] = rec[i * 3]; b[i] = rec[i * 3 + 1]; c[i] = rec[i * 3 + 2]; }
	}

	// the reads packed and uploaded, the launch on the null stream, the outputs' way back
	int run(const char* const* seqs, const size_t* lens, size_t nReads, const GaSeedParams& p, GaSeedOut& out, bool byLocus)
	{
		std::lock_guard<std::mutex> guard(lock);
		if (!have) return GA_E_INVALID;
		const size_t nSeeds = nReads * p.max_seeds;
		out.n_seeds.assign(nReads, 0); out.n_hits.assign(nReads, 0); out.truncated.assign(nReads, 0);
		out.node.assign(nSeeds, 0); out.pos.assign(nSeeds, 0); out.support.assign(nSeeds, 0);
		out.locus_hits.clear(); out.locus_first_p.clear(); out.locus_last_p.clear(); out.n_loci.clear();
		if (byLocus)
		{
			out.locus_hits.assign(nSeeds, 0); out.locus_first_p.assign(nSeeds, 0); out.locus_last_p.assign(nSeeds, 0);
			out.n_loci.assign(nReads, 0);
		}
		out.kernel_ms = 0;
		if (nReads == 0) return 0;
		HIP_OK(hipSetDevice(device));
		// the batch: characters (every read at a multiple of 16 with 16 bytes of padding behind it), read records, the hand-out order
		std::vector<gas::SeedRead> recs(nReads);
		uint64_t seqBytes = 0;
		for (size_t i = 0; i < nReads; i++)
		{
			if (lens[i] > 0xfffffff0ull) return GA_E_INVALID;
			recs[i] = gas::SeedRead{seqBytes, (uint32_t)lens[i], 0};
			seqBytes += ((lens[i] + 15) & ~(size_t)15) + 16;
		}
		std::vector<uint32_t> order(nReads);
		for (size_t i = 0; i < nReads; i++) order[i] = (uint32_t)i;
		std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return lens[a] > lens[b]; });
		auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
		const size_t oSeq = 0, oRecs = up(seqBytes), oOrder = oRecs + up(nReads * sizeof(gas::SeedRead)), oNext = oOrder + up(nReads * 4);      // (oNext: end of the uploaded part)
		const size_t oOutN = oNext, oOutSeed = oOutN + up(nReads * 12), oOutLocus = oOutSeed + up(nSeeds * 12);
		const size_t oOutNLoci = oOutLocus + (byLocus ? up(nSeeds * 12) : 0), total = oOutNLoci + (byLocus ? up(nReads * 4) : 0);
		std::shared_ptr<char> host = owner->hostBlock(oNext);
		if (!host) return GA_E_DEVICE;
		memset(host.get(), 0, oNext);
		for (size_t i = 0; i < nReads; i++) memcpy(host.get() + recs[i].off, seqs[i], lens[i]);
		memcpy(host.get() + oRecs, recs.data(), nReads * sizeof(gas::SeedRead));
		memcpy(host.get() + oOrder, order.data(), nReads * 4);
		if (int st = work.ensure(total, total + total / 8)) return st;
		uint8_t* w = (uint8_t*)work.p;
		gas::SeedLaunch L;
		uint32_t slots = 0;
		const SeedIo io{w + oSeq, (const gas::SeedRead*)(w + oRecs), (const uint32_t*)(w + oOrder), (uint32_t*)(w + oOutN), (uint32_t*)(w + oOutSeed), (uint32_t*)(w + oOutLocus), (uint32_t*)(w + oOutNLoci)};
		if (int st = prepareLaunch(L, slots, p, nReads, byLocus, io)) return st;
		if (int st = ev.create()) return st;
		HIP_OK(hipMemcpyAsync(w, host.get(), oNext, hipMemcpyHostToDevice, 0));
		HIP_OK(hipMemsetAsync(w + oNext, 0, total - oNext, 0));
		HIP_OK(hipEventRecord(ev[0], 0));
		launch(L, slots, byLocus, 0);
		HIP_OK(hipEventRecord(ev[1], 0));
		std::vector<uint32_t> outN(nReads * 3), outSeed(nSeeds * 3);
		HIP_OK(hipMemcpy(outN.data(), w + oOutN, outN.size() * 4, hipMemcpyDeviceToHost));
		HIP_OK(hipMemcpy(outSeed.data(), w + oOutSeed, outSeed.size() * 4, hipMemcpyDeviceToHost));
		HIP_OK(hipEventSynchronize(ev[1]));
		float ms = 0;
		if (int st = ev.elapsed(0, 1, ms)) return st;
		out.kernel_ms = ms;
		unpack3(outN, out.n_seeds, out.n_hits, out.truncated);
		unpack3(outSeed, out.node, out.pos, out.support);
		if (byLocus)
		{
			std::vector<uint32_t> outLocus(nSeeds * 3);
			HIP_OK(hipMemcpy(outLocus.data(), w + oOutLocus, outLocus.size() * 4, hipMemcpyDeviceToHost));
			HIP_OK(hipMemcpy(out.n_loci.data(), w + oOutNLoci, nReads * 4, hipMemcpyDeviceToHost));
			unpack3(outLocus, out.locus_hits, out.locus_first_p, out.locus_last_p);
		}
		return 0;
	}
};

}  // namespace gasd
