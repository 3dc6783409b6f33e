// ga_dev.h -- what the parts of the device back end share: the owners of what a stage borrows (events, a stream, blocks of the graph's
// block list, a device allocation of its own: DevBuf, GrownBuf), the scan and the sort in their two steps, the graph and the pileup as
// they lie in HBM, and what every stage of a batch uses (BatchCore).
// The stages themselves, each with its own state, are in ga_dev_prepare.h, ga_dev_ladder.h and ga_dev_post.h; the seed engine, which the
// graph holds, is ga_dev_seed.h, included here between the owners and the graph.
// Not a header for others: a part of ga_device.hip's translation unit, included once below its kernels.
#ifndef GA_DEVICE_PARTS
#error "ga_dev.h is a part of ga_device.hip"
#endif

namespace {

#define HIP_OK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { fprintf(stderr, "graphaligner_amd: %s failed: %s\n", #call, hipGetErrorString(e_)); return GA_E_DEVICE; } } while (0)

// a group of events: made at first use, destroyed with their owner (or sooner, by destroy())
template <int N> struct Events
{
	hipEvent_t e[N] = {};
	~Events() { destroy(); }
	int create() { for (hipEvent_t& x : e) if (!x) HIP_OK(hipEventCreate(&x)); return 0; }
	void destroy() { for (hipEvent_t& x : e) if (x) { hipEventDestroy(x); x = nullptr; } }
	hipEvent_t operator[](int i) const { return e[i]; }
	int elapsed(int i, int j, float& ms) const { HIP_OK(hipEventElapsedTime(&ms, e[i], e[j])); return 0; }
};
// a stream, destroyed with its owner (declared before the owner's events and blocks: it goes last)
struct Stream
{
	hipStream_t s = nullptr;
	~Stream() { if (s) hipStreamDestroy(s); }
	// (non-blocking: a copy or a kernel on it must not wait for another batch's kernel through the null stream)
	int create() { if (!s) HIP_OK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); return 0; }
	operator hipStream_t() const { return s; }
};

// rocprim's exclusive sum over n elements in its two steps: size() asks for the bytes of temporary storage, run() puts the scan on the stream
template <typename T> struct Scan
{
	T* in; T* out; size_t n;
	size_t tmpBytes = 0;
	int size(hipStream_t stream) { HIP_OK(rocprim::exclusive_scan(nullptr, tmpBytes, in, out, (T)0, n, rocprim::plus<T>(), stream)); return 0; }
	int run(void* tmp, hipStream_t stream) { HIP_OK(rocprim::exclusive_scan(tmp, tmpBytes, in, out, (T)0, n, rocprim::plus<T>(), stream)); return 0; }
};
// rocprim's stable sort of n (key, value) pairs by the keys' bits [0, bits), in the same two steps
template <typename K, typename V> struct SortPairs
{
	K* keysIn; K* keysOut; V* valsIn; V* valsOut; size_t n; unsigned bits;
	size_t tmpBytes = 0;
	int size(hipStream_t stream) { HIP_OK(rocprim::radix_sort_pairs(nullptr, tmpBytes, keysIn, keysOut, valsIn, valsOut, n, 0u, bits, stream)); return 0; }
	int run(void* tmp, hipStream_t stream) { HIP_OK(rocprim::radix_sort_pairs(tmp, tmpBytes, keysIn, keysOut, valsIn, valsOut, n, 0u, bits, stream)); return 0; }
};

// one temporary device allocation of the seed engine (ga_dev_seed.h), freed when its scope ends, sooner by reset(), or handed over by
// release().  Straight from hipMalloc and back to hipFree, not from the graph's block list: an index build holds tens of bytes per entry
// for a moment, and the block list would keep such blocks idle (and never frees on a failed build).
template <typename T> struct DevBuf
{
	T* p = nullptr;
	DevBuf() = default;
	DevBuf(const DevBuf&) = delete;
	DevBuf& operator=(const DevBuf&) = delete;
	~DevBuf() { reset(); }
	int alloc(size_t count)
	{
		reset();
		void* q = nullptr;
		HIP_OK(hipMalloc(&q, count * sizeof(T)));
		p = (T*)q;
		return 0;
	}
	void reset() { if (p) hipFree(p); p = nullptr; }
	T* release() { T* q = p; p = nullptr; return q; }
	operator T*() const { return p; }
};
// a device buffer kept between calls and grown when needed: ensure() frees and reallocates only when the buffer is too small (then to
// `room` bytes where that is more: head room), freed with its owner
struct GrownBuf
{
	void* p = nullptr;
	size_t bytes = 0;
	GrownBuf() = default;
	GrownBuf(const GrownBuf&) = delete;
	GrownBuf& operator=(const GrownBuf&) = delete;
	~GrownBuf() { if (p) hipFree(p); }
	int ensure(size_t need, size_t room = 0)
	{
		if (need <= bytes) return 0;
		if (p) hipFree(p);
		p = nullptr; bytes = 0;
		void* q = nullptr;
		HIP_OK(hipMalloc(&q, std::max(need, room)));
		p = q; bytes = std::max(need, room);
		return 0;
	}
};

// pinned host blocks for the batches' copies of the reads (page-locking half a GB per batch costs more than copying it): a block goes
// back to the pool when the last holder -- the batch, or results whose edit sequences point into it -- lets go of it
struct PinnedPool
{
	std::mutex lock;
	std::vector<std::pair<size_t, char*>> idle;
	~PinnedPool() { for (auto& b : idle) hipHostFree(b.second); }
};

}  // namespace

// the seed engine: it uses the owners above, and the graph below holds one and needs the complete type
#include "ga_dev_seed.h"

namespace {

// the counters of one pileup: `nPlanes` planes of one 32-bit word per entry (ga_backend.h: a column, or a slot for the EDGES kind), in the
// HBM of the graph's device; the EDGES kind keeps its mirror-slot table next to them
struct DevGraph;
struct BlockLease;
struct DevPileup : GaBackendPileup
{
	DevGraph* g = nullptr;             // (a pileup is freed before its graph)
	int device = 0;
	uint32_t kind = 0, nPlanes = 0;
	uint64_t entries = 0;
	uint32_t* planes = nullptr;
	uint32_t* mirror = nullptr;
	~DevPileup() override { hipSetDevice(device); if (planes) hipFree(planes); if (mirror) hipFree(mirror); }
	size_t bytes() const { return (size_t)nPlanes * entries * 4; }
	int reset() override
	{
		// (the caller lets no add into this pileup run at the same time -- ga_pileup_reset holds the pileup exclusively -- and an add has
		// finished when addToPileup returns: the null stream alone is waited for, not the device with every other batch's kernels)
		HIP_OK(hipSetDevice(device));
		HIP_OK(hipMemsetAsync(planes, 0, bytes(), nullptr));
		HIP_OK(hipStreamSynchronize(nullptr));
		return 0;
	}
	int download(uint64_t first, uint64_t n, uint32_t* out) const override
	{
		if (first > entries || n > entries - first) return GA_E_INVALID;
		HIP_OK(hipSetDevice(device));
		// (an add has finished on its batch's stream when addToPileup returns: nothing to wait for)
		for (uint32_t k = 0; k < nPlanes && n; k++) HIP_OK(hipMemcpy(out + (size_t)k * n, planes + (size_t)k * entries + first, n * 4, hipMemcpyDeviceToHost));
		return 0;
	}
	// site queries (ga_dev_post.h)
	int sites(const GaSiteQuery& q, GaSitesOut& out) override;
	int sitesWith(const GaSiteQuery& q, GaSitesOut& out, BlockLease& blocks);
};

struct DevGraph : GaBackendGraph
{
	std::shared_ptr<PinnedPool> pinned = std::make_shared<PinnedPool>();
	bool buildsMatchWords() const override { return true; }
	bool codesOps() const override { return true; }
	bool codesPileup() const override { return true; }
	bool writesPathSeq() const override { return true; }
	GaBackendPileup* createPileup(const GaPileupSpec& spec, int* status) override
	{
		*status = GA_E_INVALID;
		const bool edges = spec.kind == GA_KIND_EDGES;
		if (spec.planes == 0 || spec.planes != ga_pileup_planes_of_kind(spec.kind) || spec.entries != ga_pileup_entries(spec.kind, totalBp, edgeSlots)) return nullptr;
		if (edges && (!spec.mirrorSlot || spec.entries >= 0xffffffffull)) return nullptr;
		*status = GA_E_DEVICE;
		if (hipSetDevice(device) != hipSuccess) return nullptr;
		std::unique_ptr<DevPileup> p(new DevPileup());
		p->g = this; p->device = device; p->kind = (uint32_t)spec.kind; p->nPlanes = spec.planes; p->entries = spec.entries;
		if (hipMalloc((void**)&p->planes, std::max<size_t>(p->bytes(), 16)) != hipSuccess) { p->planes = nullptr; (void)hipGetLastError(); return nullptr; }
		if (edges)
		{
			if (hipMalloc((void**)&p->mirror, std::max<size_t>((size_t)p->entries * 4, 16)) != hipSuccess) { p->mirror = nullptr; (void)hipGetLastError(); return nullptr; }
			if (p->entries && hipMemcpy(p->mirror, spec.mirrorSlot, (size_t)p->entries * 4, hipMemcpyHostToDevice) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
		}
		if (p->reset() != 0) return nullptr;
		*status = 0;
		return p.release();
	}
	std::shared_ptr<char> hostBlock(size_t bytes) override
	{
		const size_t two = (size_t)2 << 20;
		bytes = (bytes + two - 1) & ~(two - 1);
		std::shared_ptr<PinnedPool> pool = pinned;
		char* p = nullptr;
		size_t cap = 0;
		{
			std::lock_guard<std::mutex> guard(pool->lock);
			size_t best = pool->idle.size();
			for (size_t i = 0; i < pool->idle.size(); i++)
				if (pool->idle[i].first >= bytes && pool->idle[i].first <= 2 * bytes + two && (best == pool->idle.size() || pool->idle[i].first < pool->idle[best].first)) best = i;
			if (best != pool->idle.size()) { cap = pool->idle[best].first; p = pool->idle[best].second; pool->idle.erase(pool->idle.begin() + (long)best); }
		}
		if (!p)
		{
			hipSetDevice(device);
			if (hipHostMalloc((void**)&p, bytes, hipHostMallocDefault) != hipSuccess) return GaBackendGraph::hostBlock(bytes);      // (pageable memory: the upload is then a staged copy)
			cap = bytes;
		}
		return std::shared_ptr<char>(p, [pool, cap](char* q) {
			std::lock_guard<std::mutex> guard(pool->lock);
			if (pool->idle.size() < 6) pool->idle.emplace_back(cap, q); else hipHostFree(q);
		});
	}

	// seeding (ga_seed.h): the k-mer index of this graph and its buffers, built on request
	std::unique_ptr<gasd::DevSeedEngine> seed;
	GaSeedEngine* seedEngine() override { return seed.get(); }

	// seeded batches (ga_plan.h): twin[n] and digraph id & 1 per node, uploaded at the first seeded prepare, freed with the graph
	std::mutex twinLock;
	uint32_t* dTwin = nullptr;
	uint8_t* dRev = nullptr;
	uint32_t* dOpsTwin = nullptr;      // the twin table alone, for GA_F_OPS batches of ga_batch_prepare (uploaded at the first of them)
	// site queries (ga_sites.h): the per-node fold table, uploaded at the first fold query over a columns kind, freed with the graph; the
	// stream and the two events the queries run on (one query at a time: sitesLock)
	std::mutex sitesLock;
	uint32_t* dFold = nullptr;
	Stream sitesStream;
	Events<2> evS;
	GaBackendBatch* beginSeededBatch(const GaSeededRequest& req, GaSeededPlan& plan, int* status) override;

	int device = 0;
	GaDevGraph g;
	GaHmmTables* hmm = nullptr;
	std::vector<void*> allocs;
	int cus = 0;
	uint64_t totalBp = 0;
	uint64_t edgeSlots = 0;            // the in-neighbour lists' total length: the entries of a pileup of the EDGES kind
	// scratch pool owned by the graph: batches reuse it instead of allocating tens of GB each
	uint8_t* pool = nullptr;
	size_t poolBytes = 0;
	bool poolBusy = false;
	~DevGraph() override
	{
		hipSetDevice(device);
		for (void* p : allocs) hipFree(p);
		for (auto& b : idleBlocks) hipFree(b.second);
		if (pool) hipFree(pool);
		if (hostPool) hipHostFree(hostPool);
	}
	// device buffers of the batches (match words, jobs, outputs, trace pool): handed back here instead of hipFree'd, because hipFree
	// waits for the whole device -- i.e. for the kernels of whatever batch is running -- and the stages of consecutive batches are
	// meant to overlap (sharding.run_overlapped).  A later batch of similar size takes them again.  (Taken and given through a BlockLease.)
	std::mutex blockLock;
	std::vector<std::pair<size_t, void*>> idleBlocks;
	void* takeBlock(size_t bytes)
	{
		{
			std::lock_guard<std::mutex> lock(blockLock);
			size_t best = idleBlocks.size();
			for (size_t i = 0; i < idleBlocks.size(); i++)
				if (idleBlocks[i].first >= bytes && idleBlocks[i].first <= bytes + bytes / 2 + 4096 && (best == idleBlocks.size() || idleBlocks[i].first < idleBlocks[best].first)) best = i;
			if (best != idleBlocks.size())
			{
				void* p = idleBlocks[best].second;
				idleBlocks.erase(idleBlocks.begin() + (long)best);
				return p;
			}
		}
		void* p = nullptr;
		if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
		return p;
	}
	void giveBlock(void* p, size_t bytes)
	{
		std::lock_guard<std::mutex> lock(blockLock);
		// (bounded: beyond a few dozen idle blocks the oldest go back to the device)
		if (idleBlocks.size() >= 48) { hipFree(idleBlocks.front().second); idleBlocks.erase(idleBlocks.begin()); }
		idleBlocks.emplace_back(bytes, p);
	}
	// (one graph can serve batches run from several host threads: the pool changes hands under a lock)
	std::mutex poolLock;
	uint8_t* takePool(size_t bytes)
	{
		std::lock_guard<std::mutex> lock(poolLock);
		if (poolBusy) return nullptr;
		if (bytes > poolBytes)
		{
			if (pool) hipFree(pool);
			pool = nullptr; poolBytes = 0;
			if (hipMalloc((void**)&pool, bytes) != hipSuccess) { pool = nullptr; return nullptr; }
			poolBytes = bytes;
		}
		poolBusy = true;
		return pool;
	}
	void givePool() { std::lock_guard<std::mutex> lock(poolLock); poolBusy = false; }
	size_t poolBytesIfFree() { std::lock_guard<std::mutex> lock(poolLock); return poolBusy ? 0 : poolBytes; }
	// pinned host buffer for the moves on their way back (page-locking half a GB per batch would cost more than the copy)
	std::mutex hostLock;
	uint8_t* hostPool = nullptr;
	size_t hostPoolBytes = 0;
	bool hostPoolBusy = false;
	uint8_t* takeHost(size_t bytes)
	{
		std::lock_guard<std::mutex> lock(hostLock);
		if (hostPoolBusy) return nullptr;
		if (bytes > hostPoolBytes)
		{
			if (hostPool) hipHostFree(hostPool);
			hostPool = nullptr; hostPoolBytes = 0;
			const size_t want = bytes + bytes / 8;
			if (hipHostMalloc((void**)&hostPool, want, hipHostMallocDefault) != hipSuccess) { hostPool = nullptr; return nullptr; }
			hostPoolBytes = want;
		}
		hostPoolBusy = true;
		return hostPool;
	}
	void giveHost() { std::lock_guard<std::mutex> lock(hostLock); hostPoolBusy = false; }
	template <typename T> int put(const std::vector<T>& v, const T** out)
	{
		void* p = nullptr;
		HIP_OK(hipMalloc(&p, std::max<size_t>(v.size() * sizeof(T), 16)));
		allocs.push_back(p);
		HIP_OK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
		*out = (const T*)p;
		return 0;
	}
	// tables that go up when a stage first needs them and are freed with the graph: all of them over `stream`, one wait, then their
	// pointers are published.  The caller holds the lock that guards the pointers (twinLock, sitesLock).
	struct FirstUse { void** at; const void* host; size_t bytes; };
	int uploadOnce(std::initializer_list<FirstUse> tables, hipStream_t stream)
	{
		std::vector<void*> up;
		for (const FirstUse& t : tables)
		{
			void* p = nullptr;
			HIP_OK(hipMalloc(&p, std::max<size_t>(t.bytes, 16)));
			allocs.push_back(p);
			HIP_OK(hipMemcpyAsync(p, t.host, t.bytes, hipMemcpyHostToDevice, stream));
			up.push_back(p);
		}
		HIP_OK(hipStreamSynchronize(stream));
		size_t k = 0;
		for (const FirstUse& t : tables) *t.at = up[k++];
		return 0;
	}
};

// blocks of the graph's block list, held for a batch or for one stage of it; what is still held goes back when the lease ends.
// The one rule of giving back: nothing on the stream may still use the block.  A stage that went through has waited for its stream;
// one that failed may have left work on it, so a stage's lease ends in end(rc, stream), which waits first when rc says the stage failed.
// (The batch's own lease ends with the batch.  Each of its stages -- prepare, run, fetch -- has waited for the stream when it returns
// success, and the seeded prepare also when it fails after its first launch; what a stage hands back sooner, it hands back after its wait.)
struct BlockLease
{
	DevGraph* g;
	bool loud;                         // the batch's own allocations say when the device has no memory; site queries do not
	std::vector<std::pair<size_t, void*>> held;
	BlockLease(DevGraph* g, bool loud) : g(g), loud(loud) {}
	BlockLease(const BlockLease&) = delete;
	~BlockLease() { giveAll(); }
	template <typename T> int take(T** out, size_t count)
	{
		const size_t bytes = (std::max<size_t>(count * sizeof(T), 16) + 255) & ~(size_t)255;
		void* p = g->takeBlock(bytes);
		if (!p) { if (loud) fprintf(stderr, "graphaligner_amd: no device memory for %zu bytes\n", bytes); return GA_E_DEVICE; }
		held.emplace_back(bytes, p);
		*out = (T*)p;
		return 0;
	}
	// a block that its stage no longer needs, handed back before the lease ends
	void release(void* p)
	{
		for (size_t i = 0; i < held.size(); i++)
			if (held[i].second == p) { g->giveBlock(p, held[i].first); held.erase(held.begin() + (long)i); return; }
	}
	void giveAll() { for (auto& b : held) g->giveBlock(b.second, b.first); held.clear(); }
	int end(int rc, hipStream_t stream)
	{
		if (rc) (void)hipStreamSynchronize(stream);
		giveAll();
		return rc;
	}
};

// the few switches the library reads from the environment, once per batch: GA_LANES (1 / 0: force which kernel goes first -- the GPU
// parity tests run every case both ways), GA_DEBUG_PASSES (one line per launch on stderr) and two test hooks: the trace pool's size
// and a cap on the waves a launch starts
struct Knobs
{
	int lanes = -1;                 // -1: by graph shape
	int spread = 1;                 // 1: a small batch is spread over all wave slots; 0: full waves; k > 1: k jobs per wave (GA_LANES_SPREAD, for experiments)
	bool debugPasses = false;
	uint64_t tracePoolBytes = 0;    // 0: sized from the batch
	uint32_t waveSlots = 0;         // 0: as many waves as fit; k: no launch starts more than k (GA_TEST_WAVE_SLOTS: a wave then takes group after group / job after job)
	Knobs()
	{
		if (const char* e = getenv("GA_LANES")) lanes = atoi(e) != 0 ? 1 : 0;
		debugPasses = getenv("GA_DEBUG_PASSES") != nullptr;
		if (const char* e = getenv("GA_LANES_SPREAD")) spread = atoi(e);
		if (const char* t = getenv("GA_TEST_TRACE_POOL_BYTES")) tracePoolBytes = (uint64_t)atoll(t) & ~3ull;
		if (const char* e = getenv("GA_TEST_WAVE_SLOTS")) waveSlots = (uint32_t)std::max(atoi(e), 0);
	}
};

// a job whose moves are in the trace pool and count: it finished, it covers rows, and it is not marked as dropped
inline bool movesCount(const GaJobOut& o) { return o.status == GA_OK && o.n_valid > 0 && o.reserved3 != 1; }

// a batch, layer by layer: BatchCore here is what every stage uses; each part derives the next layer from the one before and keeps that
// stage's state next to its functions -- BatchPrepared (ga_dev_prepare.h), BatchLadder (ga_dev_ladder.h), DevBatch (ga_dev_post.h).  A
// stage sees the state of the stages before it and of none after it.  Destruction runs from DevBatch down: it sets the device first.
struct BatchCore : GaBackendBatch
{
	explicit BatchCore(DevGraph* g) : g(g), blocks(g, true) {}
	~BatchCore() override { if (outsLocked) hipHostUnregister(outs.data()); }      // (then the blocks, then the stream)
	DevGraph* g;
	Knobs knobs;
	Stream stream;
	BlockLease blocks;                 // the batch's device memory, from the graph's block list
	template <typename T> int alloc(T** out, size_t count) { return blocks.take(out, count); }
	std::vector<GaJob> jobs;
	GaRunConfig cfg;
	GaLaunch L;                        // what every pass shares (graph, reads, jobs, outputs, trace pool); scratch geometry is set per pass
	std::vector<GaJobOut> outs;        // the host copy of the output records, page-locked when outsLocked
	bool outsLocked = false;
	std::vector<uint32_t> orderHost;   // all jobs, longest first (the device queues hand them out in this order)
	Events<2> evPass;                  // around the kernel of the pass in hand
	uint32_t* dList = nullptr;         // job list of the current pass
	int uploadList(const std::vector<uint32_t>& list)
	{
		HIP_OK(hipMemcpyAsync(dList, list.data(), list.size() * 4, hipMemcpyHostToDevice, stream));
		return 0;
	}
};

}  // namespace

