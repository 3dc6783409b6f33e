// ga_seed_host.cpp -- the seeding entry points of include/graphaligner_amd.h: parameter checks, the nodes' linear coordinate, and the
// translation between the back end's node indices and the ga_seed_t triples ga_align_batch takes.  The work itself is the back end's
// (GaSeedEngine: ga_seed.h on gfx950).  A translation unit of its own: the alignment-only host emulation of tests/emul links without it.
#include <cstdlib>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "../../include/graphaligner_amd.h"
#include "ga_backend.h"

namespace {

struct SeedSetOwner
{
	ga_seed_set_t pub;
	std::vector<size_t> offsets;
	std::vector<ga_seed_t> seeds;
	std::vector<uint32_t> support, nHits;
	std::vector<uint8_t> truncated;
	std::vector<uint32_t> locusHits, locusFirstP, locusLastP, nLoci;        // ga_find_seeds_loci only
};

bool paramsOk(const ga_seed_params_t& p)
{
	return p.k >= 11 && p.k <= 31 && p.sample_shift <= 8 && p.max_hits >= 1 && p.max_hits <= 65536 && p.max_seeds >= 1 && p.max_seeds <= 64;
}

// engine of an uploaded graph, or the status that says why there is none
int engineOf(const ga_graph_t* g, GaGraphView& v, GaSeedEngine** e)
{
	if (!g) return GA_E_INVALID;
	v = ga_graph_view(g);
	if (!v.finalized) return GA_E_NOT_FINALIZED;
	if (!v.device) return GA_E_NO_DEVICE;
	*e = v.device->seedEngine();
	return *e ? GA_S_OK : GA_E_NO_DEVICE;
}

}  // namespace

extern "C" {

void ga_seed_params_default(ga_seed_params_t* p)
{
	if (!p) return;
	p->k = 15; p->sample_shift = 2; p->max_occ = 8; p->max_hits = 4096; p->window = 1024; p->diag_tol = 64; p->min_support = 2; p->max_seeds = 2;
}

// max_walks 0: the in-node index
static int buildIndex(ga_graph_t* g, uint32_t k, uint32_t sample_shift, uint32_t max_walks)
{
	GaGraphView v;
	GaSeedEngine* e = nullptr;
	if (int s = engineOf(g, v, &e)) return s;
	if (k < 11 || k > 31 || sample_shift > 8) return GA_E_INVALID;
	// the linear coordinate: bigraph nodes (digraph id >> 1) laid end to end in the order they were added; a reverse copy runs backwards
	const std::vector<uint64_t>& start = v.flat->node_start;
	const size_t n = start.size() - 1;
	std::vector<int64_t> linx(n, 0);
	std::unordered_map<int64_t, int64_t> cum;
	int64_t run = 0;
	for (size_t i = 1; i + 1 < n; i++)
	{
		const int64_t id = (*v.ids)[i], len = (int64_t)(start[i + 1] - start[i]);
		auto it = cum.find(id >> 1);
		if (it == cum.end()) { it = cum.emplace(id >> 1, run).first; run += len; }
		const int64_t lin = (id & 1) ? -(it->second + len - 1) : it->second;
		linx[i] = lin * 2 + (id & 1);
	}
	return max_walks ? e->buildWalks(k, sample_shift, max_walks, linx) : e->build(k, sample_shift, linx);
}

int ga_graph_build_seed_index(ga_graph_t* g, uint32_t k, uint32_t sample_shift) { return buildIndex(g, k, sample_shift, 0); }

int ga_graph_build_seed_index_walks(ga_graph_t* g, uint32_t k, uint32_t sample_shift, uint32_t max_walks)
{
	if (max_walks < 1 || max_walks > 256) return GA_E_INVALID;
	return buildIndex(g, k, sample_shift, max_walks);
}

int ga_graph_seed_index_walk_stats(const ga_graph_t* g, ga_seed_walk_stats_t* out)
{
	GaGraphView v;
	GaSeedEngine* e = nullptr;
	if (int s = engineOf(g, v, &e)) return s;
	if (!out || !e->built()) return GA_E_INVALID;
	const GaSeedWalkInfo w = e->walkInfo();
	if (w.max_walks == 0) return GA_E_INVALID;                               // an in-node index
	out->tail_starts = w.tail_starts; out->tail_starts_skipped = w.tail_starts_skipped; out->walk_kmers = w.walk_kmers;
	out->duplicates_dropped = w.duplicates_dropped; out->max_walks = w.max_walks; out->reserved = 0;
	return GA_S_OK;
}

int ga_graph_seed_index_stats(const ga_graph_t* g, ga_seed_index_stats_t* out)
{
	GaGraphView v;
	GaSeedEngine* e = nullptr;
	if (int s = engineOf(g, v, &e)) return s;
	if (!out || !e->built()) return GA_E_INVALID;
	const GaSeedIndexInfo inf = e->info();
	const std::vector<uint64_t>& start = v.flat->node_start;
	uint64_t seen = 0;
	for (size_t i = 1; i + 2 < start.size(); i++) { const uint64_t len = start[i + 1] - start[i]; if (len >= inf.k) seen += len - inf.k + 1; }
	out->kmers_seen = seen + e->walkInfo().walk_kmers;                       // (0 for an in-node index)
	out->entries = inf.entries; out->distinct_keys = inf.distinct_keys; out->bytes = inf.bytes; out->build_ms = inf.build_ms;
	out->k = inf.k; out->sample_shift = inf.sample_shift;
	return GA_S_OK;
}

int ga_graph_set_seed_coordinate(ga_graph_t* g, int kind)
{
	GaGraphView v;
	GaSeedEngine* e = nullptr;
	if (int s = engineOf(g, v, &e)) return s;
	if (!e->built() || (kind != GA_SEED_COORD_FILE_ORDER && kind != GA_SEED_COORD_TOPOLOGY)) return GA_E_INVALID;
	GaSeedCoordInfo c;
	return e->setCoordinate(kind, c);
}

int ga_graph_seed_coord_stats(const ga_graph_t* g, ga_seed_coord_stats_t* out)
{
	GaGraphView v;
	GaSeedEngine* e = nullptr;
	if (int s = engineOf(g, v, &e)) return s;
	if (!out || !e->built()) return GA_E_INVALID;
	const GaSeedCoordInfo c = e->coordInfo();
	out->kind = c.kind; out->trees = c.trees; out->cycles_cut = c.cycles_cut; out->cycle_rounds = c.cycle_rounds; out->depth_rounds = c.depth_rounds;
	out->reserved = 0; out->extent_sum = c.extent_sum; out->build_ms = c.build_ms;
	return GA_S_OK;
}

int ga_graph_seed_coordinate_copy(const ga_graph_t* g, int64_t* lin, size_t capacity)
{
	GaGraphView v;
	GaSeedEngine* e = nullptr;
	if (int s = engineOf(g, v, &e)) return s;
	if (!e->built() || (capacity && !lin)) return GA_E_INVALID;
	return e->copyLin(lin, capacity);
}

int ga_graph_seed_index_copy(const ga_graph_t* g, uint64_t* keys, uint32_t* node_indices, uint32_t* offsets, size_t capacity)
{
	GaGraphView v;
	GaSeedEngine* e = nullptr;
	if (int s = engineOf(g, v, &e)) return s;
	if (!e->built() || (capacity && (!keys || !node_indices || !offsets))) return GA_E_INVALID;
	return e->copy(keys, node_indices, offsets, capacity);
}

// the public set from the back end's per-slot arrays: node indices become (bigraph id, reverse)
static ga_seed_set_t* makeSeedSet(const GaGraphView& v, const GaSeedOut& r, uint32_t max_seeds, size_t n_reads, bool byLocus)
{
	SeedSetOwner* o = new SeedSetOwner();
	memset(&o->pub, 0, sizeof(o->pub));
	o->offsets.assign(n_reads + 1, 0);
	o->nHits.assign(r.n_hits.begin(), r.n_hits.end());
	o->truncated.assign(n_reads, 0);
	for (size_t i = 0; i < n_reads; i++)
	{
		o->truncated[i] = r.truncated[i] ? 1 : 0;
		for (uint32_t t = 0; t < r.n_seeds[i]; t++)
		{
			const size_t at = i * max_seeds + t;
			const int64_t id = (*v.ids)[r.node[at]];
			ga_seed_t sd;
			memset(&sd, 0, sizeof(sd));
			sd.node_id = id >> 1; sd.read_pos = r.pos[at]; sd.reverse = (int32_t)(id & 1);
			o->seeds.push_back(sd);
			o->support.push_back(r.support[at]);
			if (byLocus) { o->locusHits.push_back(r.locus_hits[at]); o->locusFirstP.push_back(r.locus_first_p[at]); o->locusLastP.push_back(r.locus_last_p[at]); }
		}
		o->offsets[i + 1] = o->seeds.size();
	}
	// (never null pointers, also for an empty set)
	o->seeds.reserve(1); o->support.reserve(1); o->nHits.reserve(1); o->truncated.reserve(1);
	o->pub.n_reads = n_reads; o->pub.seed_offsets = o->offsets.data(); o->pub.seeds = o->seeds.data(); o->pub.support = o->support.data();
	o->pub.n_hits = o->nHits.data(); o->pub.truncated = o->truncated.data(); o->pub.kernel_ms = r.kernel_ms;
	if (byLocus)
	{
		o->nLoci.assign(r.n_loci.begin(), r.n_loci.end());
		o->locusHits.reserve(1); o->locusFirstP.reserve(1); o->locusLastP.reserve(1); o->nLoci.reserve(1);
		o->pub.locus_hits = o->locusHits.data(); o->pub.locus_first_p = o->locusFirstP.data(); o->pub.locus_last_p = o->locusLastP.data(); o->pub.n_loci = o->nLoci.data();
	}
	return &o->pub;
}


// byLocus: ga_find_seeds_loci
static int findSeeds(const ga_graph_t* g, const ga_read_t* reads, size_t n_reads, const ga_seed_params_t* params, ga_seed_set_t** out, bool byLocus)
{
	GaGraphView v;
	GaSeedEngine* e = nullptr;
	if (int s = engineOf(g, v, &e)) return s;
	ga_seed_params_t p;
	ga_seed_params_default(&p);
	if (params) p = *params;
	if (!out || (n_reads && !reads) || !paramsOk(p) || !e->built()) return GA_E_INVALID;
	if (e->info().k != p.k || e->info().sample_shift != p.sample_shift) return GA_E_INVALID;
	std::vector<const char*> seqs(n_reads);
	std::vector<size_t> lens(n_reads);
	for (size_t i = 0; i < n_reads; i++) { seqs[i] = reads[i].sequence; lens[i] = reads[i].length; if (lens[i] && !seqs[i]) return GA_E_INVALID; }
	const GaSeedParams bp{p.k, p.sample_shift, p.max_occ, p.max_hits, p.window, p.diag_tol, p.min_support, p.max_seeds};
	GaSeedOut r;
	if (int s = byLocus ? e->findLoci(seqs.data(), lens.data(), n_reads, bp, r) : e->find(seqs.data(), lens.data(), n_reads, bp, r)) return s;
	*out = makeSeedSet(v, r, p.max_seeds, n_reads, byLocus);
	return GA_S_OK;
}

int ga_find_seeds(const ga_graph_t* g, const ga_read_t* reads, size_t n_reads, const ga_seed_params_t* params, ga_seed_set_t** out)
{
	return findSeeds(g, reads, n_reads, params, out, false);
}

int ga_find_seeds_loci(const ga_graph_t* g, const ga_read_t* reads, size_t n_reads, const ga_seed_params_t* params, ga_seed_set_t** out)
{
	return findSeeds(g, reads, n_reads, params, out, true);
}

// the seeds a batch of ga_batch_prepare_seeded was planned from, in the shape ga_find_seeds / ga_find_seeds_loci return them
int ga_batch_seeds(const ga_batch_t* b, ga_seed_set_t** out)
{
	if (!b || !out) return GA_E_INVALID;
	const GaBatchSeedView bv = ga_batch_seed_view(b);
	if (!bv.seeded) return GA_E_INVALID;
	const GaGraphView v = ga_graph_view(bv.g);
	const size_t n = bv.nReads, slots = n * bv.maxSeeds;
	GaSeedOut r;
	r.n_seeds.resize(n); r.n_hits.resize(n); r.truncated.resize(n);
	r.node.resize(slots); r.pos.resize(slots); r.support.resize(slots);
	for (size_t i = 0; i < n; i++) { r.n_seeds[i] = bv.outN[i * 3]; r.n_hits[i] = bv.outN[i * 3 + 1]; r.truncated[i] = bv.outN[i * 3 + 2]; }
	for (size_t i = 0; i < slots; i++) { r.node[i] = bv.outSeed[i * 3]; r.pos[i] = bv.outSeed[i * 3 + 1]; r.support[i] = bv.outSeed[i * 3 + 2]; }
	if (bv.byLocus)
	{
		r.locus_hits.resize(slots); r.locus_first_p.resize(slots); r.locus_last_p.resize(slots);
		for (size_t i = 0; i < slots; i++) { r.locus_hits[i] = bv.outLocus[i * 3]; r.locus_first_p[i] = bv.outLocus[i * 3 + 1]; r.locus_last_p[i] = bv.outLocus[i * 3 + 2]; }
		r.n_loci.assign(bv.outNLoci, bv.outNLoci + n);
	}
	r.kernel_ms = bv.kernel_ms;
	*out = makeSeedSet(v, r, bv.maxSeeds, n, bv.byLocus);
	return GA_S_OK;
}

void ga_seed_set_free(ga_seed_set_t* s)
{
	if (s) delete reinterpret_cast<SeedSetOwner*>(s);       // (pub is the owner's first member)
}

}  // extern "C"
