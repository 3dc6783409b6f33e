// ga_emul_sites.cpp -- TEST-ONLY: the site-query program of graphaligner_amd/csrc/ga_sites.h compiled for the host with GA_EMULATE, wave
// by wave, behind a component hook for tests/test_pileup_sites.py (fabricated planes and tables), and a STUB back end that keeps pileups
// in host memory and answers GaBackendPileup::sites with that same program, so that the product's host code (ga_host.cpp: params
// validation, the fold table and its preconditions, the records' fields, ga_sites_free) runs in front of it without a device.  A library
// of its own (tests/emul/sites.mk -> tests/_build/libga_sites_emul.so) next to the back end's emulation, which has no pileups and stays as
// it is; tests/emul/sites_check.cpp includes this file and runs the same code stand-alone under the sanitizers.  The buffers the program
// writes (mask, counts, records) are of exactly the sizes the product takes, with guard words behind them.
// Never shipped, never loaded by graphaligner_amd/.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../graphaligner_amd/csrc/ga_sites.h"
#include "../../graphaligner_amd/csrc/ga_host.h"

namespace {

constexpr uint64_t kSiteGuard = 0xDEADBEEFCAFEF00Dull;

// the two launches and the scan between them, as the product issues them (ga_device.hip: DevPileup::sitesWith), over `nWaves` waves
int emulSites(gast::SitesLaunch L, uint64_t maxSites, uint32_t nWaves, std::vector<GaSiteRec>& recs, uint64_t& total)
{
	recs.clear();
	total = 0;
	if (L.first > L.entries || L.n > L.entries - L.first || !L.alt_den || !nWaves) return GA_E_INVALID;
	if (!L.n) return 0;
	L.n_tiles = (L.n + gast::kTile - 1) / gast::kTile;
	const size_t nT = (size_t)L.n_tiles, guards = 8;
	std::vector<uint64_t> mask(nT * gast::kRounds + guards, kSiteGuard), counts(nT + 1 + guards, kSiteGuard), offsets(nT + 1, 0);
	counts[nT] = 0;
	L.mask = mask.data(); L.counts = counts.data(); L.offsets = offsets.data();
	gast::SitesLds lds;
	memset(&lds, 0xA5, sizeof(lds));
	for (uint32_t w = 0; w < nWaves; w++) gast::mark_wave(L, lds, w, nWaves);
	for (size_t k = 0; k < guards; k++) if (mask[nT * gast::kRounds + k] != kSiteGuard || counts[nT + 1 + k] != kSiteGuard) return GA_E_DEVICE;
	for (size_t t = 0; t < nT; t++) { if (counts[t] > gast::kTile) return GA_E_DEVICE; offsets[t + 1] = offsets[t] + counts[t]; }
	total = offsets[nT];
	const uint64_t nRecs = maxSites ? std::min(total, maxSites) : total;
	std::vector<GaSiteRec> out((size_t)nRecs + guards);
	memset(out.data(), 0xEE, out.size() * sizeof(GaSiteRec));
	L.recs = out.data(); L.n_recs = nRecs;
	// (the waves in another order than the marking launch's: the places come from the scan, not from who runs first)
	if (nRecs) for (uint32_t w = nWaves; w-- > 0;) gast::write_wave(L, w, nWaves);
	for (size_t k = 0; k < guards; k++) if (out[(size_t)nRecs + k].entry != 0xEEEEEEEEEEEEEEEEull) return GA_E_DEVICE;
	out.resize((size_t)nRecs);
	recs.swap(out);
	return 0;
}

}  // namespace

extern "C" uint32_t ga_emul_sites_tile() { return gast::kTile; }

// component hook: the program over fabricated planes ([nPlanes][entries]) and tables.  kind: 8 BASES, 1 DEPTH, 32 EDGES.  nodeStart
// [nNodes + 1] and foldTable [nNodes] (ga_backend.h: GA_FOLD_*) for a fold over columns, mirror [entries] for a fold over EDGES.
// params: flags, alt_num, alt_den, then min_depth, min_alt, first, n, max_sites.  recs: room for `cap` records of 10 words (entry low,
// entry high, the eight counts).  Returns the records written, or -1; *total = the sites found.
extern "C" long ga_emul_sites_query(const uint32_t* planes, uint64_t entries, uint32_t kind, uint32_t nNodes, const uint64_t* nodeStart, const uint32_t* foldTable,
                                    const uint32_t* mirror, const uint32_t* params32, const uint64_t* params64, uint32_t nWaves, uint32_t* recs, uint64_t cap, uint64_t* total)
{
	gast::SitesLaunch L;
	memset(&L, 0, sizeof(L));
	L.planes = planes; L.entries = entries; L.kind = kind; L.nPlanes = ga_pileup_planes_of_kind((int)kind);
	if (!L.nPlanes) return -1;
	L.fold = params32[0] & 1u; L.n_nodes = nNodes; L.node_start = nodeStart; L.fold_table = foldTable; L.mirror = mirror;
	if (L.fold && (kind == GA_KIND_EDGES ? !mirror : (!nodeStart || !foldTable || !nNodes))) return -1;
	L.alt_num = params32[1]; L.alt_den = params32[2];
	L.min_depth = params64[0]; L.min_alt = params64[1]; L.first = params64[2]; L.n = params64[3];
	std::vector<GaSiteRec> got;
	uint64_t n = 0;
	if (emulSites(L, params64[4], nWaves, got, n) != 0) return -1;
	*total = n;
	if (got.size() > cap) return -1;
	static_assert(sizeof(GaSiteRec) == 40, "a record is ten words");
	if (!got.empty()) memcpy(recs, got.data(), got.size() * sizeof(GaSiteRec));
	return (long)got.size();
}

// ---- the stub back end: no device behind it.  Pileups in host memory, sized as the spec says; site queries through the program above ----
namespace {
struct StubSitesGraph;
struct StubSitesPileup : GaBackendPileup
{
	const StubSitesGraph* g = nullptr;
	uint32_t kind = 0, nPlanes = 0;
	uint64_t entries = 0;
	std::vector<uint32_t> words, mirror;
	int reset() override { std::fill(words.begin(), words.end(), 0u); return 0; }
	int download(uint64_t first, uint64_t n, uint32_t* out) const override
	{
		if (first > entries || n > entries - first) return GA_E_INVALID;
		for (uint32_t k = 0; k < nPlanes; k++) std::copy(words.begin() + (size_t)(k * entries + first), words.begin() + (size_t)(k * entries + first + n), out + (size_t)k * n);
		return 0;
	}
	int sites(const GaSiteQuery& q, GaSitesOut& out) override;
};
struct StubSitesGraph : GaBackendGraph
{
	GaFlatGraph flat;
	bool codesPileup() const override { return true; }
	GaBackendPileup* createPileup(const GaPileupSpec& spec, int* status) override
	{
		*status = GA_E_INVALID;
		if (!spec.planes || spec.planes != ga_pileup_planes_of_kind(spec.kind) || spec.entries != ga_pileup_entries(spec.kind, flat.node_start.back(), ga_edge_slot_count(flat))) return nullptr;
		if (spec.kind == GA_KIND_EDGES && !spec.mirrorSlot) return nullptr;
		StubSitesPileup* p = new StubSitesPileup();
		p->g = this; p->kind = (uint32_t)spec.kind; p->nPlanes = spec.planes; p->entries = spec.entries;
		p->words.assign((size_t)spec.planes * spec.entries, 0u);
		if (spec.kind == GA_KIND_EDGES) p->mirror.assign(spec.mirrorSlot, spec.mirrorSlot + spec.entries);
		*status = 0;
		return p;
	}
};
int StubSitesPileup::sites(const GaSiteQuery& q, GaSitesOut& out)
{
	out = GaSitesOut();
	const bool edges = kind == (uint32_t)GA_KIND_EDGES;
	const uint32_t nNodes = (uint32_t)g->flat.node_start.size() - 1;
	if (q.fold && !edges && (!q.foldTable || q.nNodes != nNodes)) return GA_E_INVALID;
	gast::SitesLaunch L;
	memset(&L, 0, sizeof(L));
	// (copies of exactly the tables' sizes: a read past one of them is a read past an allocation)
	std::vector<uint32_t> planes(words), fold;
	std::vector<uint64_t> nodeStart(g->flat.node_start);
	if (q.fold && !edges) fold.assign(q.foldTable, q.foldTable + q.nNodes);
	L.planes = planes.data(); L.entries = entries; L.kind = kind; L.nPlanes = nPlanes;
	L.fold = q.fold ? 1u : 0u; L.n_nodes = nNodes; L.node_start = nodeStart.data(); L.fold_table = fold.data(); L.mirror = mirror.data();
	L.first = q.first; L.n = q.n; L.min_depth = q.min_depth; L.min_alt = q.min_alt; L.alt_num = q.alt_num; L.alt_den = q.alt_den;
	return emulSites(L, q.max_sites, 3, out.recs, out.n_total);
}
}  // namespace

GaBackendGraph* ga_backend_upload_graph(const GaFlatGraph& flat, const GaHmmTables&, int device, int* status)
{
	if (device != 0) { *status = GA_E_NO_DEVICE; return nullptr; }
	StubSitesGraph* g = new StubSitesGraph();
	g->flat = flat;
	*status = 0;
	return g;
}
GaBackendBatch* ga_backend_create_batch(GaBackendGraph*, GaRowsProvider, const uint64_t*, const GaEqSource*, size_t, const std::vector<GaJob>&, const GaRunConfig&, int* status)
{
	*status = GA_E_NO_DEVICE;
	return nullptr;
}

// sets the counters of a pileup made on the stub back end: words[plane * entries + entry]
extern "C" int ga_emul_sites_poke(ga_pileup_t* p, const uint32_t* words, uint64_t n)
{
	StubSitesPileup* s = p ? dynamic_cast<StubSitesPileup*>(p->dev) : nullptr;
	if (!s || n != s->words.size()) return GA_E_INVALID;
	std::copy(words, words + n, s->words.begin());
	return 0;
}
