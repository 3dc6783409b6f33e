// ga_emul_plan.cpp -- TEST-ONLY (ga_emul.h): the first half of a seeded batch (ga_batch_prepare_seeded).  The seed engine finds the
// seeds, then the plan program of graphaligner_amd/csrc/ga_plan.h runs on the host launch by launch: first_bad_lane for the 64 lanes of
// every read's wave and their minimum, plan_slot for every slot, the two scans as running sums (what replaces the device library's
// scans here), plan_write for every slot and plan_tail; then the match words from the plan's fills, unless they are withheld.  The
// work arrays and the download's block are filled with a pattern before use.
#include <algorithm>
#include <chrono>
#include <cstring>

#include "ga_emul.h"
#include "../../graphaligner_amd/csrc/ga_plan.h"

using namespace gae;

namespace {

// the launches of DevBatch::beginSeeded between the seeding kernel and the match words, a launch = a loop over its items
void runPlan(gap::PlanLaunch& L, const uint8_t* hasComplement)
{
	const uint32_t nSlots = L.n_reads * L.max_seeds;
	for (uint32_t r = 0; r < L.n_reads; r++)
	{
		uint32_t bad = gap::kNone;
		for (uint32_t lane = 0; lane < 64; lane++) bad = std::min(bad, gap::first_bad_lane(L, hasComplement, r, lane));
		L.first_bad[r] = bad;
	}
	for (uint32_t s = 0; s <= nSlots; s++) gap::plan_slot(L, s);
}
void runLayout(gap::PlanLaunch& L)
{
	const uint32_t nSlots = L.n_reads * L.max_seeds;
	uint32_t jobs = 0;
	uint64_t rows = 0;
	for (uint32_t s = 0; s <= nSlots; s++) { L.job_at[s] = jobs; L.rows_at[s] = rows; jobs += L.slot_jobs[s]; rows += L.slot_rows[s]; }
	for (uint32_t s = 0; s < nSlots; s++) gap::plan_write(L, s);
	gap::plan_tail(L);
}

struct PlanArrays
{
	std::vector<uint32_t> firstBad, nBw, nFw, slotJobs, jobAt;
	std::vector<uint64_t> slotRows, rowsAt;
	void attach(gap::PlanLaunch& L, size_t nReads, size_t nSlots)
	{
		firstBad.assign(nReads + 1, 0xa5a5a5a5u); nBw.assign(nSlots + 1, 0xa5a5a5a5u); nFw = nBw; slotJobs = nBw; jobAt = nBw;
		slotRows.assign(nSlots + 1, 0xa5a5a5a5a5a5a5a5ull); rowsAt = slotRows;
		L.first_bad = firstBad.data(); L.n_bw = nBw.data(); L.n_fw = nFw.data(); L.slot_jobs = slotJobs.data(); L.job_at = jobAt.data();
		L.slot_rows = slotRows.data(); L.rows_at = rowsAt.data();
	}
};

}  // namespace

GaBackendBatch* EmulGraph::beginSeededBatch(const GaSeededRequest& req, GaSeededPlan& plan, int* status)
{
	if (without & NO_SEEDED) return GaBackendGraph::beginSeededBatch(req, plan, status);
	GaSeedEngine* eng = seedEngine();
	if (!eng || !eng->built()) { *status = 100; return nullptr; }
	const size_t nReads = req.nReads, nSlots = nReads * req.p.max_seeds;
	const gas::SeedRead* recs = (const gas::SeedRead*)(req.block + req.oRecs);
	std::vector<const char*> seqs(nReads);
	std::vector<size_t> lens(nReads);
	for (size_t i = 0; i < nReads; i++) { seqs[i] = req.block + recs[i].off; lens[i] = recs[i].len; }
	GaSeedOut so;
	if (int s = req.byLocus ? eng->findLoci(seqs.data(), lens.data(), nReads, req.p, so) : eng->find(seqs.data(), lens.data(), nReads, req.p, so)) { *status = s; return nullptr; }
	// the download's block: the seeding kernel's outputs as the device lays them out, then the plan
	auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
	const size_t oOutN = 0, oOutSeed = oOutN + up(nReads * 12), oOutLocus = oOutSeed + up(nSlots * 12), oOutNLoci = oOutLocus + up(nSlots * 12);
	const size_t oTotals = oOutNLoci + up(nReads * 4), oSeeds = oTotals + 256, oJobs = oSeeds + up(nSlots * sizeof(GaPlanSeed));
	const size_t oFills = oJobs + up(2 * nSlots * sizeof(GaJob)), oFillRead = oFills + up(2 * nSlots * sizeof(GaEqFill)), bytes = oFillRead + up(2 * nSlots * 4);
	std::shared_ptr<char> keep = GaBackendGraph::hostBlock(bytes);
	if (!keep) { *status = 102; return nullptr; }
	char* h = keep.get();
	memset(h, 0xa5, bytes);
	uint32_t* outN = (uint32_t*)(h + oOutN); uint32_t* outSeed = (uint32_t*)(h + oOutSeed); uint32_t* outLocus = (uint32_t*)(h + oOutLocus); uint32_t* outNLoci = (uint32_t*)(h + oOutNLoci);
	for (size_t i = 0; i < nReads; i++) { outN[i * 3] = so.n_seeds[i]; outN[i * 3 + 1] = so.n_hits[i]; outN[i * 3 + 2] = so.truncated[i]; }
	for (size_t i = 0; i < nSlots; i++) { outSeed[i * 3] = so.node[i]; outSeed[i * 3 + 1] = so.pos[i]; outSeed[i * 3 + 2] = so.support[i]; }
	if (req.byLocus)
	{
		for (size_t i = 0; i < nSlots; i++) { outLocus[i * 3] = so.locus_hits[i]; outLocus[i * 3 + 1] = so.locus_first_p[i]; outLocus[i * 3 + 2] = so.locus_last_p[i]; }
		for (size_t i = 0; i < nReads; i++) outNLoci[i] = so.n_loci[i];
	}
	const auto t0 = std::chrono::steady_clock::now();
	gap::PlanLaunch L;
	memset(&L, 0, sizeof(L));
	L.node_start = flat.node_start.data(); L.twin = req.twin; L.rev = req.rev;
	L.n_nodes = (uint32_t)(flat.node_start.size() - 1); L.n_reads = (uint32_t)nReads; L.max_seeds = req.p.max_seeds; L.overlap = req.overlap;
	L.seq = (const uint8_t*)req.block; L.reads = recs; L.out_n = outN; L.out_seed = outSeed;
	PlanArrays work;
	work.attach(L, nReads, nSlots);
	L.seeds = (GaPlanSeed*)(h + oSeeds); L.jobs = (GaJob*)(h + oJobs); L.fills = (GaEqFill*)(h + oFills); L.fill_read = (uint32_t*)(h + oFillRead);
	L.totals = (uint64_t*)(h + oTotals);
	runPlan(L, req.hasComplement);
	runLayout(L);
	plan.keep = keep;
	plan.outN = outN; plan.outSeed = outSeed;
	if (req.byLocus) { plan.outLocus = outLocus; plan.outNLoci = outNLoci; }
	plan.seeds = L.seeds; plan.jobs = L.jobs; plan.fills = L.fills; plan.fillRead = L.fill_read; plan.badFills = nullptr;
	plan.nJobs = (size_t)L.totals[0]; plan.rowsTotal = L.totals[1];
	plan.seed_ms = so.kernel_ms;
	plan.plan_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	if (plan.rowsTotal > req.rowsBound) { *status = 102; return nullptr; }
	EmulBatch* b = new EmulBatch();
	b->g = this;
	b->seeded = true;
	if (buildsMatchWords())
	{
		// the match words from the fills as the plan left them (ga_eq_words_planned_kernel)
		GaEqSource src;
		src.seq = req.block; src.seqBytes = req.blockBytes;
		src.fills = L.fills; src.nFills = plan.nJobs;
		src.rowCode = req.rowCode; src.rowCodeRc = req.rowCodeRc; src.padCode = req.padCode;
		src.twin = req.twin;
		b->buildWords(src, (size_t)(plan.rowsTotal / 64 + 1) * 5);
		plan.badFills = b->bad.data();
	}
	*status = 0;
	return b;
}

// component hook: the layout step (slot_sizes, the two scans, plan_write, plan_tail) over fabricated job sizes, no sequences: per slot the
// rows before padding of its backward and its forward job (0: none).  Out: per slot the rows_off and n_rows of either job (rows_off
// ~0: none) and the totals (jobs, rows).  tests/test_seed_plan.py feeds it sizes whose sum passes 2^32 rows.
extern "C" int ga_emul_seed_plan_layout(const uint32_t* nBw, const uint32_t* nFw, uint32_t nSlots, uint32_t overlap, uint64_t* bwRowsOff, uint64_t* fwRowsOff,
                                        uint32_t* bwRows, uint32_t* fwRows, uint64_t* totals)
{
	gap::PlanLaunch L;
	memset(&L, 0, sizeof(L));
	const gas::SeedRead rec{0, 0, 0};
	const uint32_t twin[1] = {0};
	std::vector<uint32_t> outSeed((size_t)nSlots * 3 + 3, 0);
	const uint64_t nodeStart[2] = {0, 1};
	L.node_start = nodeStart; L.twin = twin; L.n_nodes = 1; L.n_reads = 1; L.max_seeds = nSlots; L.overlap = overlap;
	L.reads = &rec; L.out_seed = outSeed.data();
	PlanArrays work;
	work.attach(L, 1, nSlots);
	std::vector<GaPlanSeed> seeds(nSlots + 1, GaPlanSeed{0, 0, 0, 1, -1, -1});
	std::vector<GaJob> jobs(2 * (size_t)nSlots + 1);
	std::vector<GaEqFill> fills(2 * (size_t)nSlots + 1);
	std::vector<uint32_t> fillRead(2 * (size_t)nSlots + 1);
	uint64_t tot[2] = {0, 0};
	L.seeds = seeds.data(); L.jobs = jobs.data(); L.fills = fills.data(); L.fill_read = fillRead.data(); L.totals = tot;
	for (uint32_t s = 0; s <= nSlots; s++)
	{
		L.n_bw[s] = s < nSlots ? nBw[s] : 0; L.n_fw[s] = s < nSlots ? nFw[s] : 0;
		gap::slot_sizes(L.n_bw[s], L.n_fw[s], L.slot_jobs[s], L.slot_rows[s]);
	}
	runLayout(L);
	for (uint32_t s = 0; s < nSlots; s++)
	{
		bwRowsOff[s] = seeds[s].bw_job >= 0 ? jobs[seeds[s].bw_job].rows_off : ~0ull;
		fwRowsOff[s] = seeds[s].fw_job >= 0 ? jobs[seeds[s].fw_job].rows_off : ~0ull;
		bwRows[s] = seeds[s].bw_job >= 0 ? jobs[seeds[s].bw_job].n_rows : 0;
		fwRows[s] = seeds[s].fw_job >= 0 ? jobs[seeds[s].fw_job].n_rows : 0;
	}
	totals[0] = tot[0]; totals[1] = tot[1];
	return 0;
}
