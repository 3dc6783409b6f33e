// ga_plan.h -- the job plan of a seeded batch, made on the device from the seeds the seeding kernel left in HBM (include/graphaligner_amd.h
// states the rule under ga_batch_prepare_seeded; DESIGN.md section 10c argues it).  It is what ga_batch_prepare does on the host, restated on
// node indices: per seed slot the reference's checks (getSplitAlignment, GraphAligner.h:2969-3024), the sizes of the backward and the forward
// job, and after two exclusive scans over the slots the GaJob, GaEqFill and GaPlanSeed records at their places.
//
// One function per launch and item, as in ga_seed.h: on gfx950 a kernel of ga_device.hip calls it for its wave or lane, the host build of
// tests/emul calls it for every item in turn.  Every loop is counted; no item waits for another.
#pragma once
#include "ga_backend.h"
#include "ga_seed.h"

namespace gap {

#ifdef GA_EMULATE
#define GAP_FN inline
#else
#define GAP_FN __device__ __forceinline__
#endif

constexpr uint32_t kNone = 0xffffffffu;

struct PlanLaunch
{
	const uint64_t* node_start;            // [n_nodes + 1] of the uploaded graph
	const uint32_t* twin;                  // [n_nodes] the node whose digraph id is this one's ^ 1; kNone: there is none
	const uint8_t* rev;                    // [n_nodes] digraph id & 1
	uint32_t n_nodes, n_reads, max_seeds, overlap;
	const uint8_t* seq;                    // the reads in the seeder's layout
	const gas::SeedRead* reads;
	const uint32_t* out_n;                 // the seeding kernel's outputs (ga_seed.h: SeedLaunch)
	const uint32_t* out_seed;
	uint32_t* first_bad;                   // [n_reads] first position whose character has no complement; kNone: none
	// per seed slot (read * max_seeds + t), [n_slots + 1]: rows of the two jobs before padding (0: no such job), then what the scans read
	// and write; element n_slots of the scans' outputs holds the totals
	uint32_t* n_bw; uint32_t* n_fw;
	uint32_t* slot_jobs; uint64_t* slot_rows;
	uint32_t* job_at; uint64_t* rows_at;
	GaPlanSeed* seeds;                     // [n_slots]
	GaJob* jobs; GaEqFill* fills; uint32_t* fill_read;    // [2 * n_slots]
	uint64_t* totals;                      // [2] jobs, rows
	uint64_t* eq; uint8_t* rows;           // the match words and row codes: plan_tail clears their slack behind the last job
};

GAP_FN uint64_t pad64(uint64_t n) { return (n + 63) / 64 * 64; }

// launch 1, one wave per read: this lane's share of the read, 16 bytes at a time (a read lies at a multiple of 16 with 16 bytes of padding
// behind it); the wave's minimum over its lanes is first_bad[read].  table: 256 entries, nonzero = the character has a complement
GAP_FN uint32_t first_bad_lane(const PlanLaunch& L, const uint8_t* table, uint32_t read, uint32_t lane)
{
	const gas::SeedRead r = L.reads[read];
	const uint32_t* s = (const uint32_t*)(L.seq + r.off);
	uint32_t bad = kNone;
	const uint32_t chunks = (r.len + 15) / 16;
	for (uint32_t c = lane; c < chunks; c += 64)
	{
		const uint32_t w[4] = {s[c * 4], s[c * 4 + 1], s[c * 4 + 2], s[c * 4 + 3]};
		for (uint32_t k = 0; k < 16; k++)
		{
			const uint32_t i = c * 16 + k;
			const uint8_t ch = (uint8_t)(w[k >> 2] >> ((k & 3) * 8));
			if (i < r.len && !table[ch] && i < bad) bad = i;
		}
	}
	return bad;
}

// what a slot adds to the two scans
GAP_FN void slot_sizes(uint32_t nBw, uint32_t nFw, uint32_t& jobs, uint64_t& rows)
{
	jobs = (nBw ? 1u : 0u) + (nFw ? 1u : 0u);
	rows = pad64(nBw) + pad64(nFw);
}

// launch 2, one lane per seed slot (and one for the scans' last element): the checks in the reference's order and the two job sizes
GAP_FN void plan_slot(const PlanLaunch& L, uint32_t s)
{
	const uint32_t nSlots = L.n_reads * L.max_seeds;
	if (s > nSlots) return;
	uint32_t nBw = 0, nFw = 0;
	if (s < nSlots)
	{
		const uint32_t read = s / L.max_seeds, t = s - read * L.max_seeds;
		GaPlanSeed ps{0, 0, 0, 0, -1, -1};
		if (t < L.out_n[read * 3])
		{
			const uint32_t n = L.out_seed[s * 3], p = L.out_seed[s * 3 + 1], len = L.reads[read].len;
			ps.pos = p;
			const uint32_t tw = n < L.n_nodes ? L.twin[n] : kNone;
			if (tw == kNone) ps.early = 3;                                       // GA_S_BAD_SEED
			else
			{
				ps.seed_node_index = L.rev[n] ? tw : n;
				if (!(p < len)) ps.early = 1;                                    // GA_S_ASSERTION
				else if (L.node_start[n + 1] - L.node_start[n] != L.node_start[tw + 1] - L.node_start[tw]) ps.early = 1;
				else
				{
					ps.valid = 1;
					if (p > 0)
					{
						// ReverseComplement asserts on a character outside its table anywhere in the prefix (CommonUtils.cpp:60-136)
						const uint64_t nb = (uint64_t)p + L.overlap;
						if ((uint64_t)len < nb || (uint64_t)L.first_bad[read] < nb) { ps.early = 1; ps.valid = 0; }
						else nBw = (uint32_t)nb;
					}
					if (ps.valid && p < len - 1) nFw = len - p;
				}
			}
		}
		L.seeds[s] = ps;
	}
	L.n_bw[s] = nBw; L.n_fw[s] = nFw;
	uint32_t jobs; uint64_t rows;
	slot_sizes(nBw, nFw, jobs, rows);
	L.slot_jobs[s] = jobs; L.slot_rows[s] = rows;
}

// launch 3, one lane per seed slot, after the scans: the slot's jobs and fills at the scanned places, backward before forward
GAP_FN void plan_write(const PlanLaunch& L, uint32_t s)
{
	const uint32_t nBw = L.n_bw[s], nFw = L.n_fw[s];
	if (!nBw && !nFw) return;
	const uint32_t read = s / L.max_seeds;
	const uint32_t n = L.out_seed[s * 3], p = L.out_seed[s * 3 + 1];
	const uint64_t seqOff = L.reads[read].off;
	uint32_t at = L.job_at[s];
	uint64_t ro = L.rows_at[s];
	if (nBw)
	{
		const uint32_t padded = (uint32_t)pad64(nBw);
		L.jobs[at] = GaJob{ro, padded, L.twin[n], nBw - L.overlap, 0};          // trace_rows = the seed's position (GraphAligner.h:3069)
		L.fills[at] = GaEqFill{seqOff, ro / 64, 0, nBw, padded, 1};
		L.fill_read[at] = read;
		L.seeds[s].bw_job = (int32_t)at;
		at++; ro += padded;
	}
	if (nFw)
	{
		const uint32_t padded = (uint32_t)pad64(nFw);
		L.jobs[at] = GaJob{ro, padded, n, nFw >= L.overlap ? nFw - L.overlap : 0u, 0};   // (:3051)
		L.fills[at] = GaEqFill{seqOff, ro / 64, p, nFw, padded, 0};
		L.fill_read[at] = read;
		L.seeds[s].fw_job = (int32_t)at;
	}
}

// launch 3's last item: the totals, and the slack behind the last job (one slice of match words, 128 row codes) cleared
GAP_FN void plan_tail(const PlanLaunch& L)
{
	const uint32_t nSlots = L.n_reads * L.max_seeds;
	const uint64_t rowsTotal = L.rows_at[nSlots];
	L.totals[0] = L.job_at[nSlots];
	L.totals[1] = rowsTotal;
	if (L.eq) for (uint32_t k = 0; k < 5; k++) L.eq[rowsTotal / 64 * 5 + k] = 0;
	if (L.rows) for (uint32_t k = 0; k < 16; k++) ((uint64_t*)(L.rows + rowsTotal))[k] = 0;
}

}  // namespace gap
