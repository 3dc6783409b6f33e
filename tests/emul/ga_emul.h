// ga_emul.h -- TEST-ONLY: the one host emulation of the device programs (tests/_build/libga_emul.so).  The product's host code
// (ga_host.cpp, ga_vgio.cpp, ga_seed_host.cpp) is linked against this back end instead of ga_device.hip; every device header
// (ga_kernel.h, ga_lanes.h, ga_seed.h, ga_plan.h, ga_ops.h) is compiled for the host with GA_EMULATE and the wave primitives of
// ga_wave_emul.h, and what the product does by a kernel launch is a loop over the launch's items here.  One graph, one batch and one
// seed engine, split over a few files by subject:
//   ga_emul_backend.cpp  the graph and the batch, the switch below, the match words
//   ga_emul_ladder.cpp   EmulBatch::climb and launch: the passes of the product's ladder (ga_ladder.h), each a loop over its jobs
//   ga_emul_seed.cpp     the seed engine
//   ga_emul_plan.cpp     EmulGraph::beginSeededBatch: the plan of a seeded batch
//   ga_emul_ops.cpp      EmulBatch::codeOps: the operations of GA_F_OPS
//   ga_emul_hooks.cpp    component hooks for unit tests of pieces of ga_kernel.h, ga_sparse.h and ga_lanes.h
// Never shipped, never loaded by graphaligner_amd/.
#pragma once
#include <memory>
#include <vector>

#include "../../graphaligner_amd/csrc/ga_backend.h"
#include "../../graphaligner_amd/csrc/ga_ladder.h"

namespace gae {

// With nothing set the back end does what the product's does: the same passes over the same jobs (ga_ladder.h), with two intended
// differences -- its capacities are its own, and its first pass does not follow the graph's shape (GA_LANES=0: the wave-per-read
// kernel first; else the lanes = reads kernel, always from <10,64>, every later size for any number of jobs).  GA_EMUL_WITHOUT, read at every ga_backend_upload_graph, is a comma-separated
// list of capabilities that the graph and its batches withhold; a withheld capability answers what the interface's base class answers
// (ga_backend.h), so the tests can see how the host code and the Python layers behave in front of a back end that lacks it.
enum : uint32_t
{
	NO_WIDE = 1,           // wide: no run_job<4096,true> pass
	NO_WIDE_SPARSE = 2,    // wide_sparse: no run_job<4096,true,true> pass
	NO_WORDS = 4,          // words: the host builds the match words
	NO_OPS = 8,            // ops: GA_F_OPS is refused
	NO_SEEDING = 16,       // seeding: seedEngine() is null
	NO_WALKS = 32,         // walks: buildWalks, walkInfo
	NO_LOCI = 64,          // loci: findLoci
	NO_TOPOLOGY = 128,     // topology: setCoordinate, coordInfo, copyLin
	NO_SEEDED = 256,       // seeded: beginSeededBatch
};

GaSeedEngine* newSeedEngine(const GaDevGraph* g, uint32_t without);
struct KeptBuffers;

struct EmulGraph : GaBackendGraph
{
	GaFlatGraph flat;
	std::vector<uint32_t> nodeRec;
	GaHmmTables hmm;
	GaDevGraph dev;
	uint32_t without = 0;
	std::unique_ptr<GaSeedEngine> seed;
	GaSeedEngine* seedEngine() override { return seed.get(); }
	bool buildsMatchWords() const override { return !(without & NO_WORDS); }
	bool codesOps() const override { return !(without & NO_OPS); }
	GaBackendBatch* beginSeededBatch(const GaSeededRequest& req, GaSeededPlan& plan, int* status) override;
};

struct EmulBatch : GaBackendBatch
{
	EmulGraph* g = nullptr;
	GaRowsProvider rowsProvider;
	std::vector<uint8_t> rows;
	std::vector<uint64_t> eq;
	std::vector<GaJob> jobs;
	GaRunConfig cfg;
	std::vector<GaJobOut> outs;
	std::vector<uint8_t> pool;
	uint64_t poolTop = 0;
	std::vector<uint8_t> passOf;   // which pass of the last run finished each job (0 = the first)
	int passNo = 0;
	uint64_t retried = 0;

	bool seeded = false;       // made by beginSeededBatch: finishSeeded brings the jobs

	// a batch that built its match words itself holds what the operations program reads: the reads and one GaEqFill per job
	bool ownWords = false;
	std::vector<GaEqFill> fills;
	std::vector<uint8_t> bad;              // per fill: a row outside IUPAC
	const char* seq = nullptr; size_t seqBytes = 0;
	const uint32_t* twin = nullptr;
	uint8_t rowCode[256];
	// the match words as ga_eq_words_kernel builds them, 64 row codes at a time
	void buildWords(const GaEqSource& src, size_t eqWords);

	std::vector<uint64_t> opsOffsets;
	std::vector<uint32_t> opsRuns;
	uint64_t opsJobs = 0, opsMoves = 0;
	double opsMs = 0;

	// ga_emul_ladder.cpp: all passes over the jobs, as DevBatch::run makes them -- climb hands the product's policy launch as its back end
	bool poison = false, reuse = false;
	KeptBuffers* kept = nullptr;
	template <int MAXN, bool GENERAL, bool SPARSE = false> void runOne(uint32_t job, uint32_t capCols, uint64_t arenaWords, uint32_t traceCap);
	template <int N> void runLanesGroup(const std::vector<uint32_t>& group, uint32_t capCols, uint32_t capRows, uint32_t capMoves);
	int launch(gald::Variant v, const std::vector<uint32_t>& list, bool first);
	void climb();
	// ga_emul_ops.cpp: the two launches of ga_ops.h behind the last pass
	void codeOps();

	int finishSeeded(const std::vector<GaJob>& jobsIn, const GaRunConfig& c, GaRowsProvider r, const uint64_t* eqIn, size_t eqWords) override;
	const std::vector<uint8_t>* invalidFills() const override { return ownWords ? &bad : nullptr; }
	bool emittingRuns() const override { return cfg.emit_runs != 0; }
	int run() override
	{
		climb();
		if (cfg.emit_ops) codeOps();
		return 0;
	}
	int fetch(std::vector<GaJobOut>& o, const uint8_t** traces, uint64_t* nBytes) override
	{
		o = outs;
		for (size_t i = 0; i < o.size(); i++) o[i].reserved2 = passOf[i];      // 0 = finished by the first pass
		*traces = pool.data();
		*nBytes = poolTop;
		return 0;
	}
	int fetchOps(GaOpsOut& out) override;
	GaRunStats stats() const override { GaRunStats s; s.jobs_retried = retried; s.slots = 1; return s; }
};

}  // namespace gae
