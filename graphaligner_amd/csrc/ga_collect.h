// ga_collect.h -- the device's raw traces back into AlignmentResults (GraphAligner.h:408-491, 594-847, 3026-3098): the restatements
// of the reference's trace post-processing, and ga_batch_collect, which runs them over a batch's reads on the host threads and writes
// every read's results into the batch's arrays.
// Not a header for others: a part of ga_host.cpp's translation unit, included once at its end (as ga_device.hip includes the device
// programs), and a file of that name because the test build (tests/emul) compiles ga_host.cpp and tracks csrc/*.h.
#ifndef GA_HOST_PARTS
#error "ga_collect.h is a part of ga_host.cpp"
#endif
#include <chrono>
#include <limits>
#include <tuple>

#include "ga_host.h"

using namespace gahost;

namespace {

int mapDeviceStatus(int s)
{
	switch (s)
	{
		case GA_OK: return GA_S_OK;
		case GA_ASSERTION: return GA_S_ASSERTION;
		case GA_UNSUPPORTED_BAND: return GA_S_UNSUPPORTED_BAND;
		case GA_UNSUPPORTED_CYCLE: return GA_S_UNSUPPORTED_CYCLE;
		case GA_UNSUPPORTED_RAMP: return GA_S_UNSUPPORTED_RAMP;
		case GA_CAP_NODES: case GA_CAP_COLS: case GA_CAP_ARENA: case GA_CAP_TRACE: case GA_CAP_HEAP: case GA_PUNT: return GA_S_CAPACITY;
		default: return GA_E_DEVICE;
	}
}

// traceToAlignment (GraphAligner.h:782-847).  Node indices come straight from the device trace.
// std::string::substr's clamping (the reference builds the pieces with substr, GraphAligner.h:829,845)
SeqSpan spanOf(const ReadSeq& s, uint64_t pos, uint64_t len)
{
	if (pos > s.size()) pos = s.size();
	return SeqSpan{pos, std::min<uint64_t>(len, s.size() - pos)};
}

Partial toMappings(const ga_graph& g, const ReadSeq& sequence, int32_t score, const Trace& trace)
{
	Partial res;
	res.score = score;
	res.failed = false;
	if (trace.empty()) { res.failed = true; return res; }
	size_t pos = 0;
	uint32_t oldNode = trace[0].node;
	while (oldNode == 0)                                    // dummyNodeStart
	{
		pos++;
		if (pos == trace.size()) { res.failed = true; res.score = std::numeric_limits<int32_t>::max(); return res; }
		oldNode = trace[pos].node;
	}
	const uint64_t dummyEndAsIndex = g.bases.size() - 1;   // (sic) the reference compares a node index with a column index (:802,816)
	if (oldNode == dummyEndAsIndex) { res.failed = true; res.score = std::numeric_limits<int32_t>::max(); return res; }
	int rank = 0;
	ga_mapping_t m;
	memset(&m, 0, sizeof(m));
	m.rank = rank; m.node_id = g.ids[oldNode]; m.is_reverse = g.reverse[oldNode]; m.offset = trace[pos].offset;
	Pos nodeStart = trace[pos], nodeEnd = trace[pos], beforeNode = trace[pos];
	auto column = [&](const Pos& p) { return g.nodeStart[p.node] + p.offset; };
	for (; pos < trace.size(); pos++)
	{
		if (trace[pos].node == dummyEndAsIndex) break;
		if (trace[pos].node == oldNode) { nodeEnd = trace[pos]; continue; }
		m.from_length = (int64_t)(column(nodeEnd) - column(nodeStart) + 1);
		m.to_length = (int64_t)(nodeEnd.row - beforeNode.row);
		res.maps.push_back(m);
		res.seqs.push_back(spanOf(sequence, nodeStart.row, nodeEnd.row - beforeNode.row));
		oldNode = trace[pos].node;
		beforeNode = nodeEnd;
		nodeStart = trace[pos];
		nodeEnd = trace[pos];
		rank++;
		memset(&m, 0, sizeof(m));
		m.rank = rank; m.node_id = g.ids[oldNode]; m.is_reverse = g.reverse[oldNode];
	}
	m.from_length = (int64_t)(column(nodeEnd) - column(nodeStart));        // no +1 on the last mapping (:843)
	m.to_length = (int64_t)(nodeEnd.row - beforeNode.row);
	res.maps.push_back(m);
	res.seqs.push_back(spanOf(sequence, nodeStart.row, nodeEnd.row - beforeNode.row));
	return res;
}

// mergeAlignments (GraphAligner.h:648-688): backward part first, then forward
Partial mergePartials(const ga_graph& g, const Partial& first, const Partial& second)
{
	if (first.failed) return second;
	if (second.failed) return first;
	if (first.maps.empty()) return second;
	if (second.maps.empty()) return first;
	Partial out;
	out.failed = false;
	out.maps = first.maps;
	out.seqs = first.seqs;
	out.score = first.score + second.score;
	size_t startAt = 0;
	const ga_mapping_t& a = first.maps.back();
	const ga_mapping_t& b = second.maps.front();
	uint32_t an = g.lookup.at(a.node_id), bn = g.lookup.at(b.node_id);
	if (a.node_id == b.node_id && a.is_reverse == b.is_reverse) startAt = 1;
	else if (g.hasOutNeighbor(an, bn)) startAt = 0;
	for (size_t i = startAt; i < second.maps.size(); i++) { out.maps.push_back(second.maps[i]); out.seqs.push_back(second.seqs[i]); }
	return out;
}

bool readMatches(char readChar, char graphChar)
{
	uint8_t code = tables().rowCode[(uint8_t)readChar];
	uint8_t b = tables().baseCode[(uint8_t)graphChar];
	return b < 4 && ((code >> b) & 1);
}

// getTraceInfoInner (GraphAligner.h:718-780).  Returns false where the reference's characterMatch
// would assert: a diagonal step over a read character that is not IUPAC (e.g. 'U'), which can
// survive the backward split because ReverseComplement maps it (CommonUtils.cpp:85-88).
bool traceItemsInner(const ga_graph& g, const ReadSeq& seq, const Trace& tr, std::vector<ga_trace_item_t>& out)
{
	for (size_t i = 1; i < tr.size(); i++)
	{
		const Pos& now = tr[i];
		const Pos& old = tr[i - 1];
		bool sameColumn = now.node == old.node && now.offset == old.offset;
		bool diagonal = now.row != old.row;
		if (sameColumn)
		{
			bool selfLoop = now.row == old.row + 1 && g.nodeLen(now.node) == 1 && g.hasOutNeighbor(now.node, now.node);
			if (!selfLoop) diagonal = false;
		}
		ga_trace_item_t it;
		memset(&it, 0, sizeof(it));
		it.node_id = (int32_t)(g.ids[now.node] / 2);
		it.reverse = g.ids[now.node] % 2 == 1;
		it.offset = now.offset;
		it.read_pos = now.row;
		it.graph_char = g.baseChar(now.node, now.offset);
		it.read_char = seq[now.row];
		if (now.row == old.row) it.type = 4;
		else if (sameColumn && !diagonal) it.type = 3;
		else
		{
			if (tables().rowCode[(uint8_t)seq[now.row]] & GA_ROW_INVALID) return false;
			it.type = readMatches(seq[now.row], it.graph_char) ? 1 : 2;
		}
		out.push_back(it);
	}
	return true;
}

// getTraceInfo (GraphAligner.h:690-716)
bool traceItems(const ga_graph& g, const ReadSeq& seq, const Trace& bw, const Trace& fw, std::vector<ga_trace_item_t>& out)
{
	if (!bw.empty() && !traceItemsInner(g, seq, bw, out)) return false;
	if (!bw.empty() && !fw.empty())
	{
		ga_trace_item_t it;
		memset(&it, 0, sizeof(it));
		it.type = 5;
		it.node_id = (int32_t)(g.ids[fw[0].node] / 2);
		it.reverse = fw[0].node % 2 == 1;                   // node INDEX parity, as in the reference (:704)
		it.offset = fw[0].offset;
		it.read_pos = fw[0].row;
		it.graph_char = g.baseChar(fw[0].node, fw[0].offset);
		it.read_char = seq[fw[0].row];
		out.push_back(it);
	}
	if (!fw.empty() && !traceItemsInner(g, seq, fw, out)) return false;
	return true;
}

// addAlignmentNodes (GraphAligner.h:594-634)
typedef std::vector<std::tuple<uint64_t, uint64_t, uint32_t>> Tried;
void noteTried(Tried& tried, const Trace& t)
{
	if (t.empty()) return;
	uint32_t oldNode = t[0].node;
	uint64_t lo = t[0].row, hi = t[0].row;
	for (size_t i = 1; i < t.size(); i++)
	{
		if (t[i].node != oldNode)
		{
			tried.emplace_back(lo, hi, oldNode);
			lo = t[i].row;
			oldNode = t[i].node;
		}
		hi = t[i].row;
	}
	tried.emplace_back(lo, hi, oldNode);
}

// The device hands back, per job, the cell the traceback starts in and one byte per backward move (GA_MOVE_*; a move out of a node's
// first column names the in-neighbour it enters): one move takes a cell to its predecessor
inline void stepBack(const ga_graph& g, Pos& p, uint8_t move)
{
	const int code = move & 3, via = move >> 2;
	if (code != GA_MOVE_LEFT) p.row -= 1;
	if (code != GA_MOVE_UP)
	{
		if (p.offset > 0) p.offset -= 1;
		else
		{
			p.node = g.inNeighbor(p.node, (uint32_t)via);
			p.offset = g.nodeLen(p.node) - 1;
		}
	}
}

// the items of a read's list as (plane, column): the cells are the parts' (items[k] describes bw[k + 1], then SPLIT, then fw[k + 1])
void hostPairs(const ga_graph& g, const Trace& bw, const Trace& fw, const std::vector<ga_trace_item_t>& items, std::vector<uint64_t>& into)
{
	into.clear();
	size_t at = 0;
	const uint32_t lastNode = g.nodeCount() - 1;
	for (const Trace* part : {&bw, &fw})
	{
		for (size_t i = 1; i < part->size() && at < items.size(); i++, at++)
		{
			const Pos& p = (*part)[i];
			const ga_trace_item_t& it = items[at];
			if (p.node == 0 || p.node == lastNode) continue;
			uint32_t plane;
			if (it.type == 1) plane = 0;
			else if (it.type == 2)
			{
				switch (it.read_char) { case 'A': case 'a': plane = 1; break; case 'C': case 'c': plane = 2; break; case 'G': case 'g': plane = 3; break;
				                        case 'T': case 't': plane = 4; break; default: plane = 5; }
			}
			else if (it.type == 4) plane = 6;
			else if (it.type == 3) plane = 7;
			else continue;
			into.push_back(ga_pileup_pair(plane, g.nodeStart[p.node] + p.offset));
		}
		if (part == &bw && !bw.empty() && !fw.empty()) at++;         // (the SPLIT item)
	}
}

// the crossings of a read's list as edge slots (the rule of the EDGES kind): two consecutive items of one part -- the cells part[i],
// part[i + 1], i >= 1 -- in two columns, the second not the next offset of the same node, neither on a dummy node, over an edge of the graph
void hostSlots(const ga_graph& g, const Trace& bw, const Trace& fw, std::vector<uint32_t>& into)
{
	into.clear();
	const uint32_t lastNode = g.nodeCount() - 1;
	for (const Trace* part : {&bw, &fw})
		for (size_t i = 1; i + 1 < part->size(); i++)
		{
			const Pos& a = (*part)[i];
			const Pos& b = (*part)[i + 1];
			if (a.node == b.node && (b.offset == a.offset || b.offset == a.offset + 1)) continue;
			if (a.node == 0 || a.node == lastNode || b.node == 0 || b.node == lastNode) continue;
			const uint32_t slot = ga_edge_slot_of(g.flat, a.node, b.node);
			if (slot != 0xffffffffu) into.push_back(slot);
		}
}

// the path sequence of a read from its parts' cells and its TraceItem list (include/graphaligner_amd.h: GA_F_PATHSEQ): per part the base
// of its first cell, then the graph_char of every item of type MATCH, MISMATCH or DELETION; cells on a dummy node give nothing
void hostPathBases(const ga_graph& g, const Trace& bw, const Trace& fw, const std::vector<ga_trace_item_t>& items, std::vector<char>& into, uint32_t& nBackward)
{
	into.clear();
	nBackward = 0;
	size_t at = 0;
	const uint32_t lastNode = g.nodeCount() - 1;
	for (const Trace* part : {&bw, &fw})
	{
		if (!part->empty() && (*part)[0].node != 0 && (*part)[0].node != lastNode) into.push_back(g.baseChar((*part)[0].node, (*part)[0].offset));
		for (size_t i = 1; i < part->size() && at < items.size(); i++, at++)
		{
			const Pos& p = (*part)[i];
			const int type = items[at].type;
			if (p.node == 0 || p.node == lastNode) continue;
			if (type == 1 || type == 2 || type == 4) into.push_back(items[at].graph_char);
		}
		if (part == &bw) { nBackward = (uint32_t)into.size(); if (!bw.empty() && !fw.empty()) at++; }         // (the SPLIT item)
	}
}

// a TraceItem list's types cut into maximal runs
void itemRuns(const std::vector<ga_trace_item_t>& items, std::vector<uint32_t>& into)
{
	into.clear();
	for (const ga_trace_item_t& it : items)
	{
		if (!into.empty() && (into.back() & 7u) == (uint32_t)it.type) into.back() += 1u << 3;
		else into.push_back((uint32_t)it.type | (1u << 3));
	}
}

struct NodeRun { uint32_t node, firstOffset, lastOffset; uint64_t firstRow, lastRow; };

// what a worker thread keeps between its reads, and what it hands over when all are done (a cache line of its own: the vectors'
// ends move with every read)
struct alignas(64) Scratch
{
	std::vector<ga_trace_item_t> items;
	std::vector<uint32_t> opRuns, pileJobs;
	std::vector<uint64_t> pilePairs, pairsOfRead;
	std::vector<uint32_t> pileSlots, slotsOfRead;
	std::vector<char> pathBases;
	uint32_t pathBackward = 0;
	std::vector<NodeRun> runs;
	uint64_t columnUpdates = 0;
};

// the seed of a read whose alignment is kept: its two traces as the reference holds them, and the jobs they came from
struct BestSeed
{
	bool have = false;
	uint64_t estimate = 0, pos = 0;
	Trace fw, bw;
	int32_t fwScore = 0, bwScore = 0;
	int64_t fwJob = -1, bwJob = -1;
};

// ga_batch_collect in four stages.  Every read's results go straight into the batch's arrays, at places fixed before the threads start:
// a read's path has at most (moves that left a node through its first column, counted by the traceback) + 1 node runs per job, its edit
// sequences are pieces of the read, its trace items at most one per move.  The arrays have gaps where a read needs less; first_mapping /
// n_mappings, edit_seq_off and first_trace / n_trace say where each read's entries are.
struct Collector
{
	ga_batch* const b;
	const ga_graph& g;
	const size_t nReads;
	// GA_F_OPS: every job's runs as the back end coded them (ga_ops.h), in the final order of the job's part of the TraceItem list
	// GA_F_PILEUP: the same walk on the device later (ga_pileup.h), so the same reads are left to the host's TraceItem list
	// GA_F_PATHSEQ: every job's bases as the back end wrote them (ga_pathseq.h), in the final order of the job's part
	const bool wantTrace, wantOps, wantPile, wantPath, wantWalk;
	std::unique_ptr<ResultsOwner> R;
	// the records, moves and runs stay the back end's from fetch until fetchDone
	struct Fetched { GaBackendBatch* dev = nullptr; void done() { if (dev) dev->fetchDone(); dev = nullptr; } ~Fetched() { done(); } } fetched;
	std::vector<GaJobOut> outs;
	const uint8_t* moves = nullptr;
	uint64_t nMoveBytes = 0;
	GaOpsOut devOps;
	GaPathSeqOut devPath;
	std::vector<uint64_t> mapAt, editAt, traceAt, opsAt, pathAt;
	// GA_F_OPS: reads whose runs are derived here from the TraceItem list instead (include/graphaligner_amd.h: GA_F_OPS): a character
	// outside IUPAC (the item pass decides the read's status), and a forward part that the reference leaves unshifted (:3091-3094)
	// or whose rows it does not cut at the overlap (the unsigned difference of :3051 wraps) -- there the device's characters are not
	// the list's
	std::vector<uint8_t> opsOnHost;
	ga_read_result_t* allReads = nullptr;
	ga_mapping_t* allMappings = nullptr;
	const char* allEdits = nullptr;
	ga_trace_item_t* allTrace = nullptr;
	ga_read_ops_t* allReadOps = nullptr;
	uint32_t* allOps = nullptr;
	ga_read_path_seq_t* allReadPath = nullptr;
	char* allPathBases = nullptr;
	std::atomic<int> overflow{0};
	std::atomic<uint64_t> forwardOnlyReads{0}, opsFromDevice{0}, opsFromHost{0}, pileFromDevice{0}, pileFromHost{0}, pathFromDevice{0}, pathFromHost{0};
	std::chrono::steady_clock::time_point t0, t1, t2;
	size_t nThreads = 1;

	explicit Collector(ga_batch* batch)
		: b(batch), g(*batch->g), nReads(batch->reads.size()), wantTrace((batch->flags & GA_F_TRACE) != 0), wantOps((batch->flags & GA_F_OPS) != 0),
		  wantPile((batch->flags & GA_F_PILEUP) != 0), wantPath((batch->flags & GA_F_PATHSEQ) != 0), wantWalk(wantOps || wantPile || wantPath) {}

	int fetch();
	int sizePlaces();
	void assemble();
	int publish(ga_results_t** out);

	void work(size_t lo, size_t hi, Scratch& s);
	Trace deviceTrace(int64_t job);
	void nodeRuns(const GaJobOut& o, uint64_t traceable, std::vector<NodeRun>& runs) const;
	bool runMappings(size_t ri, const std::vector<NodeRun>& runs);
	bool forwardOnly(size_t ri, ga_read_result_t& rr, Scratch& s);
	int seedTraces(const SeedPlan& sp, const ReadSeq& seq, BestSeed& cur);
	int bestSeed(size_t ri, ga_read_result_t& rr, BestSeed& best);
	bool derive(size_t ri, const BestSeed& best, Scratch& s, bool& hostOps, bool& hostPile, bool& hostPath);
	void store(size_t ri, ga_read_result_t& rr, const BestSeed& best, Scratch& s, bool hostOps, bool hostPile, bool hostPath);
	void devicePath(int64_t bwJob, bool bwCells, int64_t fwJob, bool fwCells, std::vector<char>& into, uint32_t& nBackward) const;
	bool storePath(size_t ri, const std::vector<char>& basesOfRead, uint32_t nBackward, bool fromHost);
	void deviceOps(int64_t bwJob, bool bwCells, int64_t fwJob, bool fwCells, std::vector<uint32_t>& into) const;
	bool storeOps(size_t ri, const std::vector<uint32_t>& runsOfRead, bool fromHost);
	void fail(ga_read_result_t& rr) { overflow.store(1); rr.status = GA_E_DEVICE; }   // (a bound of sizePlaces is wrong: fail loudly instead of writing past a read's place)
};

// ---- stage 1: records, moves and runs from the back end ----------------------------------------
int Collector::fetch()
{
	t0 = std::chrono::steady_clock::now();
	if (int s = b->dev->fetch(outs, &moves, &nMoveBytes)) return s;
	fetched.dev = b->dev;
	b->collected = false;
	b->pileList.clear(); b->pilePairs.clear(); b->pileSlots.clear();
	if (wantOps)
	{
		if (int s = b->dev->fetchOps(devOps)) return s;
		if (!outs.empty() && (!devOps.runs || !devOps.offsets)) return GA_E_DEVICE;
	}
	if (wantPath)
	{
		if (int s = b->dev->fetchPathSeq(devPath)) return s;
		if (!outs.empty() && (!devPath.bases || !devPath.offsets)) return GA_E_DEVICE;
	}
	t1 = std::chrono::steady_clock::now();
	b->columnUpdates = 0;
	b->slicesRun = 0;
	for (const GaJobOut& o : outs) b->slicesRun += o.n_run;         // (column updates are summed per read below: seeds the reference would skip do not count)
	return GA_S_OK;
}

// ---- stage 2: every read's place in the arrays --------------------------------------------------
int Collector::sizePlaces()
{
	R.reset(new ResultsOwner());
	mapAt.assign(nReads + 1, 0); editAt.assign(nReads + 1, 0); traceAt.assign(nReads + 1, 0); opsAt.assign(wantOps ? nReads + 1 : 0, 0);
	pathAt.assign(wantPath ? nReads + 1 : 0, 0);
	opsOnHost.assign(wantWalk ? nReads : 0, 0);
	for (size_t ri = 0; ri < nReads; ri++)
	{
		const ReadPlan& rp = b->reads[ri];
		uint64_t runs = 1, items = 0, opRuns = 0, bases = 0;
		for (size_t k = rp.firstSeed; k < rp.firstSeed + rp.nSeeds; k++)
		{
			const SeedPlan& sp = b->seeds[k];
			for (int64_t job : {sp.bwJob, sp.fwJob})
				if (job >= 0 && outs[job].status == GA_OK)
				{
					runs += (uint64_t)outs[job].n_node_steps + 1; items += (uint64_t)outs[job].trace_len + 2;
					if (wantOps) opRuns += devOps.offsets[job + 1] - devOps.offsets[job] + 1;
					if (wantPath) bases += devPath.offsets[job + 1] - devPath.offsets[job];
				}
			if (wantWalk)
			{
				if (sp.fwJob >= 0 && sp.pos > 0 && !(sp.bwJob >= 0 && outs[sp.bwJob].n_valid > 0)) opsOnHost[ri] = 1;
				if (sp.fwJob >= 0 && b->seqs[ri].size() - sp.pos < (uint64_t)g.dbgOverlap) opsOnHost[ri] = 1;
			}
		}
		mapAt[ri + 1] = mapAt[ri] + runs;
		editAt[ri + 1] = editAt[ri] + b->seqs[ri].size();
		traceAt[ri + 1] = traceAt[ri] + (wantTrace ? items : 0);
		if (wantWalk && b->readInvalid[ri].load(std::memory_order_relaxed)) opsOnHost[ri] = 1;
		if (wantOps) opsAt[ri + 1] = opsAt[ri] + (opsOnHost[ri] ? items : opRuns);
		// (a part of K cells has at most K bases, and a job's cells are its moves + 1)
		if (wantPath) pathAt[ri + 1] = pathAt[ri] + (opsOnHost[ri] ? items : bases);
	}
	if (wantPath)
	{
		allReadPath = (ga_read_path_seq_t*)R->allReadPath.get((nReads + 1) * sizeof(ga_read_path_seq_t));
		allPathBases = (char*)R->allPathBases.get(pathAt[nReads] + 1);
		if (!allReadPath || !allPathBases) return GA_E_INVALID;
	}
	if (wantOps)
	{
		allReadOps = (ga_read_ops_t*)R->allReadOps.get((nReads + 1) * sizeof(ga_read_ops_t));
		allOps = (uint32_t*)R->allOps.get((opsAt[nReads] + 1) * sizeof(uint32_t));
		if (!allReadOps || !allOps) return GA_E_INVALID;
	}
	allReads = (ga_read_result_t*)R->allReads.get((nReads + 1) * sizeof(ga_read_result_t));
	allMappings = (ga_mapping_t*)R->allMappings.get((mapAt[nReads] + 1) * sizeof(ga_mapping_t));
	// (no copy of the edit sequences: they are pieces of the reads, and the results share the batch's read buffer)
	allEdits = b->seqBuf;
	R->seqKeep = b->seqKeep;
	allTrace = (ga_trace_item_t*)R->allTrace.get((traceAt[nReads] + 1) * sizeof(ga_trace_item_t));
	return allReads && allMappings && allEdits && allTrace ? GA_S_OK : GA_E_INVALID;
}

// ---- stage 3: the reads, on the host threads ----------------------------------------------------
// Replaying a job's moves gives the reference's trace, which runs from row 0 upwards (getTraceFromTable :949-952).
Trace Collector::deviceTrace(int64_t job)
{
	Trace t;
	const GaJobOut& o = outs[job];
	if (o.n_valid == 0) return t;
	if (o.reserved3 == 1) { overflow.store(1); return t; }      // (node runs, not moves: only batches that need no cell list get them)
	const uint8_t* mv = moves + o.trace_off;
	t.resize((size_t)o.trace_len + 1);
	Pos p{o.start_node, o.start_offset, o.start_row};
	size_t at = t.size() - 1;
	t[at] = p;
	for (uint32_t i = 0; i < o.trace_len; i++) { stepBack(g, p, mv[i]); t[--at] = p; }
	return t;
}

// The node runs of a forward job's path below row `traceable`, from the read's end to its start: the traceback's own records, or the
// moves replayed once, with node runs noted as they end.
void Collector::nodeRuns(const GaJobOut& o, uint64_t traceable, std::vector<NodeRun>& runs) const
{
	runs.clear();
	if (o.reserved3 == 1)
	{
		// the traceback's own node runs (five words each), from the read's end to its start like the replay's
		const uint32_t* rec = (const uint32_t*)(moves + o.trace_off);
		runs.resize(o.trace_len);
		for (uint32_t k = 0; k < o.trace_len; k++, rec += 5) runs[k] = NodeRun{rec[0], rec[1], rec[3], rec[2], rec[4]};
	}
	else
	{
		const uint8_t* mv = moves + o.trace_off;
		const uint32_t nMoves = o.trace_len;
		Pos p{o.start_node, o.start_offset, o.start_row};
		uint32_t i = 0;
		while (p.row >= traceable && i < nMoves) stepBack(g, p, mv[i++]);        // the trace's tail beyond the read's end is dropped (:3051-3055)
		if (p.row < traceable)
		{
			// a run is opened at its last cell (the first one met on the way back) and closed, with its first cell, when the path
			// leaves the node; eight diagonal steps inside a node are taken at once
			runs.push_back(NodeRun{p.node, p.offset, p.offset, p.row, p.row});
			const uint64_t eightDiagonals = 0x0101010101010101ull * (uint64_t)GA_MOVE_DIAG;
			while (i < nMoves)
			{
				if (i + 8 <= nMoves && p.offset >= 8)
				{
					uint64_t w;
					memcpy(&w, mv + i, 8);
					if (w == eightDiagonals) { p.offset -= 8; p.row -= 8; i += 8; continue; }
				}
				const Pos before = p;
				stepBack(g, p, mv[i++]);
				if (p.node != before.node)
				{
					runs.back().firstOffset = before.offset; runs.back().firstRow = before.row;
					runs.push_back(NodeRun{p.node, p.offset, p.offset, p.row, p.row});
				}
			}
			runs.back().firstOffset = p.offset; runs.back().firstRow = p.row;
		}
	}
	// traceToAlignment's dummy nodes (:786-800, 816): cells of the start dummy at the read's start are skipped, a path that begins
	// in the end dummy fails, and the path is cut where it first enters the end dummy
	const uint64_t dummyEndAsIndex = g.bases.size() - 1;
	while (!runs.empty() && runs.back().node == 0) runs.pop_back();
	if (!runs.empty() && runs.back().node == dummyEndAsIndex) runs.clear();
	for (size_t k = runs.size(); k-- > 0;)
		if (runs[k].node == dummyEndAsIndex) { runs.erase(runs.begin(), runs.begin() + (long)k + 1); break; }
}

// a read's mappings from the node runs of its one job (noted from the read's end to its start); false: they do not fit its place
bool Collector::runMappings(size_t ri, const std::vector<NodeRun>& runs)
{
	const ReadSeq& seq = b->seqs[ri];
	const size_t nRuns = runs.size();
	if (nRuns > mapAt[ri + 1] - mapAt[ri]) return false;
	uint64_t editTop = editAt[ri];
	uint64_t beforeRow = runs[nRuns - 1].firstRow;
	for (size_t k = 0; k < nRuns; k++)
	{
		const NodeRun& r = runs[nRuns - 1 - k];
		ga_mapping_t m;
		memset(&m, 0, sizeof(m));
		m.rank = (int32_t)k;
		m.node_id = g.ids[r.node];
		m.is_reverse = g.reverse[r.node];
		m.offset = k == 0 ? r.firstOffset : 0;
		m.from_length = (int64_t)r.lastOffset - (int64_t)r.firstOffset + (k + 1 < nRuns ? 1 : 0);        // no +1 on the last mapping (:843)
		m.to_length = (int64_t)(r.lastRow - beforeRow);
		const SeqSpan piece = spanOf(seq, r.firstRow, r.lastRow - beforeRow);
		m.edit_seq_off = (uint64_t)(seq.data() - allEdits) + piece.pos;
		if (piece.len > editAt[ri + 1] - editTop) return false;
		editTop += piece.len;
		allMappings[mapAt[ri] + k] = m;
		beforeRow = r.lastRow;
	}
	return true;
}

// the winning seed's runs: backward job, one SPLIT run when both parts have cells, forward job
void Collector::deviceOps(int64_t bwJob, bool bwCells, int64_t fwJob, bool fwCells, std::vector<uint32_t>& into) const
{
	into.clear();
	if (bwCells && bwJob >= 0) into.insert(into.end(), devOps.runs + devOps.offsets[bwJob], devOps.runs + devOps.offsets[bwJob + 1]);
	if (bwCells && fwCells) into.push_back(GA_OP_SPLIT | (1u << 3));
	if (fwCells && fwJob >= 0) into.insert(into.end(), devOps.runs + devOps.offsets[fwJob], devOps.runs + devOps.offsets[fwJob + 1]);
}

// the winning seed's bases: backward job, forward job
void Collector::devicePath(int64_t bwJob, bool bwCells, int64_t fwJob, bool fwCells, std::vector<char>& into, uint32_t& nBackward) const
{
	into.clear();
	if (bwCells && bwJob >= 0) into.insert(into.end(), devPath.bases + devPath.offsets[bwJob], devPath.bases + devPath.offsets[bwJob + 1]);
	nBackward = (uint32_t)into.size();
	if (fwCells && fwJob >= 0) into.insert(into.end(), devPath.bases + devPath.offsets[fwJob], devPath.bases + devPath.offsets[fwJob + 1]);
}

// a read's finished bases into its place
bool Collector::storePath(size_t ri, const std::vector<char>& basesOfRead, uint32_t nBackward, bool fromHost)
{
	if (basesOfRead.size() > pathAt[ri + 1] - pathAt[ri]) return false;
	ga_read_path_seq_t& rp = allReadPath[ri];
	rp.n_bases = (uint32_t)basesOfRead.size();
	rp.n_backward = nBackward;
	if (!basesOfRead.empty()) memcpy(allPathBases + pathAt[ri], basesOfRead.data(), basesOfRead.size());
	if (!fromHost) pathFromDevice++;                        // (a read on the host path was counted when its item pass ran)
	return true;
}

// a read's finished runs into its place, with the four counts
bool Collector::storeOps(size_t ri, const std::vector<uint32_t>& runsOfRead, bool fromHost)
{
	if (runsOfRead.size() > opsAt[ri + 1] - opsAt[ri]) return false;
	ga_read_ops_t& ro = allReadOps[ri];
	ro.n_ops = (uint32_t)runsOfRead.size();
	uint32_t sum[8] = {0, 0, 0, 0, 0, 0, 0, 0};
	for (size_t k = 0; k < runsOfRead.size(); k++) { allOps[opsAt[ri] + k] = runsOfRead[k]; sum[runsOfRead[k] & 7u] += runsOfRead[k] >> 3; }
	ro.n_match = sum[GA_OP_MATCH]; ro.n_mismatch = sum[GA_OP_MISMATCH]; ro.n_insertion = sum[GA_OP_INSERTION]; ro.n_deletion = sum[GA_OP_DELETION];
	if (!fromHost) opsFromDevice++;                         // (a read on the host path was counted when its item pass ran)
	return true;
}

// The common shape -- one seed at the read's first base, so one forward job, and no TraceItem list wanted -- without the detour
// over a cell list: the mappings are written from the job's node runs.  Same result as the general code below
// (getPiecewiseTracesFromSplit :3039-3098 without a backward part, traceToAlignment :782-847, mergeAlignments with a failed first
// part).  Returns whether the read was dealt with here.
bool Collector::forwardOnly(size_t ri, ga_read_result_t& rr, Scratch& s)
{
	const ReadPlan& rp = b->reads[ri];
	if (rp.nSeeds != 1 || wantTrace || (wantWalk && opsOnHost[ri])) return false;
	const SeedPlan& sp = b->seeds[rp.firstSeed];
	if (sp.early != GA_S_OK || sp.bwJob >= 0 || sp.fwJob < 0 || sp.pos != 0) return false;
	const GaJobOut& o = outs[sp.fwJob];
	if (o.status != GA_OK) return false;
	rr.reserved = (int32_t)o.reserved2;                                      // which kernel pass finished the job (0 = the first)
	// (the reference's eager TraceItem pass asserts on characters outside IUPAC: with the one forward job from the first base the
	// job's rows are the whole read, and the match-word pass has noted whether one of them is such a character)
	if (b->readInvalid[ri].load(std::memory_order_relaxed)) return false;
	rr.column_updates += o.n_columns;
	rr.status = GA_S_OK;
	if (o.n_valid == 0) return true;                                         // nothing kept: both parts fail (rr stays failed)
	nodeRuns(o, b->seqs[ri].size() - sp.pos - g.dbgOverlap, s.runs);
	if (s.runs.empty()) return true;                                         // an empty trace fails (:786-790)
	if (!runMappings(ri, s.runs)) { fail(rr); return true; }
	if (wantOps)
	{
		deviceOps(-1, false, sp.fwJob, true, s.opRuns);
		if (!storeOps(ri, s.opRuns, false)) { fail(rr); return true; }
	}
	if (wantPile) { s.pileJobs.push_back((uint32_t)sp.fwJob | GA_PILEUP_COUNTS); pileFromDevice++; }
	if (wantPath)
	{
		// the device bytes of the one job, as they are
		const uint64_t from = devPath.offsets[sp.fwJob], n = devPath.offsets[sp.fwJob + 1] - from;
		if (n > pathAt[ri + 1] - pathAt[ri]) { fail(rr); return true; }
		if (n) memcpy(allPathBases + pathAt[ri], devPath.bases + from, n);
		allReadPath[ri].n_bases = (uint32_t)n;
		pathFromDevice++;
	}
	rr.failed = 0;
	rr.score = o.score;
	rr.n_mappings = s.runs.size();
	rr.n_trace = 0;
	rr.query_position = 0;
	rr.alignment_start = 0;
	rr.alignment_end = (uint64_t)o.n_valid * W;
	return true;
}

// getPiecewiseTracesFromSplit (:3039-3098): a seed's two traces, cut at the read's ends, the backward one mirrored
int Collector::seedTraces(const SeedPlan& sp, const ReadSeq& seq, BestSeed& cur)
{
	if (sp.fwJob >= 0 && outs[sp.fwJob].n_valid > 0)
	{
		const uint64_t traceable = seq.size() - sp.pos - g.dbgOverlap;
		cur.fw = deviceTrace(sp.fwJob);
		cur.fwScore = outs[sp.fwJob].score;
		while (!cur.fw.empty() && cur.fw.back().row >= traceable) cur.fw.pop_back();
	}
	if (sp.bwJob >= 0 && outs[sp.bwJob].n_valid > 0)
	{
		const uint64_t traceable = sp.pos;
		cur.bw = deviceTrace(sp.bwJob);
		cur.bwScore = outs[sp.bwJob].score;
		while (!cur.bw.empty() && cur.bw.back().row >= traceable) cur.bw.pop_back();
		// reverseTrace (:3026-3037)
		std::reverse(cur.bw.begin(), cur.bw.end());
		const uint64_t endRow = sp.pos - 1;
		for (auto& p : cur.bw)
		{
			uint32_t other;
			if (g.reverseNode(p.node, other) != GA_S_OK || p.row > endRow) return GA_S_ASSERTION;
			p.offset = g.nodeLen(other) - 1 - p.offset;
			p.node = other;
			p.row = endRow - p.row;
		}
		for (auto& p : cur.fw) p.row += sp.pos;                            // only inside this branch (:3091-3094)
	}
	return GA_S_OK;
}

// the seeds of a read in turn (:412-461): the one with the longest estimate is kept.  Returns the read's status.
int Collector::bestSeed(size_t ri, ga_read_result_t& rr, BestSeed& best)
{
	const ReadPlan& rp = b->reads[ri];
	Tried tried;
	for (size_t k = rp.firstSeed; k < rp.firstSeed + rp.nSeeds; k++)
	{
		const SeedPlan& sp = b->seeds[k];
		if (sp.early == GA_S_BAD_SEED) return GA_S_BAD_SEED;
		bool covered = false;
		for (auto& t : tried) if (std::get<0>(t) <= sp.pos && std::get<1>(t) >= sp.pos && std::get<2>(t) == sp.seedNodeIndex) { covered = true; break; }
		if (covered) continue;                                               // "seed already aligned" (:425-429)
		if (sp.early != GA_S_OK) return sp.early;
		int status = GA_S_OK;
		BestSeed cur;
		for (int64_t job : {sp.bwJob, sp.fwJob})
		{
			if (job < 0) continue;
			rr.column_updates += outs[job].n_columns;
			rr.reserved = std::max<int32_t>(rr.reserved, (int32_t)outs[job].reserved2);
			if (outs[job].status != GA_OK) status = mapDeviceStatus(outs[job].status);
			else cur.estimate += (uint64_t)outs[job].n_valid * W;
		}
		if (status == GA_S_OK) status = seedTraces(sp, b->seqs[ri], cur);
		if (status != GA_S_OK) return status;
		noteTried(tried, cur.fw);
		noteTried(tried, cur.bw);
		if (!best.have || cur.estimate > best.estimate)
		{
			cur.have = true; cur.pos = sp.pos; cur.fwJob = sp.fwJob; cur.bwJob = sp.bwJob;
			best = std::move(cur);
		}
	}
	return GA_S_OK;
}

// What is derived from the kept seed's cells: the TraceItem list (s.items; left empty unless GA_F_TRACE wants it) and, for the reads
// left to the host, the runs of GA_F_OPS (s.opRuns) and the items of GA_F_PILEUP (s.pairsOfRead).  False where the reference asserts.
bool Collector::derive(size_t ri, const BestSeed& best, Scratch& s, bool& hostOps, bool& hostPile, bool& hostPath)
{
	const ReadSeq& seq = b->seqs[ri];
	// the reference always builds the TraceItem list (:463) and characterMatch asserts on a
	// non-IUPAC read character; only reads that contain one need the scan when no trace is wanted
	bool suspicious = false;
	if (!wantTrace || wantWalk) for (char c : seq) if (tables().rowCode[(uint8_t)c] & GA_ROW_INVALID) { suspicious = true; break; }
	s.items.clear();
	// (a character outside IUPAC that no job's rows show as such -- 'U' in a backward part, which ReverseComplement maps -- is found
	// by this scan; the device's runs of such a read are within the bound its place was sized with, and storeOps checks it)
	hostOps = wantOps && (opsOnHost[ri] || suspicious);
	hostPile = wantPile && (opsOnHost[ri] || suspicious);
	hostPath = wantPath && (opsOnHost[ri] || suspicious);
	if (!(wantTrace || suspicious || hostOps || hostPile || hostPath)) return true;
	const bool fine = traceItems(g, seq, best.bw, best.fw, s.items);
	if (hostOps) opsFromHost++;
	if (hostPath) pathFromHost++;
	if (hostPath && fine) hostPathBases(g, best.bw, best.fw, s.items, s.pathBases, s.pathBackward);
	if (hostPile && fine) { hostPairs(g, best.bw, best.fw, s.items, s.pairsOfRead); hostSlots(g, best.bw, best.fw, s.slotsOfRead); }
	if (hostOps && fine) itemRuns(s.items, s.opRuns);
	if (!wantTrace || !fine) s.items.clear();
	return fine;
}

// the kept seed's mappings (traceToAlignment of both parts, merged), runs, pileup entries and trace items into the read's place
void Collector::store(size_t ri, ga_read_result_t& rr, const BestSeed& best, Scratch& s, bool hostOps, bool hostPile, bool hostPath)
{
	const ReadSeq& seq = b->seqs[ri];
	Partial fwp = toMappings(g, seq, best.fwScore, best.fw);
	Partial bwp = toMappings(g, seq, best.bwScore, best.bw);
	if (fwp.failed && bwp.failed) return;
	Partial merged = mergePartials(g, bwp, fwp);
	uint64_t editBytes = 0;
	for (const SeqSpan& piece : merged.seqs) editBytes += piece.len;
	if (merged.maps.size() > mapAt[ri + 1] - mapAt[ri] || editBytes > editAt[ri + 1] - editAt[ri] || s.items.size() > traceAt[ri + 1] - traceAt[ri]) { fail(rr); return; }
	if (wantOps)
	{
		if (!hostOps) deviceOps(best.bwJob, !best.bw.empty(), best.fwJob, !best.fw.empty(), s.opRuns);
		if (!storeOps(ri, s.opRuns, hostOps)) { fail(rr); return; }
	}
	if (wantPath)
	{
		if (!hostPath) devicePath(best.bwJob, !best.bw.empty(), best.fwJob, !best.fw.empty(), s.pathBases, s.pathBackward);
		if (!storePath(ri, s.pathBases, s.pathBackward, hostPath)) { fail(rr); return; }
	}
	if (wantPile)
	{
		if (hostPile)
		{
			s.pilePairs.insert(s.pilePairs.end(), s.pairsOfRead.begin(), s.pairsOfRead.end());
			s.pileSlots.insert(s.pileSlots.end(), s.slotsOfRead.begin(), s.slotsOfRead.end());
			pileFromHost++;
		}
		else
		{
			if (!best.bw.empty() && best.bwJob >= 0) s.pileJobs.push_back((uint32_t)best.bwJob | GA_PILEUP_COUNTS);
			if (!best.fw.empty() && best.fwJob >= 0) s.pileJobs.push_back((uint32_t)best.fwJob | GA_PILEUP_COUNTS);
			pileFromDevice++;
		}
	}
	rr.failed = 0;
	rr.score = merged.score;
	rr.n_mappings = merged.maps.size();
	for (size_t i = 0; i < merged.maps.size(); i++)
	{
		ga_mapping_t m = merged.maps[i];
		m.edit_seq_off = (uint64_t)(seq.data() - allEdits) + merged.seqs[i].pos;
		allMappings[mapAt[ri] + i] = m;
	}
	rr.n_trace = s.items.size();
	if (!s.items.empty()) memcpy(allTrace + traceAt[ri], s.items.data(), s.items.size() * sizeof(s.items[0]));
	const uint64_t lastAligned = !best.bw.empty() ? best.bw[0].row : best.pos;
	rr.query_position = lastAligned;
	rr.alignment_start = lastAligned;
	rr.alignment_end = lastAligned + best.estimate;
}

void Collector::work(size_t lo, size_t hi, Scratch& s)
{
	for (size_t ri = lo; ri < hi; ri++)
	{
		ga_read_result_t& rr = allReads[ri];
		memset(&rr, 0, sizeof(rr));
		rr.failed = 1;
		rr.score = std::numeric_limits<int32_t>::max();
		rr.first_mapping = mapAt[ri];
		rr.first_trace = traceAt[ri];
		if (wantOps) { memset(&allReadOps[ri], 0, sizeof(ga_read_ops_t)); allReadOps[ri].first_op = opsAt[ri]; }
		if (wantPath) { memset(&allReadPath[ri], 0, sizeof(ga_read_path_seq_t)); allReadPath[ri].first_base = pathAt[ri]; }
		if (b->reads[ri].nSeeds == 0) { rr.status = GA_S_ASSERTION; continue; }          // assert(seedHits.size() > 0) (:412)
		if (forwardOnly(ri, rr, s)) { s.columnUpdates += rr.column_updates; forwardOnlyReads++; continue; }
		BestSeed best;
		rr.status = bestSeed(ri, rr, best);
		s.columnUpdates += rr.column_updates;
		if (rr.status != GA_S_OK || !best.have) continue;
		bool hostOps = false, hostPile = false, hostPath = false;
		if (!derive(ri, best, s, hostOps, hostPile, hostPath)) { rr.status = GA_S_ASSERTION; continue; }
		store(ri, rr, best, s, hostOps, hostPile, hostPath);
	}
}

void Collector::assemble()
{
	// reads are independent: small pieces handed out from a counter (reads sorted by nothing in particular, but their lengths differ),
	// one Scratch per thread; GA_F_PILEUP: every thread notes the aligned reads' winning jobs and host items and hands them over here
	std::vector<Scratch> scratch(64);
	nThreads = forChunks(nReads, scratch.size(), 64, [this](size_t threads) { return std::max<size_t>(16, nReads / (threads * 16) + 1); },
	                     [&](size_t lo, size_t hi, size_t thread) { work(lo, hi, scratch[thread]); });
	for (size_t t = 0; t < nThreads; t++)
	{
		b->columnUpdates += scratch[t].columnUpdates;
		b->pileList.insert(b->pileList.end(), scratch[t].pileJobs.begin(), scratch[t].pileJobs.end());
		b->pilePairs.insert(b->pilePairs.end(), scratch[t].pilePairs.begin(), scratch[t].pilePairs.end());
		b->pileSlots.insert(b->pileSlots.end(), scratch[t].pileSlots.begin(), scratch[t].pileSlots.end());
	}
	b->opsFromDevice = opsFromDevice.load(); b->opsFromHost = opsFromHost.load();
	b->pathFromDevice = pathFromDevice.load(); b->pathFromHost = pathFromHost.load();
	fetched.done();
	t2 = std::chrono::steady_clock::now();
}

// ---- stage 4: hand-over ---------------------------------------------------------------------------
int Collector::publish(ga_results_t** out)
{
	if (overflow.load()) { b->pileList.clear(); b->pilePairs.clear(); b->pileSlots.clear(); return GA_E_DEVICE; }
	if (wantPile)
	{
		// longest first, as the passes' own lists are: the kernel deals the entries over its waves statically
		std::sort(b->pileList.begin(), b->pileList.end(), [&](uint32_t x, uint32_t y) {
			const uint32_t lx = outs[x & ~GA_PILEUP_COUNTS].trace_len, ly = outs[y & ~GA_PILEUP_COUNTS].trace_len;
			return lx != ly ? lx > ly : x < y;
		});
		b->pileFromDevice = pileFromDevice.load(); b->pileFromHost = pileFromHost.load();
		b->collected = true;
	}
	ga_results_t& pub = R->pub;
	pub.n_reads = nReads; pub.reads = allReads;
	pub.n_mappings = mapAt[nReads]; pub.mappings = allMappings;
	pub.n_edit_bytes = b->seqBufBytes; pub.edit_bytes = allEdits;
	pub.n_trace = traceAt[nReads]; pub.trace = allTrace;
	pub.read_ops = allReadOps; pub.n_ops = wantOps ? opsAt[nReads] : 0; pub.ops = allOps;
	pub.read_path_seq = allReadPath; pub.n_path_bases = wantPath ? pathAt[nReads] : 0; pub.path_bases = allPathBases;
	*out = &R.release()->pub;
	if (getenv("GA_DEBUG_COLLECT"))
	{
		auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
		fprintf(stderr, "graphaligner_amd: collect: fetch %.1f ms (%zu trace bytes), assembly %.1f ms on %zu threads (%llu of %zu reads on the forward-only path), hand-over %.1f ms\n", ms(t0, t1), (size_t)nMoveBytes, ms(t1, t2), nThreads, (unsigned long long)forwardOnlyReads.load(), nReads, ms(t2, std::chrono::steady_clock::now()));
	}
	return GA_S_OK;
}

}  // namespace

extern "C" {

int ga_batch_collect(ga_batch_t* b, ga_results_t** out)
{
	if (!b || !out || !b->dev || !b->ran) return GA_E_INVALID;
	Collector c(b);
	int s = c.fetch();
	if (!s) s = c.sizePlaces();
	if (s) return s;
	c.assemble();
	return c.publish(out);
}

int ga_batch_stats(const ga_batch_t* b, ga_batch_stats_t* out)
{
	if (!b || !out || !b->dev) return GA_E_INVALID;
	memset(out, 0, sizeof(*out));
	GaRunStats st = b->dev->stats();
	out->n_jobs = b->jobs.size();
	out->kernel_ms = st.kernel_ms;
	out->main_kernel_ms = st.main_ms;
	out->main_variant = st.main_variant;
	out->slots = st.slots;
	out->waves_per_cu = st.waves_per_cu;
	out->scratch_bytes = st.scratch_bytes;
	out->jobs_retried = st.jobs_retried;
	for (int k = 0; k < 8; k++) out->stamps[k] = st.stamps[k];
	out->column_updates = b->columnUpdates;
	out->reserved = (int32_t)b->cfg.emit_runs;
	out->slices = b->slicesRun;
	return GA_S_OK;
}

int ga_batch_ops_stats(const ga_batch_t* b, ga_batch_ops_stats_t* out)
{
	if (!b || !out || !b->dev || !(b->flags & GA_F_OPS)) return GA_E_INVALID;
	memset(out, 0, sizeof(*out));
	GaOpsOut o;
	if (b->ran && b->dev->fetchOps(o) == 0)
	{
		out->count_kernel_ms = o.count_ms; out->write_kernel_ms = o.write_ms;
		out->jobs_coded = o.jobs; out->moves_read = o.moves; out->runs_written = o.n_runs;
	}
	out->reads_from_device = b->opsFromDevice; out->reads_from_host = b->opsFromHost;
	return GA_S_OK;
}

int ga_batch_path_seq_stats(const ga_batch_t* b, ga_batch_path_seq_stats_t* out)
{
	if (!b || !out || !b->dev || !(b->flags & GA_F_PATHSEQ)) return GA_E_INVALID;
	memset(out, 0, sizeof(*out));
	GaPathSeqOut o;
	if (b->ran && b->dev->fetchPathSeq(o) == 0)
	{
		out->count_kernel_ms = o.count_ms; out->write_kernel_ms = o.write_ms;
		out->jobs_walked = o.jobs; out->moves_read = o.moves; out->bases_written = o.n_bases;
	}
	out->reads_from_device = b->pathFromDevice; out->reads_from_host = b->pathFromHost;
	return GA_S_OK;
}

void ga_batch_free(ga_batch_t* b) { delete b; }

void ga_results_free(ga_results_t* r)
{
	if (!r) return;
	delete reinterpret_cast<ResultsOwner*>(r);     // `pub` is the owner's first member
}

// results over a graph loaded with ga_graph_load_gfa_split, expressed on the nodes of the GFA file: consecutive mappings on pieces of
// one node become one mapping (lengths add up, the edit sequences are contiguous), offsets and trace items move to the node's coordinates
int ga_results_unsplit(const ga_graph_t* g, const ga_results_t* in, ga_results_t** out)
{
	if (!g || !in || !out) return GA_E_INVALID;
	ResultsOwner* R = new ResultsOwner();
	// (every mapping's edit sequence is copied: the pieces of merged mappings are joined here, whatever lies between them in `in`)
	R->edits.reserve(in->n_edit_bytes / 4 + 64);
	auto piece = [&](int64_t digraphId) -> const ga_graph::Piece* {
		auto it = g->pieces.find(digraphId / 2);
		return it == g->pieces.end() ? nullptr : &it->second;
	};
	for (size_t i = 0; i < in->n_reads; i++)
	{
		ga_read_result_t rr = in->reads[i];
		const size_t firstMap = R->mappings.size(), firstTrace = R->trace.size();
		const ga_graph::Piece* prevPiece = nullptr;
		for (uint64_t k = 0; k < rr.n_mappings; k++)
		{
			ga_mapping_t m = in->mappings[rr.first_mapping + k];
			const char* const editFrom = in->edit_bytes + m.edit_seq_off;
			const size_t editLen = (size_t)m.to_length;
			const ga_graph::Piece* p = piece(m.node_id);
			if (p)
			{
				const bool rev = (m.node_id & 1) != 0;
				if (R->mappings.size() > firstMap)
				{
					ga_mapping_t& last = R->mappings.back();
					const bool adjacent = prevPiece && prevPiece->orig == p->orig && last.node_id == p->orig * 2 + (rev ? 1 : 0) &&
					                      (rev ? p->start + p->len == prevPiece->start : prevPiece->start + prevPiece->len == p->start);
					if (adjacent)
					{
						last.from_length += m.from_length;
						last.to_length += m.to_length;
						R->edits.insert(R->edits.end(), editFrom, editFrom + editLen);
						prevPiece = p;
						continue;
					}
				}
				if (k == 0) m.offset = (int64_t)(rev ? p->origLen - (p->start + p->len) : p->start) + m.offset;
				m.node_id = p->orig * 2 + (rev ? 1 : 0);
			}
			prevPiece = p;
			m.rank = (int32_t)(R->mappings.size() - firstMap);
			m.edit_seq_off = R->edits.size();
			R->edits.insert(R->edits.end(), editFrom, editFrom + editLen);
			R->mappings.push_back(m);
		}
		for (uint64_t k = 0; k < rr.n_trace; k++)
		{
			ga_trace_item_t t = in->trace[rr.first_trace + k];
			auto it = g->pieces.find((int64_t)t.node_id);
			if (it != g->pieces.end())
			{
				const ga_graph::Piece& p = it->second;
				t.offset = (t.reverse ? p.origLen - (p.start + p.len) : p.start) + t.offset;
				t.node_id = (int32_t)p.orig;
			}
			R->trace.push_back(t);
		}
		rr.first_mapping = firstMap; rr.n_mappings = R->mappings.size() - firstMap;
		rr.first_trace = firstTrace; rr.n_trace = R->trace.size() - firstTrace;
		R->reads.push_back(rr);
		if (in->read_ops)
		{
			// (runs pass through unchanged: types do not depend on where nodes are cut)
			ga_read_ops_t ro = in->read_ops[i];
			const uint64_t from = ro.first_op;
			ro.first_op = R->ops.size();
			R->ops.insert(R->ops.end(), in->ops + from, in->ops + from + ro.n_ops);
			R->readOps.push_back(ro);
		}
		if (in->read_path_seq)
		{
			// (so do the bases: cutting nodes into pieces does not change them)
			ga_read_path_seq_t rp = in->read_path_seq[i];
			const uint64_t from = rp.first_base;
			rp.first_base = R->pathBases.size();
			R->pathBases.insert(R->pathBases.end(), in->path_bases + from, in->path_bases + from + rp.n_bases);
			R->readPath.push_back(rp);
		}
	}
	R->pub.n_reads = R->reads.size(); R->pub.reads = R->reads.data();
	R->pub.n_mappings = R->mappings.size(); R->pub.mappings = R->mappings.data();
	R->pub.n_edit_bytes = R->edits.size(); R->pub.edit_bytes = R->edits.data();
	R->pub.n_trace = R->trace.size(); R->pub.trace = R->trace.data();
	if (in->read_ops) { R->pub.read_ops = R->readOps.data(); R->pub.n_ops = R->ops.size(); R->pub.ops = R->ops.data(); }
	if (in->read_path_seq) { R->pub.read_path_seq = R->readPath.data(); R->pub.n_path_bases = R->pathBases.size(); R->pub.path_bases = R->pathBases.data(); }
	*out = &R->pub;
	return GA_S_OK;
}

}  // extern "C"
