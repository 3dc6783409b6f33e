/* graphaligner_amd.h -- C ABI of the MI355X-native seed-and-extend aligner.
 *
 * Drop-in boundary: the two free functions the reference's driver calls per read,
 *     AlignmentResult AlignOneWay(const AlignmentGraph&, const std::string& seq_id,
 *                                 const std::string& sequence, int initialBandwidth,
 *                                 int rampBandwidth, size_t dynamicRowStart,
 *                                 const std::vector<std::tuple<int,size_t,bool>>& seedHits);
 * (reference GraphAlignerWrapper.h:53-54, called from Aligner.cpp:128,140), plus the graph
 * construction calls its loaders make (AlignmentGraph.h:25-28, BigraphToDigraph.cpp:106-189).
 * A GPU cannot be fed one read per call, so the ABI is batch-first; AlignOneWay is the
 * one-element case (see INTEGRATION.md for the C++ shim a maintainer would add).
 *
 * Plain pointers and sizes only.  No exceptions cross this boundary: every function returns
 * a ga_status, and per-read failures are reported in ga_read_result.status / .failed
 * (replacing ThreadReadAssertion::AssertionFailure, GraphAligner.h assert()s, and the
 * alignmentFailed / INT32_MAX-score convention of GraphAligner.h:636-641).
 *
 * The library needs a gfx950 device: ga_graph_upload / ga_batch_run return GA_E_NO_DEVICE
 * when none is usable.  There is no CPU fallback.
 *
 * Memory the library keeps between calls: a scratch pool, a pinned download buffer, idle device blocks of finished batches and up to
 * six pinned blocks for the batches' copies of the reads per uploaded graph (freed with the graph; a batch's copy of its reads is also
 * what its results' edit_bytes point into, so such a block lives until both the batch and its results are freed), and up to
 * GA_RESULT_POOL_MB (default 4096) of recycled result arrays per process.  Environment knobs, none of them needed:
 * GA_HOST_THREADS (host threads for job building and result assembly; default: the CPUs the process may use), GA_RESULT_POOL_MB,
 * GA_LANES=1/0 (force / forbid the lanes = reads kernel as the first pass; default by the graph's mean node length),
 * GA_LANES_SPREAD=0 / k (full waves / k reads per wave instead of spreading a small batch over all wave slots), GA_DEBUG_PASSES / GA_DEBUG_COLLECT
 * (one line per kernel pass / per host stage on stderr), GA_TEST_WAVE_SLOTS=k (a test hook: no kernel pass starts more than k waves, so that
 * a wave takes one group of reads or one job after the other; unset: as many waves as the device holds).
 */
#ifndef GRAPHALIGNER_AMD_H
#define GRAPHALIGNER_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum ga_status {
	GA_S_OK = 0,
	/* per-read outcomes (ga_read_result.status) */
	GA_S_ASSERTION = 1,         /* the reference's always-on assert() throws for this read (Aligner.cpp:143) */
	GA_S_UNSUPPORTED_BAND = 2,  /* internal: a band of >= 200000 bp, where the reference uses its sparse method (GraphAligner.h:2483); resolved by the
	                               last kernel variant, which carries that method and the backtrace override -- returned only when that pass
	                               could not get its device memory */
	GA_S_BAD_SEED = 3,          /* seed node id unknown: std::out_of_range in the reference (GraphAligner.h:423) */
	GA_S_CAPACITY = 10,         /* device buffers too small even after the automatic retry: a band of more than 4 096 nodes, bit-vector
	                             * (< 200 000 cells) or sparse (>= 200 000 cells), or whose projection heap needs more than 16 384 entries; a
	                             * sparse band of up to 256 nodes with more than 8 192 cells within the bandwidth in one row (e.g. 40 long
	                             * branches met at a ramp width of 70) or more than 65 536 touched columns; a sparse band of 257 to 4 096 nodes
	                             * with more than 131 072 such cells in one row or more than 262 144 touched columns; a traceback move into an
	                             * in-neighbour whose ordinal in the node's in-list is above 62 */
	GA_S_UNSUPPORTED_CYCLE = 20,/* internal: band subgraph has a cycle (GraphAligner.h:2362-2397); resolved by the general kernel variants, not returned */
	GA_S_UNSUPPORTED_RAMP = 21, /* internal: ramp redo (GraphAligner.h:2648-2719) taken; resolved by the general kernel variants, not returned */
	/* call-level errors */
	GA_E_INVALID = 100,
	GA_E_NO_DEVICE = 101,
	GA_E_DEVICE = 102,
	GA_E_NOT_FINALIZED = 103
} ga_status;

/* ---- graph: mirrors AlignmentGraph's public build interface (AlignmentGraph.h:25-28) ---------- */
typedef struct ga_graph ga_graph_t;

ga_graph_t* ga_graph_create(void);                                         /* AlignmentGraph::AlignmentGraph (AlignmentGraph.cpp:12-31) */
void ga_graph_destroy(ga_graph_t* g);
/* AlignmentGraph::AddNode (AlignmentGraph.cpp:47-89): digraph id, ACGT sequence; duplicate ids are ignored */
int ga_graph_add_node(ga_graph_t* g, int64_t digraph_id, const char* seq, size_t len, int reverse_node);
/* AlignmentGraph::AddEdgeNodeId (AlignmentGraph.cpp:91-106): duplicate edges are ignored */
int ga_graph_add_edge(ga_graph_t* g, int64_t from_digraph_id, int64_t to_digraph_id);
/* A FINISHED graph mirrored verbatim: the in- and out-neighbour lists of one node exactly as AlignmentGraph holds them
 * (inNeighbors[i], outNeighbors[i], AlignmentGraph.h:49-50), digraph ids, before ga_graph_finalize.  Both orders are part of the result
 * (traceback ties follow inNeighbors, GraphAligner.h:503; the band's heap is fed in outNeighbors order, :1132-1134, 1153-1155), and a
 * replay of edges grouped by target cannot reproduce both: use this instead of ga_graph_add_edge when copying a built AlignmentGraph.
 * A node given lists here ignores edges added for it with ga_graph_add_edge. */
int ga_graph_set_neighbors(ga_graph_t* g, int64_t digraph_id, const int64_t* in_ids, size_t n_in, const int64_t* out_ids, size_t n_out);
/* the loaders' bidirected -> directed conversion (BigraphToDigraph.cpp:27-56, 58-104):
 * node id -> 2*id (forward) and 2*id+1 (reverse complement); each edge -> two directed edges */
int ga_graph_add_bigraph_node(ga_graph_t* g, int64_t id, const char* seq, size_t len);
int ga_graph_add_bigraph_edge(ga_graph_t* g, int64_t from, int from_start, int64_t to, int to_end);
/* AlignmentGraph::Finalize (AlignmentGraph.cpp:108-154); dbg_overlap = AlignmentGraph::DBGOverlap */
int ga_graph_finalize(ga_graph_t* g, int dbg_overlap);
/* DirectedGraph::StreamGFAGraphFromFile (BigraphToDigraph.cpp:137-189) over an in-memory GFA text; finalizes */
int ga_graph_load_gfa(ga_graph_t* g, const char* text, size_t len);
/* the same with every segment longer than max_node_len cut into a chain of pieces (the first keeps the segment's id, the others get new
 * ids above the largest id of the file): the reference never splits nodes and leaves bands of >= 200 000 bp to its sparse method
 * (GraphAlignerCommon.h:10), so a graph of long segments (a single-contig GFA) only reaches the bit-vector path when cut up.  Blunt
 * graphs only (overlap 0).  This is an OPTION, not the reference's behaviour: alignments are those of the cut graph. */
int ga_graph_load_gfa_split(ga_graph_t* g, const char* text, size_t len, uint32_t max_node_len);
/* where a (bigraph) node id of a split graph comes from: 0 and (original id, start inside it, its length), or 1 when the id is not a piece */
int ga_graph_split_lookup(const ga_graph_t* g, int64_t bigraph_id, int64_t* orig_id, uint64_t* start, uint64_t* orig_len);
/* copy the flattened graph into the HBM of `device` (replicated per GPU; one process per GPU) */
int ga_graph_upload(ga_graph_t* g, int device);
int64_t ga_graph_node_count(const ga_graph_t* g);   /* AlignmentGraph::NodeSize, including the two dummy nodes */
int64_t ga_graph_bp(const ga_graph_t* g);           /* AlignmentGraph::SizeInBp */
/* the columns of a digraph node (2 * bigraph id + strand): a column is the reference's MatrixPosition.first, node_start[node index] +
 * offset, 0 .. ga_graph_bp(g) - 1 with the two dummy nodes' columns first and last.  GA_E_INVALID for an id the graph does not have */
int ga_graph_node_columns(const ga_graph_t* g, int64_t digraph_id, uint64_t* first_column, uint64_t* length);

/* ---- reads and seeds ----------------------------------------------------------------------------- */
typedef struct ga_read {
	const char* name;        /* seq_id */
	const char* sequence;
	size_t length;
} ga_read_t;

typedef struct ga_seed {     /* std::tuple<int,size_t,bool> seedHits (Aligner.cpp:269) */
	int64_t node_id;         /* BIGRAPH node id */
	uint64_t read_pos;       /* query_position */
	int32_t reverse;
	int32_t reserved;
} ga_seed_t;

/* ---- results: flat POD mirror of AlignmentResult (GraphAlignerWrapper.h:10-51) ---------------------- */
typedef struct ga_mapping {  /* vg::Mapping with its single vg::Edit (GraphAligner.h:782-847) */
	int64_t node_id;         /* DIGRAPH id, as the engine returns it; the driver halves it (Aligner.cpp:83-91) */
	int32_t is_reverse;
	int32_t rank;
	int64_t offset;          /* Position.offset: set on the first mapping only */
	int64_t from_length;
	int64_t to_length;
	uint64_t edit_seq_off;   /* Edit.sequence = results->edit_bytes[edit_seq_off .. +to_length) */
} ga_mapping_t;

typedef struct ga_trace_item {   /* AlignmentResult::TraceItem (GraphAlignerWrapper.h:22-31) */
	int32_t node_id;
	int32_t reverse;
	uint64_t offset;
	uint64_t read_pos;
	int32_t type;            /* 1 MATCH 2 MISMATCH 3 INSERTION 4 DELETION 5 FORWARDBACKWARDSPLIT */
	char graph_char;
	char read_char;
	char pad[2];
} ga_trace_item_t;

typedef struct ga_read_result {
	int32_t status;          /* ga_status, per read */
	int32_t failed;          /* AlignmentResult::alignmentFailed */
	int32_t score;           /* vg::Alignment.score; INT32_MAX when failed */
	int32_t reserved;        /* diagnostic: 0 when the first kernel pass finished all of the read's extensions, else the number of the last pass that did */
	uint64_t alignment_start, alignment_end, query_position;
	uint64_t first_mapping, n_mappings;     /* into results->mappings */
	uint64_t first_trace, n_trace;          /* into results->trace (empty unless requested) */
	uint64_t column_updates;                /* band columns computed for this read (first pass) */
} ga_read_result_t;

/* per read with GA_F_OPS: its runs are results->ops[first_op .. first_op + n_ops); the four counts are summed run lengths */
typedef struct ga_read_ops {
	uint64_t first_op;
	uint32_t n_ops, n_match, n_mismatch, n_insertion, n_deletion, reserved;
} ga_read_ops_t;
#define GA_OP_MATCH 1u
#define GA_OP_MISMATCH 2u
#define GA_OP_INSERTION 3u
#define GA_OP_DELETION 4u
#define GA_OP_SPLIT 5u

/* per read with GA_F_PATHSEQ: its path sequence is results->path_bases[first_base .. first_base + n_bases), ASCII A, C, G, T, not
 * terminated; the first n_backward of them are the backward part's (0: the read has no backward part; n_bases: it has no forward part) */
typedef struct ga_read_path_seq {
	uint64_t first_base;
	uint32_t n_bases, n_backward;
} ga_read_path_seq_t;

/* The three arrays behind `reads` are written by several host threads at places fixed before the lengths are known, so they have GAPS:
 * n_mappings / n_edit_bytes / n_trace are the arrays' extents, not counts of valid entries, and the bytes between one read's entries
 * and the next's are unspecified (recycled memory).  Valid entries are exactly those a read's record points at:
 * mappings[first_mapping .. first_mapping + n_mappings), trace[first_trace .. first_trace + n_trace), and per mapping
 * edit_bytes[edit_seq_off .. edit_seq_off + to_length).  Never iterate an array from 0 to its extent. */
typedef struct ga_results {
	size_t n_reads;
	const ga_read_result_t* reads;
	size_t n_mappings;                      /* extent of `mappings` (see above) */
	const ga_mapping_t* mappings;
	size_t n_edit_bytes;                    /* extent of `edit_bytes` */
	const char* edit_bytes;
	size_t n_trace;                         /* extent of `trace` */
	const ga_trace_item_t* trace;
	/* GA_F_OPS only (all three NULL / 0 without the flag): per read its operations as runs; `ops` has gaps like the arrays above */
	const ga_read_ops_t* read_ops;          /* [n_reads] */
	size_t n_ops;                           /* extent of `ops` */
	const uint32_t* ops;                    /* a run: bits 0-2 the type, bits 3-31 the length (at least 1) */
	/* GA_F_PATHSEQ only (all three NULL / 0 without the flag): per read the graph's bases along its alignment; `path_bases` has gaps like
	 * the arrays above: valid bytes are exactly those a read's record points at */
	const ga_read_path_seq_t* read_path_seq; /* [n_reads] */
	size_t n_path_bases;                    /* extent of `path_bases` */
	const char* path_bases;
} ga_results_t;

/* ---- alignment ----------------------------------------------------------------------------------------- */
/* reads[i] owns seeds[seed_offsets[i] .. seed_offsets[i+1]).  flags: GA_F_TRACE fills TraceItem lists; GA_F_OPS fills read_ops / ops.
 *
 * GA_F_OPS: PER-BASE OPERATIONS, RUN-LENGTH CODED ON THE DEVICE.  THE RULE.  ops(read) is the sequence of the `type` fields of the read's
 * TraceItem list -- exactly the list GA_F_TRACE returns (getTraceInfo, GraphAligner.h:690-780) --, types 1 MATCH, 2 MISMATCH, 3 INSERTION,
 * 4 DELETION, 5 FORWARDBACKWARDSPLIT, taken in list order and cut into maximal runs of equal type.  A read with failed != 0 or status !=
 * GA_S_OK has no runs.  A run is one uint32_t: bits 0-2 the type, bits 3-31 the length (at least 1).  The rule is defined by that list
 * and by nothing else.
 * What it means per extension job (one direction of one seed), whose traceback is a stream of moves from its start cell (last row) back
 * to row 0.  Cells at rows >= the job's trace_rows are dropped (the first moves of the stream); K kept cells give K - 1 items, one per
 * kept move, the first cell of a part has none.  A kept move leads from cell A (later, higher row) back to cell B.  A move left (same
 * row) is a DELETION.  A move up (same column) is an INSERTION, unless the column is a node of length 1 that has itself as
 * out-neighbour: the reference counts that step as a diagonal (:742).  A diagonal is a MATCH or a MISMATCH.  Forward job: the item
 * describes A, the characters are seq[pos + row(A)] and the graph base at A.  Backward job: the final trace is the job's reversed and
 * mirrored (reverseTrace, :3026-3037), so the item describes B's mirror cell: the characters are seq[pos - 1 - row(B)] and the base of
 * the other strand's node at the offset counted from its end (the complement of the graph base at B, except in a graph with overlaps,
 * whose strands are cut differently); its stream order is already the final order, a forward job's is its reverse.  The match test is characterMatch
 * (:2039-2110: the read character's IUPAC set against the graph base); a cell on a dummy node matches nothing.  A read's list is the
 * backward part, one SPLIT item when both parts have cells, the forward part; nothing merges across the SPLIT.
 * Where they are made: by two kernels inside ga_batch_run, after the last pass, from the jobs' move bytes where they lie in HBM (a
 * counting launch, a scan, a writing launch: no bound and no capacity miss); ga_batch_collect copies the winning seed's runs.  Two kinds
 * of reads get their runs from the TraceItem list on the host instead, and are counted (ga_batch_ops_stats): a read with a character
 * outside IUPAC, and a read whose forward part the reference does not shift by the seed's position although that is > 0 (:3091-3094).
 * With GA_F_OPS the first pass hands back moves, not node runs, exactly as with GA_F_TRACE.  Without the flag nothing changes: no
 * kernel more, no allocation more.  A back end that does not code operations refuses the prepare with GA_E_INVALID.  Memory kept
 * with the graph from the first flagged batch on: the table of every node's mirror node, 4 bytes per node. */
#define GA_F_TRACE 1u
#define GA_F_OPS 2u
/* GA_F_PILEUP: the batch can be added to a pileup after its collect (ga_batch_pileup_add below, where the rule is).  Like the other two
 * flags it makes the first pass hand back moves, not node runs; it keeps the graph's mirror table (4 bytes per node) with the graph from
 * the first flagged batch on; ga_batch_collect remembers, per aligned read, the winning seed's backward and forward job and whether each
 * part has cells.  Nothing is launched or allocated in ga_batch_run because of the flag, and no result changes.  A back end that cannot
 * add pileups refuses the prepare with GA_E_INVALID. */
#define GA_F_PILEUP 4u
/* GA_F_PATHSEQ: PATH SEQUENCES, THE GRAPH'S BASES ALONG EACH ALIGNMENT, WRITTEN ON THE DEVICE (what the reference's ExtractPathSequence
 * spells out of an alignment's path, and later releases call --corrected-out).  THE RULE.  A read's alignment has up to two parts, the
 * winning seed's backward part and its forward part.  After reverseTrace each part is a list of cells c_0 .. c_{K-1} in read order with
 * K - 1 TraceItems, item k describing c_k (getTraceInfoInner, GraphAligner.h:718-780).  The path sequence of a part is the base of c_0,
 * then the graph_char of every item k >= 1 whose type is MATCH, MISMATCH or DELETION: one base per column the part visits, in read
 * order.  An INSERTION stays in its column and gives nothing.  A step up inside a node of length 1 that has itself as out-neighbour is a
 * diagonal to the reference (:742) and gives that base again.  A cell on either dummy node gives nothing.  A backward part's bases are
 * those of its mirror cells: the other strand's node at the offset counted from its end, read through the graph's mirror table as
 * GA_F_OPS does (the complement is taken only on a back end that was given no table).  A read's path sequence is the backward part's
 * bases followed by the forward part's; n_backward says where the one ends.  The SPLIT item gives nothing: its graph_char is the forward
 * part's c_0, which the forward part already emits.
 * THE SEAM.  The reference extends the two parts independently from the seed node (getSplitAlignment, :2969-3020), so at the seam the two
 * pieces may overlap or leave a gap inside that node, exactly as the reference's mappings do.  Nothing is stitched.
 * A read with failed != 0 or status != GA_S_OK has no sequence (n_bases 0).
 * What it means per extension job, whose traceback is a stream of moves from its start cell back to row 0 (see GA_F_OPS): cells at rows
 * >= the job's trace_rows are dropped; a job with no kept cell has no bases.  Forward job: the item describes cell A, where the move
 * starts; c_0 is the stream's last cell; the bases are stored back to front.  Backward job: the item describes cell B, where the move
 * leads to; c_0 is the first cell of the stream at a row < trace_rows; the bases are stored in stream order.
 * Where they are made: by two kernels inside ga_batch_run, after the last pass and after the GA_F_OPS kernels when both flags are set (a
 * counting launch, the 64-bit scan, a writing launch of one byte per base: no bound, no capacity miss); no read character is looked at.
 * ga_batch_collect copies the winning seed's bytes.  The reads GA_F_OPS leaves to the host get their bases from the host's cell lists
 * (ga_batch_path_seq_stats counts them).  Like the other flags it makes the first pass hand back moves, not node runs, and keeps the
 * mirror table (4 bytes per node) with the graph.  Without the flag nothing changes: no kernel more, no allocation more, no result byte
 * different.  Limits: one byte per base, some one byte per move of the winning jobs (2-bit packing is not done); a job's count is
 * 32-bit.  A back end that does not write path sequences refuses the prepare with GA_E_INVALID.
 * Measured on one MI355X, 50 000 x 10 kb reads (520 M moves, 500 M bases; profiles/path_seq_bench_*.json): the
 * counting and the writing launch 4.2 and 4.9 ms on the linear graph, 6.1 and 6.9 ms on the bubble graph, each 1.0 to 1.5 ms less than the
 * GA_F_OPS launch of the same batch; ga_batch_collect 101 ms for the whole batch (500 MB of bases on top of the moves). */
#define GA_F_PATHSEQ 8u
int ga_align_batch(const ga_graph_t* g, const ga_read_t* reads, size_t n_reads, const ga_seed_t* seeds, const size_t* seed_offsets,
                   int initial_bandwidth, int ramp_bandwidth, uint32_t flags, ga_results_t** out);
void ga_results_free(ga_results_t* r);
/* results over a split graph (ga_graph_load_gfa_split) on the nodes of the GFA file: runs of pieces merged, offsets and trace items remapped */
int ga_results_unsplit(const ga_graph_t* g, const ga_results_t* in, ga_results_t** out);

/* staged form of the same call, for callers that keep inputs resident in HBM and for measurement:
 *   prepare = validate seeds, build extension jobs, upload reads;  run = the device work only;
 *   collect = download + assemble AlignmentResults. */
/* Threading: a graph is read-only once uploaded and may serve any number of batches from any threads.  One batch is used by one thread
 * at a time (prepare -> run -> collect may run on three different threads, as the overlapped pipeline does, but never concurrently on
 * the same batch).  Batches of one graph that RUN concurrently do not share scratch: the first takes the graph's pool, the others
 * allocate their own for the duration. */
typedef struct ga_batch ga_batch_t;
int ga_batch_prepare(const ga_graph_t* g, const ga_read_t* reads, size_t n_reads, const ga_seed_t* seeds, const size_t* seed_offsets,
                     int initial_bandwidth, int ramp_bandwidth, uint32_t flags, ga_batch_t** out);
int ga_batch_run(ga_batch_t* b);
int ga_batch_collect(ga_batch_t* b, ga_results_t** out);
void ga_batch_free(ga_batch_t* b);

typedef struct ga_batch_stats {
	uint64_t n_jobs;             /* extension jobs (read directions) */
	uint64_t column_updates;     /* sum over jobs of band columns computed (unit of work) */
	uint64_t slices;             /* 64-row slices computed */
	uint64_t jobs_retried;       /* jobs the first pass handed to the wave-per-read kernel ladder */
	double kernel_ms;            /* HIP-event time of the extension kernel(s) of the last ga_batch_run, all passes */
	double prep_kernel_ms;       /* HIP-event time of the read-coding kernel */
	uint32_t slots, waves_per_cu;
	uint64_t scratch_bytes;
	uint64_t stamps[8];          /* diagnostic builds (GA_STAMPS) only: shader cycles per phase, summed over jobs */
	double main_kernel_ms;       /* HIP-event time of the first pass alone (the lanes = reads kernel over all jobs) */
	int32_t main_variant;        /* > 0: lanes = reads kernel, band nodes per lane * 1000 + record block * 10 + (1 when 32 lanes per wave);
	                                < 0: wave-per-read kernel with that many band nodes in LDS */
	int32_t reserved;            /* 1: the batch's results need no cell lists (no GA_F_TRACE, one seed at the first base of every read, IUPAC
	                                characters only) and the first-pass kernel handed back node runs instead of one byte per move */
} ga_batch_stats_t;
int ga_batch_stats(const ga_batch_t* b, ga_batch_stats_t* out);

/* a batch prepared with GA_F_OPS (GA_E_INVALID otherwise): the two operations kernels of the last ga_batch_run and, from the last
 * ga_batch_collect, where the reads' runs came from */
typedef struct ga_batch_ops_stats {
	double count_kernel_ms;      /* HIP-event time of the counting launch */
	double write_kernel_ms;      /* ... of the writing launch */
	uint64_t jobs_coded;         /* jobs with status ok, kept slices and move bytes */
	uint64_t moves_read;         /* their moves */
	uint64_t runs_written;       /* their runs */
	uint64_t reads_from_device;  /* aligned reads whose runs are the kernels' */
	uint64_t reads_from_host;    /* reads whose runs -- or whose GA_S_ASSERTION -- came from the TraceItem list on the host (see GA_F_OPS) */
} ga_batch_ops_stats_t;
int ga_batch_ops_stats(const ga_batch_t* b, ga_batch_ops_stats_t* out);

/* a batch prepared with GA_F_PATHSEQ (GA_E_INVALID otherwise): the two path-sequence kernels of the last ga_batch_run and, from the last
 * ga_batch_collect, where the reads' bases came from */
typedef struct ga_batch_path_seq_stats {
	double count_kernel_ms;      /* HIP-event time of the counting launch */
	double write_kernel_ms;      /* ... of the writing launch */
	uint64_t jobs_walked;        /* jobs with status ok, kept slices and move bytes */
	uint64_t moves_read;         /* their moves */
	uint64_t bases_written;      /* their bases (all jobs, not the winning seeds' alone) */
	uint64_t reads_from_device;  /* aligned reads whose bases are the kernels' */
	uint64_t reads_from_host;    /* reads whose bases -- or whose GA_S_ASSERTION -- came from the cell lists on the host */
} ga_batch_path_seq_stats_t;
int ga_batch_path_seq_stats(const ga_batch_t* b, ga_batch_path_seq_stats_t* out);

/* ---- pileups: per-base coverage and allele counts summed on the device -------------------------------- */
/* THE RULE.  A pileup of kind K over an uploaded graph is K planes of uint32_t, one entry per column of the graph (ga_graph_node_columns:
 * column = node_start[node index] + offset, 0 .. ga_graph_bp(g) - 1, the two dummy nodes included).  All entries start at zero.  Adding a
 * batch adds, for every read of the batch's last collect with status == GA_S_OK and failed == 0, every item of the TraceItem list that
 * GA_F_TRACE would return for it (the winning seed's backward part, then the forward part): one to the entry of (the item's plane, the
 * column of digraph node 2 * node_id + reverse at `offset`).  An item whose cell lies on one of the two dummy nodes is not counted (those
 * two columns stay zero); the SPLIT item (type 5) is not counted; the first cell of each part has no item (GA_F_OPS above: K kept cells
 * give K - 1 items) and so no count: up to two cells per read.  The rule is defined by that list and by nothing else.
 *   GA_PILEUP_BASES (K = 8): plane 0 MATCH items; planes 1-4 MISMATCH items whose read_char is A/a, C/c, G/g, T/t; plane 5 MISMATCH items
 *   with any other byte; plane 6 DELETION items; plane 7 INSERTION items, at the column the read stays in.
 *   GA_PILEUP_DEPTH (K = 1): plane 0 = items of type MATCH, MISMATCH or DELETION.
 * Counters wrap modulo 2^32.  Columns are per strand: a backward part's items lie on the other strand's nodes (reverseTrace), exactly as
 * GA_F_OPS mirrors them, and nothing is folded onto the forward strand.  Over a graph loaded with ga_graph_load_gfa_split the columns are
 * the pieces'; ga_graph_split_lookup maps a piece to its segment.
 * Where it is made: one kernel walks the winning jobs' move bytes where they lie in HBM after the last pass (the walk of the GA_F_OPS
 * kernels) and issues one 32-bit atomic add per item; the two kinds of reads that GA_F_OPS takes from the host's TraceItem list (a byte
 * outside IUPAC -- such a read ends as an assertion and adds nothing --, and a forward part the reference leaves unshifted) add through
 * a list of (plane, column) pairs that ga_batch_collect keeps and a second, trivial kernel.  Integer adds: the result does not depend
 * on the order of batches or waves.  Memory: 4 * K bytes per column in the HBM of the graph's device.
 *
 * KIND, PLANES, ENTRIES.  A pileup's kind names what it counts; its planes are the counters one entry has (8 for BASES, 1 for DEPTH and
 * EDGES); its entries are what it counts over: the graph's columns for BASES and DEPTH, the graph's SLOTS for EDGES.  A kind constant is
 * a name, not a size.
 *
 * THE RULE OF GA_PILEUP_EDGES (edge support: which edges the alignments cross).  One plane of uint32_t, one entry per slot.  Slots are the
 * in-neighbour lists of the finalized graph laid end to end in node-index order (a bigraph node is its forward copy, then its reverse copy;
 * within a list the order the edges were added in, a repeated edge once): slot in_off[node] + k is the edge from the node's k-th
 * in-neighbour to the node.  ga_graph_edge_slot_count gives their number, ga_graph_edge_slots the digraph ids (from, to) of each; in-edges
 * of the two dummy nodes, where a graph has them, are slots too and stay zero.  Adding a batch takes, for every read of the last collect
 * with status == GA_S_OK and failed == 0, the same TraceItem list as above, cut at the SPLIT item into parts, and for every two
 * consecutive items a, b of one part adds one at the slot of the directed edge (2 * a.node_id + a.reverse) -> (2 * b.node_id + b.reverse)
 * when b's column is not a's column, b is not the next offset of the same digraph node, neither item lies on a dummy node, and that edge
 * exists in the graph.  So the first cell of each part, which has no item, gives no crossing out of it and nothing is counted across the
 * SPLIT (up to three crossings per read); a turn through a self-loop on a one-base node stays in its column and is not counted; a turn
 * from the last offset of a longer self-loop node to its offset 0 is.  Edges are per strand like columns: a backward part counts on the
 * other strand's edge twin(to) -> twin(from), and nothing is folded on the device (an edge a -> b and its mirror b ^ 1 -> a ^ 1 are one
 * edge of the bigraph; the caller sums the two).  Counters wrap modulo 2^32.  Over a split graph the slots are the pieces' edges.
 * Where it is made: the same walk over the same move bytes, on the same GA_F_PILEUP batches (no other prepare flag; one batch may be
 * added to a BASES, a DEPTH and an EDGES pileup in turn), with one 32-bit atomic add per counted crossing; the reads taken from the host's
 * list add through a list of slot indices.  Memory: 4 bytes per slot for the counters and 4 more for the mirror-slot table (the slot of
 * the other strand's copy of each edge), both in the HBM of the graph's device. */
#define GA_PILEUP_DEPTH 1
#define GA_PILEUP_BASES 8
#define GA_PILEUP_EDGES 32
/* the slots of a finalized graph (no device needed): their number, and the digraph ids of n slots from `first` (GA_E_INVALID for a range
 * past the slot count) */
int ga_graph_edge_slot_count(const ga_graph_t* g, uint64_t* n_slots);
int ga_graph_edge_slots(const ga_graph_t* g, uint64_t first, uint64_t n, int64_t* from_ids, int64_t* to_ids);
typedef struct ga_pileup ga_pileup_t;
/* zeroed; GA_E_INVALID for another kind or a graph that is not uploaded or whose back end has no pileups, GA_E_DEVICE when it does not
 * fit.  A pileup is freed before its graph. */
int ga_pileup_create(const ga_graph_t* g, int kind, ga_pileup_t** out);
void ga_pileup_free(ga_pileup_t* p);
/* reset and download wait for the adds in flight on other threads and hold new ones back while they run */
int ga_pileup_reset(ga_pileup_t* p);
/* adds the alignments of the batch's last collect.  Valid after ga_batch_collect and until the batch's next ga_batch_run or
 * ga_batch_free (with the flag the back end keeps the move bytes in HBM that long).  GA_E_INVALID when the batch lacks GA_F_PILEUP, has
 * not been collected since its last run, or belongs to another graph.  Calling it twice adds twice.  It runs on the batch's own stream
 * and returns when the add is done; two batches may add into one pileup at the same time from two threads, because the adds are atomic. */
int ga_batch_pileup_add(ga_batch_t* b, ga_pileup_t* p);
/* out[plane * n_columns + i] = entry (plane, first_column + i), for every plane of the kind; the range is in entries -- columns, or slots
 * for GA_PILEUP_EDGES -- and GA_E_INVALID when it leaves them */
int ga_pileup_download(const ga_pileup_t* p, uint64_t first_column, uint64_t n_columns, uint32_t* out);
typedef struct ga_pileup_stats {
	double add_kernel_ms;        /* HIP-event time of the last add's kernel(s) */
	uint64_t batches_added;      /* since create or the last reset, like the four below */
	uint64_t reads_from_device;  /* aligned reads whose items the kernel found in the move bytes */
	uint64_t reads_from_host;    /* aligned reads whose items came from the host's list */
	uint64_t jobs_walked, moves_read;
	uint64_t items_added;        /* from both sources; equals the sum over all entries as long as no counter wrapped */
	int32_t kind, reserved;
	uint64_t columns;            /* the entry count: the graph's columns, or its slots for GA_PILEUP_EDGES */
} ga_pileup_stats_t;
int ga_pileup_stats(const ga_pileup_t* p, ga_pileup_stats_t* out);

/* ---- pileup sites: both strands folded and entries selected on the device --------------------------------- */
/* THE RULE.  A site query reads a pileup's counters where they lie in HBM and returns the entries that pass a threshold, so that the
 * download is proportional to the number of sites and not to the graph.  It is defined on the pileup's counters P (plane p of entry e:
 * Pp[e]) and the graph alone.  The query takes ga_site_params_t; GA_E_INVALID unless flags is 0 or GA_SITES_FOLD, min_depth >= 1,
 * 1 <= alt_den <= 65535, alt_num <= alt_den and [first_entry, first_entry + n_entries) lies inside the pileup's entries (min_alt: any
 * value; max_sites 0: no cap).
 *
 * CANDIDATES AND FOLDED COUNTS F[0 .. planes).  All sums are uint32_t, modulo 2^32, like the counters.
 *   BASES and DEPTH, flags 0: every column c of the range is a candidate; F[p] = Pp[c].
 *   BASES and DEPTH, GA_SITES_FOLD: the candidates are the columns of the range that lie on a node with an even digraph id (the forward
 *   copies; the two dummy nodes are no candidates, their counters are zero by the rule of the pileups).  The partner of column c of
 *   `node`, whose other strand is `twin` (digraph id ^ 1) and whose length is len, is c' = node_start[twin] + len - 1 - (c - node_start[node]).
 *     BASES: F[0] = P0[c] + P0[c'];  F[p] = Pp[c] + P(5-p)[c'] for p = 1..4, which maps A <-> T and C <-> G because a read on the reverse
 *     copy carries the complement;  F[5], F[6], F[7] = the same plane's sum.
 *     DEPTH: F[0] = P0[c] + P0[c'].
 *   Preconditions of the fold over columns, checked on the host once per graph and remembered: the graph was finalized with overlap 0 and
 *   every node but the two dummy nodes has a twin of the same length whose bases are its reverse complement; otherwise GA_E_INVALID.  (With
 *   an overlap > 0 the two strands are trimmed at different ends: equal length is then not enough for c' to be the same base.)
 *   Known limit: an INSERTION of a read on the reverse strand is counted at the column that read stays in, whose mirror is one base to the
 *   right of the column at which a forward read would count the same insertion; plane 7 is folded as it is.
 *   EDGES, flags 0: every slot s of the range is a candidate; F[0] = count[s].
 *   EDGES, GA_SITES_FOLD: with m the mirror slot of s (the slot of twin(to) -> twin(from), the table the pileup keeps; none where that
 *   node or edge does not exist), s is a candidate when m is none or s <= m;  F[0] = count[s] + count[m] when m exists and m != s, else
 *   count[s].  (No precondition: a graph of one strand has no mirror slots and folds to itself.)
 *
 * SELECTION, in 64-bit arithmetic.  D = F[0] + ... + F[6] for BASES and F[0] for the other kinds; X = max(D - F[0], F[7]) for BASES and 0
 * for the other kinds.  A candidate is a site when D >= min_depth and X >= min_alt and X * alt_den >= alt_num * D.  So min_alt = 0,
 * alt_num = 0 gives every covered entry; min_alt = 1, alt_num = 0 every entry where a read differs; EDGES with min_depth = t the edges
 * supported t times.
 *
 * RESULT.  The sites in ascending entry order, the first max_sites of them; n_total is how many there were.  The order comes from a
 * scan over per-tile counts, never from an atomic: two calls on the same counters return identical bytes.  Every site carries its entry,
 * counts[8] = F (planes the kind does not have are 0) and what the host finds by binary search in its own node table: for the columns
 * kinds the bigraph node_id (digraph id / 2), offset, reverse (digraph id & 1) and graph_char (the base of the graph at the column,
 * '-' on a dummy node); for EDGES the digraph ids from_id and to_id of the slot.
 * The call holds the pileup exclusively like ga_pileup_download: it waits for adds in flight and holds new ones back.  Each rank's
 * pileup is its own: nothing here merges the pileups of several devices. */
#define GA_SITES_FOLD 1u
typedef struct ga_site_params {
	uint32_t flags;              /* 0 or GA_SITES_FOLD */
	uint32_t alt_num, alt_den;   /* the fraction alt_num / alt_den of the depth that X must reach */
	uint32_t reserved;
	uint64_t min_depth, min_alt;
	uint64_t first_entry, n_entries;
	uint64_t max_sites;          /* 0: no cap */
} ga_site_params_t;
typedef struct ga_site {
	uint64_t entry;
	uint32_t counts[8];
	int64_t node_id;             /* columns kinds: bigraph id;  EDGES: 0 */
	uint32_t offset;
	uint8_t reverse;
	char graph_char;
	uint8_t reserved[2];
	int64_t from_id, to_id;      /* EDGES: digraph ids;  columns kinds: 0 */
} ga_site_t;
typedef struct ga_sites {
	uint64_t n_sites;            /* records in `sites` */
	uint64_t n_total;            /* sites the query found (>= n_sites when max_sites cut them) */
	uint64_t entries_scanned;
	double kernel_ms;            /* HIP events over both launches and the scan between them */
	ga_site_t* sites;
} ga_sites_t;
int ga_pileup_sites(ga_pileup_t* p, const ga_site_params_t* params, ga_sites_t** out);
void ga_sites_free(ga_sites_t* s);

/* ---- seeds found on the device ------------------------------------------------------------------------- */
/* A k-mer index of the uploaded graph and, per batch of reads, up to max_seeds seeds per read in the form ga_align_batch takes.  The rule
 * (DESIGN.md section 10 has it in full): keys are 2 bits per base (A=0 C=1 G=2 T=3, first base most significant); a k-mer is kept when the
 * low sample_shift bits of a fixed 64 -> 32 bit mix of its key are zero, the same test for graph and reads; the index holds (key, node
 * index, offset) of every kept k-mer that lies INSIDE one node (no dummy nodes), ordered by (key, node index, offset).  A read's hits are the
 * index entries of its kept k-mers whose key has between 1 and max_occ entries, in order of read position p, the first max_hits of them.
 * Every node has a linear coordinate lin (forward copy: summed length of the bigraph nodes added before it; reverse copy: minus (that sum
 * + its length - 1)), diag(hit) = lin + offset - p, and support(hit) = hits of the same strand with |p' - p| <= window and |diag' - diag| <=
 * diag_tol.  Hits with p >= 193, length - p >= 193 and support >= min_support are candidates; they are taken greedily by (support
 * descending, p, node index, offset), skipping one of the same strand within diag_tol of a taken one.
 * Two builds.  ga_graph_build_seed_index: the in-node index above; k-mers that span an edge are not in it and nodes shorter than k
 * contribute nothing, so a graph of nodes shorter than k has an empty index.  ga_graph_build_seed_index_walks: the WALK index for graphs
 * of short nodes (variation graphs cut at every variant).  Every base (node, o) of every node but the dummy ones is a start.  o + k <= length:
 * the one k-mer inside the node, as above.  o + k > length (a "tail start"): one k-mer per walk that begins with the node's bases from o
 * and goes on through out-neighbours until k bases are read.  A walk never enters a dummy node; one that reaches a node without
 * out-neighbours before k bases gives nothing; one that enters a node of length 0 gives nothing (so a walk has at most k - 1 edges);
 * cycles and self-loops are walked like any other edge.  A tail start with more than max_walks walks (walks that give a k-mer; not
 * distinct keys) contributes nothing at all and is counted: all or nothing, so the index does not depend on the order of a node's
 * neighbours.  Every kept key gives the entry (key, node index of the START, o), each triple once: walks of one start with equal text
 * give one entry.  Order, lookup, hits, support, candidates and choice are those above; diag uses the start's node and o.  Both strands
 * are nodes, so reverse-complement k-mers come from the reverse nodes' own walks.  The index does not depend on where a sequence is cut
 * into nodes as long as no tail start is skipped; it grows with the variants per k bases (2^v walks over v SNPs).
 * LIMITS: the linear coordinate follows the order in which nodes were added, not topology (unless the topology coordinate below is
 * asked for): it ranks, it never decides an alignment
 * (a wrongly ranked seed costs a wasted extension); a read shorter than 386 bp gets no seed (either direction would be under the 193 bp the
 * reference's engine asserts on, GraphAligner.h:906).
 * ONE SEED PER LOCUS (ga_find_seeds_loci).  Along a long read the diagonal drifts (the read's indels, the file-order coordinate stepping
 * at every bubble), so the second hit ga_find_seeds takes is usually the first one's place again, further along.  ga_find_seeds_loci
 * groups the hits first.  Hits, their order, strand, diag, support, candidates and the truncation at max_hits are those above.  LINK: two
 * different hits i and j are linked when they have the same strand, |p_i - p_j| <= window and |diag_i - diag_j| <= diag_tol (the relation
 * support counts).  LOCUS: a connected component of the link relation over all hits the read keeps after truncation, candidates or not;
 * locus_hits is its size, locus_first_p and locus_last_p the smallest and largest p in it.  SEED HIT of a locus: its first candidate in the
 * order above (support descending, p, node index, offset); a locus without a candidate gives nothing, and n_loci of a read counts the
 * loci that have one.  CHOICE: the loci that have a candidate, ordered by locus_hits descending, then by their seed hits in the order
 * above, are taken greedily up to max_seeds; a locus is skipped when its seed hit has the same strand as an already taken seed hit and
 * lies within diag_tol of it (the skip of ga_find_seeds, kept: it covers one diagonal broken by a gap wider than window).  One seed per
 * taken locus is returned, in that order.  Loci are ranked by size because the best-supported single hit can lie in a partial copy of a
 * repeat: with max_seeds = 1 ga_find_seeds_loci can therefore name a different seed than ga_find_seeds does.  A structural variant longer
 * than diag_tol still splits a locus in two (the coordinate is file order), which costs one extension.
 * TOPOLOGY COORDINATE (ga_graph_set_seed_coordinate with GA_SEED_COORD_TOPOLOGY).  The file-order coordinate is only as good as the
 * file's order: with unsorted ids, alleles appended after the backbone or contigs interleaved, two neighbouring nodes of a walk have
 * unrelated lin and support falls to the hits inside one node.  The topology coordinate is built on the device from the edges.  Nodes
 * are digraph nodes, both strands, by node index; the two dummy nodes take no part and get lin = 0; len(v) is v's length in columns.
 * PARENT: parent(v) is the first entry u of v's in-neighbour list, in its stored order, with u != v and u not a dummy node; a node
 * without one is a root.  CYCLES: on each cycle of the parent relation the node with the smallest node index becomes a root (its
 * parent link is dropped); what remains is a forest.  DEPTH: depth(root) = 0, depth(v) = depth(parent(v)) + len(parent(v)); tree(v)
 * is v's root.  EXTENT of a tree: the maximum of depth(v) + len(v) over its nodes.  BASE: trees are ordered by their root's node
 * index; the first has base 0, each next one base(previous) + extent(previous) + GA_SEED_TREE_GAP.  lin(v) = base(tree(v)) + depth(v),
 * a 64-bit integer, and the strand flag stays digraph id & 1.  Both strands are nodes with their own in-lists, so the reverse strand
 * gets trees of its own and no mirrored sign.  Everything else of the rule (diag, support, link, candidates, choice) is unchanged; only
 * the 8 bytes per node that hold lin change.  The gap keeps hits of different trees from ever being linked or counted as support; this
 * holds while window + diag_tol < GA_SEED_TREE_GAP = 2^20 (two hits within window of each other whose nodes lie in different trees
 * have diagonals at least 2^20 - window apart).
 * LIMITS of the topology coordinate: where a node has in-neighbours of different depth the coordinate follows the first one, and a
 * read through the other allele sees a step of the length difference, as any one-dimensional coordinate must; the cut of a cycle
 * splits the locus of a read that crosses it; a tree that spans an inversion edge has nodes of both strand flags, and support still
 * counts one flag at a time.  While the coordinate is built the device holds 68 bytes per node of work buffers (freed when the call
 * ends) and the scan's temporary storage; every pass takes at most ceil(log2(nodes)) + 1 rounds, one launch each.
 * Memory kept with the graph (freed by ga_graph_destroy or a new ga_graph_upload): the index (16 bytes per entry, 4 per directory bucket, 8
 * per node) and, from the first ga_find_seeds on, the last batch's device buffers and the waves' hit buffers (16 waves per CU x max_hits
 * x 20 bytes: 335 MB at the defaults on 256 CUs).  ga_find_seeds_loci runs 24 waves per CU and keeps 28 bytes more per hit (labels, locus
 * sizes, ends, best candidates and link counts): from its first call on the buffers are 24 waves per CU x max_hits x 48 bytes, 1.2 GB at
 * those figures; a caller of ga_find_seeds alone never pays that.  One
 * ga_find_seeds, ga_find_seeds_loci or index build runs at a time per graph (others wait). */
typedef struct ga_seed_params {
	uint32_t k;             /* 11..31 */
	uint32_t sample_shift;  /* 0..8: one k-mer in 2^sample_shift is kept */
	uint32_t max_occ;       /* keys with more entries are not used */
	uint32_t max_hits;      /* per read; 1..65536 */
	uint32_t window;        /* read positions either side that count as support */
	uint32_t diag_tol;
	uint32_t min_support;
	uint32_t max_seeds;     /* per read; 1..64 */
} ga_seed_params_t;
void ga_seed_params_default(ga_seed_params_t* p);   /* k 15, sample_shift 2, max_occ 8, max_hits 4096, window 1024, diag_tol 64, min_support 2, max_seeds 2 */

/* after ga_graph_upload (GA_E_NOT_FINALIZED / GA_E_NO_DEVICE otherwise); replaces an earlier index of this graph; freed with the graph
 * and dropped by a new ga_graph_upload */
int ga_graph_build_seed_index(ga_graph_t* g, uint32_t k, uint32_t sample_shift);
/* the walk index (see above): max_walks 1..256 (GA_E_INVALID otherwise), 64 is a good default.  Entry numbers are 32-bit: a build whose
 * entries (before equal triples are dropped) would not fit returns GA_E_INVALID; raise sample_shift.  While it is built the device holds
 * 2 x 16 bytes per such entry + 8 per entry for the removal of equal triples.  Replaces an earlier index of either kind, as
 * ga_graph_build_seed_index replaces a walk index. */
int ga_graph_build_seed_index_walks(ga_graph_t* g, uint32_t k, uint32_t sample_shift, uint32_t max_walks);
typedef struct ga_seed_index_stats {
	uint64_t kmers_seen;     /* k-mers inside nodes; walk index: + walk_kmers of ga_seed_walk_stats_t */
	uint64_t entries;        /* kept ones = index entries */
	uint64_t distinct_keys;
	uint64_t bytes;          /* device memory of the index: 16 per entry + directory + 8 per node */
	double build_ms;
	uint32_t k, sample_shift;
} ga_seed_index_stats_t;
int ga_graph_seed_index_stats(const ga_graph_t* g, ga_seed_index_stats_t* out);
typedef struct ga_seed_walk_stats {
	uint64_t tail_starts;          /* starts (node, o) with o + k > length, dummy nodes left out */
	uint64_t tail_starts_skipped;  /* those with more than max_walks walks: nothing of them is in the index */
	uint64_t walk_kmers;           /* walks of the tail starts that were not skipped, before sampling */
	uint64_t duplicates_dropped;   /* kept entries removed because an equal (key, node, offset) was there already */
	uint32_t max_walks, reserved;
} ga_seed_walk_stats_t;
/* GA_E_INVALID when the graph's index is an in-node one (or there is none) */
int ga_graph_seed_index_walk_stats(const ga_graph_t* g, ga_seed_walk_stats_t* out);
/* the index in its order, for tests and tools: the first min(entries, capacity) entries; node INDICES (0 = the dummy start node; bigraph
 * node number i of a graph built with ga_graph_add_bigraph_node alone is 1 + 2i forward, 2 + 2i reverse) */
int ga_graph_seed_index_copy(const ga_graph_t* g, uint64_t* keys, uint32_t* node_indices, uint32_t* offsets, size_t capacity);

/* the coordinate of the current index (see TOPOLOGY COORDINATE above).  Every index build starts in file order.  Called after an index
 * build (GA_E_INVALID without an index or for an unknown kind); it waits for a running ga_find_seeds of the graph and replaces the
 * coordinate in place, the index entries stay.  GA_SEED_COORD_FILE_ORDER puts back exactly the array the build made. */
#define GA_SEED_COORD_FILE_ORDER 0
#define GA_SEED_COORD_TOPOLOGY 1
#define GA_SEED_TREE_GAP (1 << 20)
int ga_graph_set_seed_coordinate(ga_graph_t* g, int kind);
typedef struct ga_seed_coord_stats {
	int32_t kind;            /* GA_SEED_COORD_*; file order: everything below is 0 */
	uint32_t trees;          /* roots of the forest, the cut ones included */
	uint32_t cycles_cut;     /* cycles of the parent relation = roots made by a cut */
	uint32_t cycle_rounds;   /* doubling rounds of the cycle pass: ceil(log2(nodes, dummies included)) when there is a cycle, else the
	                            smallest r with 2^r > parent steps of the longest chain */
	uint32_t depth_rounds;   /* doubling rounds of the depth pass: 0 without an edge, else 1 + the smallest r with 2^r >= those steps */
	uint32_t reserved;
	uint64_t extent_sum;     /* summed extents of the trees: the last tree's end = extent_sum + (trees - 1) * GA_SEED_TREE_GAP */
	double build_ms;         /* wall time of the call's device work */
} ga_seed_coord_stats_t;
int ga_graph_seed_coord_stats(const ga_graph_t* g, ga_seed_coord_stats_t* out);
/* lin of the first min(nodes, capacity) nodes by node index (dummy nodes included), as the index holds it now: for tests and tools */
int ga_graph_seed_coordinate_copy(const ga_graph_t* g, int64_t* lin, size_t capacity);

typedef struct ga_seed_set {
	size_t n_reads;
	const size_t* seed_offsets;   /* n_reads + 1: reads[i] owns seeds[seed_offsets[i] .. seed_offsets[i+1]), as ga_align_batch takes them */
	const ga_seed_t* seeds;
	const uint32_t* support;      /* per seed */
	const uint32_t* n_hits;       /* per read: hits used (<= max_hits) */
	const uint8_t* truncated;     /* per read: 1 when the read had more than max_hits hits */
	double kernel_ms;             /* HIP-event time of the seeding kernel */
	/* ga_find_seeds_loci only (all four NULL in a set returned by ga_find_seeds) */
	const uint32_t* locus_hits;     /* per seed: hits of its locus */
	const uint32_t* locus_first_p;  /* per seed: smallest read position of a hit of its locus */
	const uint32_t* locus_last_p;   /* per seed: largest one */
	const uint32_t* n_loci;         /* per read: loci that have a candidate (>= its seeds) */
} ga_seed_set_t;
/* params == NULL: the defaults.  params->k / sample_shift must be those of the index. */
int ga_find_seeds(const ga_graph_t* g, const ga_read_t* reads, size_t n_reads, const ga_seed_params_t* params, ga_seed_set_t** out);
/* one seed per locus (see above): the same contract, and the set is freed the same way */
int ga_find_seeds_loci(const ga_graph_t* g, const ga_read_t* reads, size_t n_reads, const ga_seed_params_t* params, ga_seed_set_t** out);
void ga_seed_set_free(ga_seed_set_t* s);

/* ---- seeded batches: seeds found and jobs planned on the device, in one call ------------------------------ */
/* ga_batch_prepare_seeded = ga_find_seeds (by_locus != 0: ga_find_seeds_loci) followed by ga_batch_prepare on those seeds, with one upload
 * of the reads and the seeds and the job plan made in HBM.  The batch runs, collects, reports and is freed like
 * one of ga_batch_prepare, and gives the same results.  THE PLAN RULE, on node indices.  Per read of length L, its seeds in the seeder's
 * order; a seed has hit node n and read position p.  twin(n): the node whose digraph id is n's ^ 1, or none.  reverse = id(n) & 1;
 * seedNodeIndex = reverse ? twin(n) : n (the even-id node of the pair); fwNode = n, bwNode = twin(n).  Checks, in this order: no twin:
 * GA_S_BAD_SEED; !(p < L): GA_S_ASSERTION; len(fwNode) != len(bwNode): GA_S_ASSERTION.  Backward part when p > 0, with ovl the graph's
 * dbg_overlap: L < p + ovl, or a character of seq[0 .. p + ovl) that has no complement (CommonUtils.cpp:60-136): GA_S_ASSERTION, the seed
 * is not valid and gets no jobs; else a job of n = p + ovl rows, n_rows = n rounded up to 64, seed_node = bwNode, trace_rows = p.
 * Forward part when p < L - 1: n = L - p rows, n_rows likewise, seed_node = fwNode, trace_rows = n >= ovl ? n - ovl : 0.  rows_off is the
 * running 64-bit sum of n_rows in the order (read, seed, backward before forward).  A read without a seed has no jobs and collects as
 * GA_S_ASSERTION, as with an empty seed list given to ga_batch_prepare.
 * Errors: GA_E_INVALID without a seed index, with params->k / sample_shift other than the index's, and on a back end without the feature.
 * Memory kept with the graph from the first call on: the twin table, 5 bytes per node. */
int ga_batch_prepare_seeded(const ga_graph_t* g, const ga_read_t* reads, size_t n_reads, const ga_seed_params_t* params /* NULL: defaults */, int by_locus,
                            int initial_bandwidth, int ramp_bandwidth, uint32_t flags, ga_batch_t** out);
/* ga_batch_prepare_seeded + ga_batch_run + ga_batch_collect */
int ga_align_reads(const ga_graph_t* g, const ga_read_t* reads, size_t n_reads, const ga_seed_params_t* params, int by_locus,
                   int initial_bandwidth, int ramp_bandwidth, uint32_t flags, ga_results_t** out);
/* the seeds the batch was planned from: the set ga_find_seeds / ga_find_seeds_loci would have returned (free with ga_seed_set_free);
 * GA_E_INVALID for a batch of ga_batch_prepare */
int ga_batch_seeds(const ga_batch_t* b, ga_seed_set_t** out);
/* the plan of ANY batch, for tests and tools: the first min(count, capacity) entries of each kind; a null array is skipped; counts (may
 * be null) receives the numbers of jobs, seeds and fills.  Jobs and fills are in plan order and correspond one to one; a seed's job
 * numbers are -1 where it has no such job; seeds are all reads' seeds in order. */
int ga_batch_plan_copy(const ga_batch_t* b, uint64_t* job_rows_off, uint32_t* job_n_rows, uint32_t* job_seed_node, uint32_t* job_trace_rows, size_t job_capacity,
                       uint64_t* seed_pos, uint32_t* seed_node_index, int32_t* seed_early, uint8_t* seed_valid, int64_t* seed_bw_job, int64_t* seed_fw_job, size_t seed_capacity,
                       uint64_t* fill_read, uint64_t* fill_off, uint64_t* fill_n, uint64_t* fill_padded, uint64_t* fill_pos, uint8_t* fill_backward, size_t fill_capacity,
                       size_t* counts);
typedef struct ga_batch_prepare_stats {
	double seed_kernel_ms;       /* HIP-event time of the seeding kernel */
	double plan_kernel_ms;       /* ... of the plan kernels and their scans */
	double eq_kernel_ms;         /* ... of the read-coding (match word) kernel */
	double host_ms;              /* wall time of the call less the three above */
	uint64_t n_seeds, n_jobs, reads_without_seed;
} ga_batch_prepare_stats_t;
/* GA_E_INVALID for a batch of ga_batch_prepare */
int ga_batch_prepare_stats(const ga_batch_t* b, ga_batch_prepare_stats_t* out);

/* ---- file formats either side of the path (no libprotobuf; zlib only) --------------------------------- */
/* gzip-framed vg.Graph chunks (stream.hpp:24-118) -> graph, as DirectedGraph::StreamVGGraphFromFile
 * (BigraphToDigraph.cpp:106-135): all nodes first, then all edges, then Finalize; DBGOverlap stays 0 */
int ga_graph_load_vg(ga_graph_t* g, const void* bytes, size_t len);
/* seed GAM -> (read name, seed hit): mapping(0).position().node_id / is_reverse, query_position (Aligner.cpp:253-271) */
typedef struct ga_named_seed { const char* read_name; ga_seed_t seed; } ga_named_seed_t;
int ga_gam_decode_seeds(const void* bytes, size_t len, ga_named_seed_t** out, size_t* n);   /* free with ga_bytes_free(*out) */
/* results -> one GAM group of vg.Alignment (Aligner.cpp:301-314); failed reads are skipped (Aligner.cpp:153-164);
 * halve_node_ids applies replaceDigraphNodeIdsWithOriginalNodeIds (Aligner.cpp:83-91) */
int ga_results_encode_gam(const ga_results_t* r, const ga_read_t* reads, int halve_node_ids, void** out, size_t* out_len);
void ga_bytes_free(void* p);

const char* ga_status_string(int status);
const char* ga_version(void);

#ifdef __cplusplus
}
#endif
#endif
