"""ctypes binding over the C ABI declared in include/graphaligner_amd.h.

The product library is graphaligner_amd/libgraphaligner_amd.so (HIP, gfx950).  It has no CPU
path: creating a Graph on a machine without a usable GPU raises.  (tests/ may point this
binding at tests/_build/libga_emul.so, a host emulation of the device program used to check
the device logic in the GPU-less build container.)"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PRODUCT_SO = os.path.join(HERE, "libgraphaligner_amd.so")

STATUS = {0: "OK", 1: "ASSERTION", 2: "UNSUPPORTED_BAND", 3: "BAD_SEED", 10: "CAPACITY", 20: "UNSUPPORTED_CYCLE", 21: "UNSUPPORTED_RAMP",
          100: "E_INVALID", 101: "E_NO_DEVICE", 102: "E_DEVICE", 103: "E_NOT_FINALIZED"}
GA_F_TRACE = 1
GA_F_OPS = 2
GA_F_PILEUP = 4
GA_F_PATHSEQ = 8
GA_PILEUP_DEPTH = 1
GA_PILEUP_BASES = 8
GA_PILEUP_EDGES = 32
# kind, planes and entries are three things (include/graphaligner_amd.h, "pileups"): the counters one entry has, per kind
GA_SITES_FOLD = 1
PILEUP_KINDS = {"bases": GA_PILEUP_BASES, "depth": GA_PILEUP_DEPTH, "edges": GA_PILEUP_EDGES}
PILEUP_PLANES_OF_KIND = {GA_PILEUP_BASES: 8, GA_PILEUP_DEPTH: 1, GA_PILEUP_EDGES: 1}
PILEUP_PLANES = ("match", "mismatch_A", "mismatch_C", "mismatch_G", "mismatch_T", "mismatch_other", "deletion", "insertion")
OP_CODES = {1: "=", 2: "X", 3: "I", 4: "D", 5: "|"}
GA_S_OK = 0
GA_S_ASSERTION = 1
GA_E_INVALID = 100


class GaRead(C.Structure):
    _fields_ = [("name", C.c_char_p), ("sequence", C.c_char_p), ("length", C.c_size_t)]


class GaSeed(C.Structure):
    _fields_ = [("node_id", C.c_int64), ("read_pos", C.c_uint64), ("reverse", C.c_int32), ("reserved", C.c_int32)]


class GaMapping(C.Structure):
    _fields_ = [("node_id", C.c_int64), ("is_reverse", C.c_int32), ("rank", C.c_int32), ("offset", C.c_int64),
                ("from_length", C.c_int64), ("to_length", C.c_int64), ("edit_seq_off", C.c_uint64)]


class GaTraceItem(C.Structure):
    _fields_ = [("node_id", C.c_int32), ("reverse", C.c_int32), ("offset", C.c_uint64), ("read_pos", C.c_uint64),
                ("type", C.c_int32), ("graph_char", C.c_char), ("read_char", C.c_char), ("pad", C.c_char * 2)]


class GaReadResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("failed", C.c_int32), ("score", C.c_int32), ("reserved", C.c_int32),
                ("alignment_start", C.c_uint64), ("alignment_end", C.c_uint64), ("query_position", C.c_uint64),
                ("first_mapping", C.c_uint64), ("n_mappings", C.c_uint64), ("first_trace", C.c_uint64), ("n_trace", C.c_uint64),
                ("column_updates", C.c_uint64)]


class GaResults(C.Structure):
    _fields_ = [("n_reads", C.c_size_t), ("reads", C.POINTER(GaReadResult)), ("n_mappings", C.c_size_t), ("mappings", C.POINTER(GaMapping)),
                ("n_edit_bytes", C.c_size_t), ("edit_bytes", C.POINTER(C.c_char)), ("n_trace", C.c_size_t), ("trace", C.POINTER(GaTraceItem))]


class GaReadOps(C.Structure):
    _fields_ = [("first_op", C.c_uint64), ("n_ops", C.c_uint32), ("n_match", C.c_uint32), ("n_mismatch", C.c_uint32), ("n_insertion", C.c_uint32),
                ("n_deletion", C.c_uint32), ("reserved", C.c_uint32)]


class GaResultsOps(C.Structure):
    """ga_results_t with the three fields GA_F_OPS fills at its end.  Results of batches without the flag are read through GaResults
    alone, so that a library from before those fields (bench.py --lib) is never read past its own struct."""
    _fields_ = GaResults._fields_ + [("read_ops", C.POINTER(GaReadOps)), ("n_ops", C.c_size_t), ("ops", C.POINTER(C.c_uint32))]


class GaReadPathSeq(C.Structure):
    _fields_ = [("first_base", C.c_uint64), ("n_bases", C.c_uint32), ("n_backward", C.c_uint32)]


class GaResultsPathSeq(C.Structure):
    """ga_results_t with the three fields GA_F_PATHSEQ fills behind those of GA_F_OPS.  Read only for batches with that flag, as
    GaResultsOps is"""
    _fields_ = GaResultsOps._fields_ + [("read_path_seq", C.POINTER(GaReadPathSeq)), ("n_path_bases", C.c_size_t), ("path_bases", C.POINTER(C.c_char))]


class GaBatchPathSeqStats(C.Structure):
    _fields_ = [("count_kernel_ms", C.c_double), ("write_kernel_ms", C.c_double), ("jobs_walked", C.c_uint64), ("moves_read", C.c_uint64),
                ("bases_written", C.c_uint64), ("reads_from_device", C.c_uint64), ("reads_from_host", C.c_uint64)]


class GaBatchOpsStats(C.Structure):
    _fields_ = [("count_kernel_ms", C.c_double), ("write_kernel_ms", C.c_double), ("jobs_coded", C.c_uint64), ("moves_read", C.c_uint64),
                ("runs_written", C.c_uint64), ("reads_from_device", C.c_uint64), ("reads_from_host", C.c_uint64)]


class GaPileupStats(C.Structure):
    _fields_ = [("add_kernel_ms", C.c_double), ("batches_added", C.c_uint64), ("reads_from_device", C.c_uint64), ("reads_from_host", C.c_uint64),
                ("jobs_walked", C.c_uint64), ("moves_read", C.c_uint64), ("items_added", C.c_uint64), ("kind", C.c_int32), ("reserved", C.c_int32),
                ("columns", C.c_uint64)]


class GaBatchStats(C.Structure):
    _fields_ = [("n_jobs", C.c_uint64), ("column_updates", C.c_uint64), ("slices", C.c_uint64), ("jobs_retried", C.c_uint64),
                ("kernel_ms", C.c_double), ("prep_kernel_ms", C.c_double), ("slots", C.c_uint32), ("waves_per_cu", C.c_uint32),
                ("scratch_bytes", C.c_uint64), ("stamps", C.c_uint64 * 8), ("main_kernel_ms", C.c_double), ("main_variant", C.c_int32),
                ("reserved", C.c_int32)]


class GaNamedSeed(C.Structure):
    _fields_ = [("read_name", C.c_char_p), ("seed", GaSeed)]


class GaSeedParams(C.Structure):
    _fields_ = [("k", C.c_uint32), ("sample_shift", C.c_uint32), ("max_occ", C.c_uint32), ("max_hits", C.c_uint32), ("window", C.c_uint32),
                ("diag_tol", C.c_uint32), ("min_support", C.c_uint32), ("max_seeds", C.c_uint32)]


class GaSeedIndexStats(C.Structure):
    _fields_ = [("kmers_seen", C.c_uint64), ("entries", C.c_uint64), ("distinct_keys", C.c_uint64), ("bytes", C.c_uint64),
                ("build_ms", C.c_double), ("k", C.c_uint32), ("sample_shift", C.c_uint32)]


class GaSeedWalkStats(C.Structure):
    _fields_ = [("tail_starts", C.c_uint64), ("tail_starts_skipped", C.c_uint64), ("walk_kmers", C.c_uint64), ("duplicates_dropped", C.c_uint64),
                ("max_walks", C.c_uint32), ("reserved", C.c_uint32)]


class GaSeedCoordStats(C.Structure):
    _fields_ = [("kind", C.c_int32), ("trees", C.c_uint32), ("cycles_cut", C.c_uint32), ("cycle_rounds", C.c_uint32), ("depth_rounds", C.c_uint32),
                ("reserved", C.c_uint32), ("extent_sum", C.c_uint64), ("build_ms", C.c_double)]


class GaBatchPrepareStats(C.Structure):
    _fields_ = [("seed_kernel_ms", C.c_double), ("plan_kernel_ms", C.c_double), ("eq_kernel_ms", C.c_double), ("host_ms", C.c_double),
                ("n_seeds", C.c_uint64), ("n_jobs", C.c_uint64), ("reads_without_seed", C.c_uint64)]


SEED_COORDINATES = {"file": 0, "topology": 1}


class GaSeedSet(C.Structure):
    _fields_ = [("n_reads", C.c_size_t), ("seed_offsets", C.POINTER(C.c_size_t)), ("seeds", C.POINTER(GaSeed)), ("support", C.POINTER(C.c_uint32)),
                ("n_hits", C.POINTER(C.c_uint32)), ("truncated", C.POINTER(C.c_uint8)), ("kernel_ms", C.c_double)]


class GaSeedSetLoci(C.Structure):
    """ga_seed_set_t as ga_find_seeds_loci fills it: four more pointers at the end.  Sets of ga_find_seeds are read through GaSeedSet
    alone, so that a library from before those fields (bench.py --lib) is never read past its own struct."""
    _fields_ = GaSeedSet._fields_ + [("locus_hits", C.POINTER(C.c_uint32)), ("locus_first_p", C.POINTER(C.c_uint32)),
                                     ("locus_last_p", C.POINTER(C.c_uint32)), ("n_loci", C.POINTER(C.c_uint32))]


# the seeding entry points, in the product library and in the host emulation (tests/_build/libga_emul.so)
SEED_EXPORTS = ["ga_seed_params_default", "ga_graph_build_seed_index", "ga_graph_seed_index_stats", "ga_graph_seed_index_copy", "ga_find_seeds",
                "ga_seed_set_free", "ga_graph_build_seed_index_walks", "ga_graph_seed_index_walk_stats", "ga_find_seeds_loci",
                "ga_graph_set_seed_coordinate", "ga_graph_seed_coord_stats", "ga_graph_seed_coordinate_copy"]

EXPORTS = ["ga_graph_create", "ga_graph_destroy", "ga_graph_add_node", "ga_graph_add_edge", "ga_graph_add_bigraph_node",
           "ga_graph_add_bigraph_edge", "ga_graph_finalize", "ga_graph_load_gfa", "ga_graph_upload", "ga_graph_node_count", "ga_graph_bp",
           "ga_align_batch", "ga_results_free", "ga_batch_prepare", "ga_batch_run", "ga_batch_collect", "ga_batch_free", "ga_batch_stats",
           "ga_graph_set_neighbors", "ga_graph_load_gfa_split", "ga_graph_split_lookup", "ga_results_unsplit", "ga_graph_load_vg", "ga_gam_decode_seeds", "ga_results_encode_gam", "ga_bytes_free", "ga_status_string", "ga_version"]

_libs = {}


def load(path=None):
    path = path or PRODUCT_SO
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise RuntimeError("%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(hipcc --offload-arch=gfx950); there is no CPU fallback" % path)
    L = C.CDLL(path)
    L.ga_graph_create.restype = C.c_void_p
    L.ga_graph_destroy.argtypes = [C.c_void_p]
    L.ga_graph_add_node.argtypes = [C.c_void_p, C.c_int64, C.c_char_p, C.c_size_t, C.c_int]
    L.ga_graph_add_edge.argtypes = [C.c_void_p, C.c_int64, C.c_int64]
    L.ga_graph_set_neighbors.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    L.ga_graph_add_bigraph_node.argtypes = [C.c_void_p, C.c_int64, C.c_char_p, C.c_size_t]
    L.ga_graph_add_bigraph_edge.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int]
    L.ga_graph_finalize.argtypes = [C.c_void_p, C.c_int]
    L.ga_graph_load_gfa.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    L.ga_graph_load_gfa_split.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_uint32]
    L.ga_graph_split_lookup.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ga_results_unsplit.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.ga_graph_upload.argtypes = [C.c_void_p, C.c_int]
    L.ga_graph_node_count.argtypes = [C.c_void_p]
    L.ga_graph_node_count.restype = C.c_int64
    L.ga_graph_bp.argtypes = [C.c_void_p]
    L.ga_graph_bp.restype = C.c_int64
    L.ga_align_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_void_p]
    L.ga_results_free.argtypes = [C.c_void_p]
    L.ga_batch_prepare.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_void_p]
    L.ga_batch_run.argtypes = [C.c_void_p]
    L.ga_batch_collect.argtypes = [C.c_void_p, C.c_void_p]
    L.ga_batch_free.argtypes = [C.c_void_p]
    L.ga_batch_stats.argtypes = [C.c_void_p, C.c_void_p]
    L.ga_graph_load_vg.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    L.ga_gam_decode_seeds.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.ga_results_encode_gam.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.ga_bytes_free.argtypes = [C.c_void_p]
    L.ga_status_string.argtypes = [C.c_int]
    L.ga_status_string.restype = C.c_char_p
    L.ga_version.restype = C.c_char_p
    if hasattr(L, "ga_batch_ops_stats"):                                   # (bench.py --lib may name a build from before GA_F_OPS)
        L.ga_batch_ops_stats.argtypes = [C.c_void_p, C.c_void_p]
    if hasattr(L, "ga_batch_path_seq_stats"):                              # (bench.py --lib may name a build from before GA_F_PATHSEQ)
        L.ga_batch_path_seq_stats.argtypes = [C.c_void_p, C.c_void_p]
    if hasattr(L, "ga_pileup_create"):                                     # (bench.py --lib may name a build from before GA_F_PILEUP)
        L.ga_graph_node_columns.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        L.ga_pileup_create.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.ga_pileup_free.argtypes = [C.c_void_p]
        L.ga_pileup_free.restype = None
        L.ga_pileup_reset.argtypes = [C.c_void_p]
        L.ga_batch_pileup_add.argtypes = [C.c_void_p, C.c_void_p]
        L.ga_pileup_download.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
        L.ga_pileup_stats.argtypes = [C.c_void_p, C.c_void_p]
    if hasattr(L, "ga_graph_edge_slots"):                                  # (bench.py --lib may name a build from before edge support)
        L.ga_graph_edge_slot_count.argtypes = [C.c_void_p, C.c_void_p]
        L.ga_graph_edge_slots.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
    if hasattr(L, "ga_pileup_sites"):                                      # (bench.py --lib may name a build from before site queries)
        L.ga_pileup_sites.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.ga_sites_free.argtypes = [C.c_void_p]
        L.ga_sites_free.restype = None
    if hasattr(L, "ga_find_seeds"):
        L.ga_seed_params_default.argtypes = [C.c_void_p]
        L.ga_seed_params_default.restype = None
        L.ga_graph_build_seed_index.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
        L.ga_graph_seed_index_stats.argtypes = [C.c_void_p, C.c_void_p]
        if hasattr(L, "ga_graph_build_seed_index_walks"):                  # (bench.py --lib may name a build from before the walk index)
            L.ga_graph_build_seed_index_walks.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
            L.ga_graph_seed_index_walk_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.ga_graph_seed_index_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        L.ga_find_seeds.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        if hasattr(L, "ga_find_seeds_loci"):                               # (nor has such a build seeds per locus)
            L.ga_find_seeds_loci.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        if hasattr(L, "ga_graph_set_seed_coordinate"):                     # (nor the topology coordinate)
            L.ga_graph_set_seed_coordinate.argtypes = [C.c_void_p, C.c_int]
            L.ga_graph_seed_coord_stats.argtypes = [C.c_void_p, C.c_void_p]
            L.ga_graph_seed_coordinate_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.ga_seed_set_free.argtypes = [C.c_void_p]
        L.ga_seed_set_free.restype = None
    if hasattr(L, "ga_batch_plan_copy"):                                   # (bench.py --lib may name a build from before seeded batches)
        L.ga_batch_plan_copy.argtypes = [C.c_void_p] + [C.c_void_p] * 4 + [C.c_size_t] + [C.c_void_p] * 6 + [C.c_size_t] + [C.c_void_p] * 6 + [C.c_size_t, C.c_void_p]
        L.ga_batch_prepare_seeded.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_void_p]
        L.ga_align_reads.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_void_p]
        L.ga_batch_prepare_stats.argtypes = [C.c_void_p, C.c_void_p]
        if hasattr(L, "ga_batch_seeds"):
            L.ga_batch_seeds.argtypes = [C.c_void_p, C.c_void_p]
    _libs[path] = L
    return L


def _check(L, s, what):
    if s != 0:
        raise RuntimeError("%s failed: %s (%d)" % (what, L.ga_status_string(s).decode(), s))


class Graph:
    """AlignmentGraph built the way the reference's loaders build it, then copied to HBM"""

    def __init__(self, nodes=None, edges=None, overlap=0, gfa=None, vg=None, device=0, lib_path=None, split=0):
        self.L = load(lib_path)
        self.h = self.L.ga_graph_create()
        if vg is not None:
            _check(self.L, self.L.ga_graph_load_vg(self.h, vg, len(vg)), "ga_graph_load_vg")
        elif gfa is not None:
            data = gfa.encode() if isinstance(gfa, str) else gfa
            if split:
                _check(self.L, self.L.ga_graph_load_gfa_split(self.h, data, len(data), int(split)), "ga_graph_load_gfa_split")
            else:
                _check(self.L, self.L.ga_graph_load_gfa(self.h, data, len(data)), "ga_graph_load_gfa")
        else:
            for nid, seq in nodes:
                b = seq.encode() if isinstance(seq, str) else seq
                _check(self.L, self.L.ga_graph_add_bigraph_node(self.h, int(nid), b, len(b)), "ga_graph_add_bigraph_node")
            for f, fs, t, te in edges:
                _check(self.L, self.L.ga_graph_add_bigraph_edge(self.h, int(f), int(fs), int(t), int(te)), "ga_graph_add_bigraph_edge")
            _check(self.L, self.L.ga_graph_finalize(self.h, overlap), "ga_graph_finalize")
        _check(self.L, self.L.ga_graph_upload(self.h, device), "ga_graph_upload")

    def __del__(self):
        try:
            self.L.ga_graph_destroy(self.h)
        except Exception:
            pass

    @property
    def node_count(self):
        return self.L.ga_graph_node_count(self.h)

    @property
    def bp(self):
        return self.L.ga_graph_bp(self.h)

    def prepare(self, reads, seeds, bw, ramp=0, flags=0, names=None):
        """reads: list of str (or a ReadSet, then seeds is ignored); seeds: list (one entry per read) of lists of (node, pos, reverse) or a single tuple"""
        return Batch(self, reads, seeds, bw, ramp, flags, names)

    def align(self, reads, seeds, bw, ramp=0, flags=0):
        b = self.prepare(reads, seeds, bw, ramp, flags)
        b.run()
        return b.collect()

    # ---- pileups (include/graphaligner_amd.h: "pileups") ----
    def pileup(self, kind="bases"):
        """counters of this graph that stay on the device: kind "bases" (8 planes per column, binding.PILEUP_PLANES), "depth" (1 plane per
        column) or "edges" (1 plane per slot of edge_slots(): the alignments that cross each directed edge).  Batches prepared with
        GA_F_PILEUP add to it after their collect (Pileup.add)"""
        return Pileup(self, kind)

    def edge_slot_count(self):
        if not hasattr(self.L, "ga_graph_edge_slots"):
            raise RuntimeError("this library has no edge slots")
        n = C.c_uint64()
        _check(self.L, self.L.ga_graph_edge_slot_count(self.h, C.byref(n)), "ga_graph_edge_slot_count")
        return int(n.value)

    def edge_slots(self, first=0, n=None):
        """(from_ids, to_ids): the digraph ids (2 * bigraph id + strand) of the directed edge of every slot -- the in-neighbour lists of
        the graph laid end to end in node-index order --, or of n slots from `first`.  Needs no device"""
        n = self.edge_slot_count() - int(first) if n is None else int(n)
        from_ids, to_ids = np.zeros(max(n, 0), dtype=np.int64), np.zeros(max(n, 0), dtype=np.int64)
        _check(self.L, self.L.ga_graph_edge_slots(self.h, int(first), n, from_ids.ctypes.data_as(C.c_void_p), to_ids.ctypes.data_as(C.c_void_p)), "ga_graph_edge_slots")
        return from_ids, to_ids

    def node_columns(self, digraph_id):
        """(first column, length) of the digraph node 2 * bigraph id + strand"""
        if not hasattr(self.L, "ga_graph_node_columns"):
            raise RuntimeError("this library has no pileups")
        first, length = C.c_uint64(), C.c_uint64()
        _check(self.L, self.L.ga_graph_node_columns(self.h, int(digraph_id), C.byref(first), C.byref(length)), "ga_graph_node_columns")
        return int(first.value), int(length.value)


    # ---- seeds found on the device (include/graphaligner_amd.h: "seeds found on the device") ----
    def _need_seeding(self):
        if not hasattr(self.L, "ga_find_seeds"):
            raise RuntimeError("this library has no seeding entry points")

    def build_seed_index(self, k=15, sample_shift=2, max_walks=0, coordinate="file"):
        """k-mer index of this graph in HBM (replaces an earlier one); returns its statistics.  max_walks 0: k-mers inside nodes;
        1..256: the walk index for graphs of short nodes (k-mers across edges, starts with more walks than that left out).
        coordinate: "file" (the order the nodes were added in) or "topology" (built from the edges: set_seed_coordinate)"""
        self._need_seeding()
        if coordinate not in SEED_COORDINATES:
            raise ValueError("build_seed_index: coordinate must be one of %s" % ", ".join(sorted(SEED_COORDINATES)))
        if max_walks:
            _check(self.L, self.L.ga_graph_build_seed_index_walks(self.h, int(k), int(sample_shift), int(max_walks)), "ga_graph_build_seed_index_walks")
        else:
            _check(self.L, self.L.ga_graph_build_seed_index(self.h, int(k), int(sample_shift)), "ga_graph_build_seed_index")
        if coordinate != "file":
            self.set_seed_coordinate(coordinate)
        return self.seed_index_stats()

    def set_seed_coordinate(self, kind):
        """replaces the linear coordinate of the current index: "file" or "topology" (or GA_SEED_COORD_*: 0, 1); returns the
        statistics of ga_seed_coord_stats_t as a dict.  Every build_seed_index starts in file order again."""
        self._need_seeding()
        if not hasattr(self.L, "ga_graph_set_seed_coordinate"):
            raise RuntimeError("this library has no ga_graph_set_seed_coordinate")
        _check(self.L, self.L.ga_graph_set_seed_coordinate(self.h, int(SEED_COORDINATES.get(kind, kind))), "ga_graph_set_seed_coordinate")
        return self.seed_coord_stats()

    def seed_coord_stats(self):
        self._need_seeding()
        st = GaSeedCoordStats()
        _check(self.L, self.L.ga_graph_seed_coord_stats(self.h, C.byref(st)), "ga_graph_seed_coord_stats")
        return {k: getattr(st, k) for k, _ in st._fields_ if k != "reserved"}

    def seed_coordinate(self):
        """lin of every node by node index (numpy int64; the two dummy nodes at both ends included): for tests and tools"""
        self._need_seeding()
        n = int(self.L.ga_graph_node_count(self.h))
        lin = np.zeros(max(n, 1), dtype=np.int64)
        _check(self.L, self.L.ga_graph_seed_coordinate_copy(self.h, lin.ctypes.data_as(C.c_void_p), n), "ga_graph_seed_coordinate_copy")
        return lin[:n]

    def seed_index_walk_stats(self):
        """tail starts, skipped ones, walk k-mers and dropped duplicates of a walk index (an error for an in-node index)"""
        self._need_seeding()
        st = GaSeedWalkStats()
        _check(self.L, self.L.ga_graph_seed_index_walk_stats(self.h, C.byref(st)), "ga_graph_seed_index_walk_stats")
        return {k: getattr(st, k) for k, _ in st._fields_ if k != "reserved"}

    def seed_index_stats(self):
        self._need_seeding()
        st = GaSeedIndexStats()
        _check(self.L, self.L.ga_graph_seed_index_stats(self.h, C.byref(st)), "ga_graph_seed_index_stats")
        return {k: getattr(st, k) for k, _ in st._fields_}

    def seed_index_entries(self):
        """(keys, node indices, offsets) of the index in its order, as numpy arrays: for tests and tools"""
        n = int(self.seed_index_stats()["entries"])
        keys, nodes, offs = np.zeros(max(n, 1), dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint32)
        _check(self.L, self.L.ga_graph_seed_index_copy(self.h, keys.ctypes.data_as(C.c_void_p), nodes.ctypes.data_as(C.c_void_p),
                                                       offs.ctypes.data_as(C.c_void_p), n), "ga_graph_seed_index_copy")
        return keys[:n], nodes[:n], offs[:n]

    def _seed_params(self, params, what, need_index=True):
        """ga_seed_params_t: the defaults, k and sample_shift of the index, then the fields `params` names.  need_index=False: without
        an index the defaults stay, and the call the parameters go to says that the index is missing"""
        p = GaSeedParams()
        self.L.ga_seed_params_default(C.byref(p))
        st = GaSeedIndexStats()
        status = self.L.ga_graph_seed_index_stats(self.h, C.byref(st))
        if need_index:
            _check(self.L, status, "ga_graph_seed_index_stats")
        if status == 0:
            p.k, p.sample_shift = st.k, st.sample_shift
        for name, v in (params or {}).items():
            if name not in dict(GaSeedParams._fields_):
                raise TypeError("%s: unknown parameter %s" % (what, name))
            setattr(p, name, int(v))
        return p

    # ---- seeded batches (include/graphaligner_amd.h: ga_batch_prepare_seeded) ----
    def prepare_seeded(self, reads, params=None, loci=False, bw=35, ramp=0, flags=0, names=None):
        """a batch whose seeds are found and whose jobs are planned on the device, from one upload of the reads: what
        prepare(reads, find_seeds(reads, loci, **params).seeds, ...) gives, without the round trip.  reads: list of str or a ReadSet
        (its seeds are ignored); params: dict of the ga_seed_params_t fields that differ from the defaults.  A library or back end
        without the feature raises SeededUnsupported."""
        return Batch(self, reads, None, bw, ramp, flags, names, find_seeds=dict(params=params, loci=loci))

    def align_reads(self, reads, params=None, loci=False, bw=35, ramp=0, flags=0):
        b = self.prepare_seeded(reads, params, loci, bw, ramp, flags)
        b.run()
        return b.collect()

    def find_seeds(self, reads, loci=False, **params):
        """reads: list of str.  params: fields of ga_seed_params_t that differ from the defaults (k and sample_shift default to the index's).
        Returns a SeedResult: .seeds = per read a list of (node, pos, reverse), as Graph.prepare / align take them, and the diagnostics.
        loci=True: one seed per locus (ga_find_seeds_loci: the read's hits grouped into connected components first); the result then
        also has .locus_hits, .locus_span and .n_loci."""
        self._need_seeding()
        if loci and not hasattr(self.L, "ga_find_seeds_loci"):
            raise RuntimeError("this library has no ga_find_seeds_loci")
        p = self._seed_params(params, "find_seeds")
        n = len(reads)
        keep = [r.encode() if isinstance(r, str) else r for r in reads]
        arr = (GaRead * max(n, 1))()
        for i, r in enumerate(keep):
            arr[i].name = b""
            arr[i].sequence = r
            arr[i].length = len(r)
        out = C.POINTER(GaSeedSetLoci if loci else GaSeedSet)()
        if loci:
            _check(self.L, self.L.ga_find_seeds_loci(self.h, arr, n, C.byref(p), C.byref(out)), "ga_find_seeds_loci")
        else:
            _check(self.L, self.L.ga_find_seeds(self.h, arr, n, C.byref(p), C.byref(out)), "ga_find_seeds")
        try:
            return _seed_result(out.contents, n, loci)
        finally:
            self.L.ga_seed_set_free(out)


class SeededUnsupported(RuntimeError):
    """ga_batch_prepare_seeded is missing from the library, or it refused with GA_E_INVALID (a back end without the feature, no seed
    index, parameters that do not fit the index): callers with a two-call path fall back to it"""


def _seed_result(S, n, loci):
    offs = np.ctypeslib.as_array(S.seed_offsets, shape=(n + 1,)).astype(np.int64) if n else np.zeros(1, dtype=np.int64)
    total = int(offs[-1])
    res = SeedResult()
    flat = [(S.seeds[i].node_id, S.seeds[i].read_pos, bool(S.seeds[i].reverse)) for i in range(total)]
    sup = [int(S.support[i]) for i in range(total)]
    res.seeds = [flat[offs[i]:offs[i + 1]] for i in range(n)]
    res.support = [sup[offs[i]:offs[i + 1]] for i in range(n)]
    res.n_hits = [int(S.n_hits[i]) for i in range(n)]
    res.truncated = [bool(S.truncated[i]) for i in range(n)]
    res.kernel_ms = S.kernel_ms
    if loci:
        size = [int(S.locus_hits[i]) for i in range(total)]
        span = [(int(S.locus_first_p[i]), int(S.locus_last_p[i])) for i in range(total)]
        res.locus_hits = [size[offs[i]:offs[i + 1]] for i in range(n)]
        res.locus_span = [span[offs[i]:offs[i + 1]] for i in range(n)]
        res.n_loci = [int(S.n_loci[i]) for i in range(n)]
    return res


class SeedResult:
    """what Graph.find_seeds returns: seeds[i] = [(node, pos, reverse), ...] of read i (best first, possibly empty), support[i] the
    seeds' support, n_hits[i] / truncated[i] the read's hit count and whether it was cut at max_hits, kernel_ms the kernel's time.
    With loci=True also locus_hits[i] (per seed: hits of its locus), locus_span[i] (per seed: smallest and largest read position of a
    hit of its locus) and n_loci[i] (loci of the read that have a candidate); None otherwise"""
    seeds = support = n_hits = truncated = None
    locus_hits = locus_span = n_loci = None
    kernel_ms = 0.0


class ReadSet:
    """reads and seeds in the form the C ABI takes them (arrays of ga_read_t / ga_seed_t + CSR offsets): what an application that
    calls the library from C or C++ already holds.  Built once, it can be handed to Graph.prepare any number of times."""

    def __init__(self, reads, seeds, names=None):
        n = len(reads)
        self._keep = [r.encode() if isinstance(r, str) else r for r in reads]
        arr = (GaRead * max(n, 1))()
        self._names = [(names[i].encode() if names is not None else b"read%d" % i) for i in range(n)]
        for i, r in enumerate(self._keep):
            arr[i].name = self._names[i]
            arr[i].sequence = r
            arr[i].length = len(r)
        flat = []
        offs = np.zeros(n + 1, dtype=np.uint64)
        for i, s in enumerate(seeds):
            lst = [s] if (len(s) == 3 and not isinstance(s[0], (tuple, list))) else list(s)
            flat.extend(lst)
            offs[i + 1] = len(flat)
        sarr = (GaSeed * max(len(flat), 1))()
        for i, (node, pos, rev) in enumerate(flat):
            sarr[i].node_id = int(node)
            sarr[i].read_pos = int(pos)
            sarr[i].reverse = int(bool(rev))
        self.arr, self.sarr, self.offs = arr, sarr, offs
        self.n_reads = n
        self.total_bp = sum(len(r) for r in self._keep)


class GaSiteParams(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("alt_num", C.c_uint32), ("alt_den", C.c_uint32), ("reserved", C.c_uint32), ("min_depth", C.c_uint64),
                ("min_alt", C.c_uint64), ("first_entry", C.c_uint64), ("n_entries", C.c_uint64), ("max_sites", C.c_uint64)]


class GaSites(C.Structure):
    _fields_ = [("n_sites", C.c_uint64), ("n_total", C.c_uint64), ("entries_scanned", C.c_uint64), ("kernel_ms", C.c_double), ("sites", C.c_void_p)]


# ga_site_t as a numpy record
SITE_DTYPE = np.dtype([("entry", "<u8"), ("counts", "<u4", (8,)), ("node_id", "<i8"), ("offset", "<u4"), ("reverse", "u1"), ("graph_char", "S1"),
                       ("reserved", "u1", (2,)), ("from_id", "<i8"), ("to_id", "<i8")])
assert SITE_DTYPE.itemsize == 72


class SiteArray(np.ndarray):
    """the records of Pileup.sites() with the query's totals"""
    total = 0
    kernel_ms = 0.0
    entries_scanned = 0


class Pileup:
    """ga_pileup_t: `planes` planes of uint32 counters over `entries` entries -- the graph's columns, or its edge slots for the kind
    "edges" --, in the HBM of the graph's device.  `kind_id` is the library's constant of the kind: a name, not a size"""

    def __init__(self, graph, kind="bases"):
        if kind not in PILEUP_KINDS:
            raise ValueError("pileup kind must be 'bases', 'depth' or 'edges'")
        self.g = graph                     # (a pileup is freed before its graph: the reference keeps the graph alive)
        self.L = graph.L
        if not hasattr(self.L, "ga_pileup_create"):
            raise RuntimeError("this library has no pileups")
        self.kind = kind
        self.kind_id = PILEUP_KINDS[kind]
        self.planes = PILEUP_PLANES_OF_KIND[self.kind_id]
        h = C.c_void_p()
        _check(self.L, self.L.ga_pileup_create(graph.h, self.kind_id, C.byref(h)), "ga_pileup_create")
        self.h = h
        # the entry count is the library's (ga_pileup_stats_t.columns): every buffer handed to a download is sized by it
        self.entries = int(self.stats()["columns"])
        self.columns = self.entries

    def add(self, batch):
        """adds the alignments of the batch's last collect (a batch prepared with GA_F_PILEUP, collected since its last run)"""
        _check(self.L, self.L.ga_batch_pileup_add(batch.h, self.h), "ga_batch_pileup_add")

    def reset(self):
        _check(self.L, self.L.ga_pileup_reset(self.h), "ga_pileup_reset")

    def counts(self, first_column=0, n_columns=None):
        """(planes, entries) uint32 array of the whole pileup, or of n_columns entries (columns; slots for "edges") from first_column"""
        n = self.entries - int(first_column) if n_columns is None else int(n_columns)
        if first_column < 0 or n < 0 or int(first_column) + n > self.entries:
            raise RuntimeError("ga_pileup_download failed: range outside the pileup's %d entries (100)" % self.entries)
        out = np.zeros((self.planes, n), dtype=np.uint32)
        _check(self.L, self.L.ga_pileup_download(self.h, int(first_column), n, out.ctypes.data_as(C.c_void_p)), "ga_pileup_download")
        return out

    def edge_support(self):
        """kind "edges": dict (from_id, to_id) -> count per edge of the bigraph, an edge's two directed copies summed (fold_edge_support
        of Graph.edge_slots() and counts())"""
        if self.kind != "edges":
            raise ValueError("edge_support: not a pileup of kind 'edges'")
        return fold_edge_support(self.g.edge_slots(), self.counts()[0])

    def sites(self, fold=True, min_depth=1, min_alt=0, alt_frac=(0, 1), first=0, n=None, max_sites=0):
        """the entries that pass the thresholds, both strands folded when `fold` (include/graphaligner_amd.h: "pileup sites"), selected
        on the device: a structured array (SITE_DTYPE) in ascending entry order, with .total = the sites found (more than len() when
        max_sites cut them), .kernel_ms and .entries_scanned"""
        if not hasattr(self.L, "ga_pileup_sites"):
            raise RuntimeError("this library has no site queries")
        q = GaSiteParams()
        q.flags = GA_SITES_FOLD if fold else 0
        q.alt_num, q.alt_den = int(alt_frac[0]), int(alt_frac[1])
        q.min_depth, q.min_alt = int(min_depth), int(min_alt)
        q.first_entry = int(first)
        q.n_entries = self.entries - int(first) if n is None else int(n)
        q.max_sites = int(max_sites)
        res = C.POINTER(GaSites)()
        _check(self.L, self.L.ga_pileup_sites(self.h, C.byref(q), C.byref(res)), "ga_pileup_sites")
        try:
            r = res.contents
            out = np.zeros(int(r.n_sites), dtype=SITE_DTYPE).view(SiteArray)
            if r.n_sites:
                C.memmove(out.ctypes.data, r.sites, int(r.n_sites) * SITE_DTYPE.itemsize)
            out.total, out.kernel_ms, out.entries_scanned = int(r.n_total), float(r.kernel_ms), int(r.entries_scanned)
        finally:
            self.L.ga_sites_free(res)
        return out

    def supported_edges(self, min_support=1):
        """kind "edges": the dict of edge_support() restricted to the edges of the bigraph whose folded count is >= min_support (>= 1),
        from one fold query on the device instead of a download of every slot"""
        if self.kind != "edges":
            raise ValueError("supported_edges: not a pileup of kind 'edges'")
        if int(min_support) < 1:
            raise ValueError("supported_edges: min_support must be at least 1")
        out = {}
        for s in self.sites(fold=True, min_depth=int(min_support)):
            a, b = int(s["from_id"]), int(s["to_id"])
            out[min((a, b), (b ^ 1, a ^ 1))] = int(s["counts"][0])
        return out

    def node(self, node_id, reverse=False):
        """(planes, length) array of the node's columns, offset 0 first"""
        if self.kind == "edges":
            raise ValueError("node: a pileup of kind 'edges' has slots, not columns")
        first, length = self.g.node_columns(2 * int(node_id) + (1 if reverse else 0))
        return self.counts(first, length)

    def stats(self):
        st = GaPileupStats()
        _check(self.L, self.L.ga_pileup_stats(self.h, C.byref(st)), "ga_pileup_stats")
        return {k: getattr(st, k) for k, _ in st._fields_ if k != "reserved"}

    def close(self):
        if self.h:
            self.L.ga_pileup_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def fold_edge_support(edge_list, counts):
    """per bidirected edge the summed counts of its two directed edges.  edge_list: the arrays (from_id, to_id) of digraph ids
    (2 * bigraph id + strand) of directed edges; counts: one per edge.  The directed edge a -> b and its mirror b ^ 1 -> a ^ 1 are the two
    strands' copies of one edge of the bigraph and fall under one key, the smaller of the two pairs; an edge listed twice is summed too.
    Returns a dict (from_id, to_id) -> count.  With counts of the alignments that cross each directed edge, an edge of the bigraph is
    supported when its folded count is >= 1"""
    from_id, to_id = (np.asarray(x, dtype=np.int64).reshape(-1) for x in edge_list)
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    if not (len(from_id) == len(to_id) == len(counts)):
        raise ValueError("fold_edge_support: one count per directed edge")
    if not len(counts):
        return {}
    # the smaller of (a, b) and (b ^ 1, a ^ 1), compared as pairs; then one sum per distinct key
    ma, mb = to_id ^ 1, from_id ^ 1
    own = (from_id < ma) | ((from_id == ma) & (to_id <= mb))
    keys = np.stack([np.where(own, from_id, ma), np.where(own, to_id, mb)], axis=1)
    uniq, inverse = np.unique(keys, axis=0, return_inverse=True)
    sums = np.zeros(len(uniq), dtype=np.int64)
    np.add.at(sums, inverse.reshape(-1), counts)
    return {(int(a), int(b)): int(c) for (a, b), c in zip(uniq.tolist(), sums.tolist())}


class Batch:
    def __init__(self, graph, reads, seeds, bw, ramp, flags, names=None, find_seeds=None):
        self.g = graph
        L = self.L = graph.L
        self.loci = None                   # a seeded batch: whether its seeds are per locus
        self.flags = int(flags)
        rs = reads if isinstance(reads, ReadSet) else ReadSet(reads, seeds if find_seeds is None else [[]] * len(reads), names)
        self._rs = rs                      # (the arrays must outlive the batch: GAM encoding reads the names)
        self._arr, self._sarr, self._offs = rs.arr, rs.sarr, rs.offs
        self.n_reads = rs.n_reads
        self.total_bp = rs.total_bp
        h = C.c_void_p()
        if find_seeds is not None:
            if not hasattr(L, "ga_batch_prepare_seeded") or not hasattr(L, "ga_find_seeds"):
                raise SeededUnsupported("this library has no ga_batch_prepare_seeded")
            p = graph._seed_params(find_seeds.get("params"), "prepare_seeded", need_index=False)
            self.loci = bool(find_seeds.get("loci"))
            st = L.ga_batch_prepare_seeded(graph.h, rs.arr, rs.n_reads, C.byref(p), int(self.loci), bw, ramp, flags, C.byref(h))
            if st == 100:
                raise SeededUnsupported("ga_batch_prepare_seeded failed: %s (%d)" % (L.ga_status_string(st).decode(), st))
            _check(L, st, "ga_batch_prepare_seeded")
            self.h = h
            return
        _check(L, L.ga_batch_prepare(graph.h, rs.arr, rs.n_reads, rs.sarr, rs.offs.ctypes.data_as(C.c_void_p), bw, ramp, flags, C.byref(h)), "ga_batch_prepare")
        self.h = h

    def run(self):
        _check(self.L, self.L.ga_batch_run(self.h), "ga_batch_run")

    def stats(self):
        st = GaBatchStats()
        _check(self.L, self.L.ga_batch_stats(self.h, C.byref(st)), "ga_batch_stats")
        d = {k: getattr(st, k) for k, _ in st._fields_}
        d["stamps"] = list(st.stamps)
        return d

    def ops_stats(self):
        """ga_batch_ops_stats_t of a batch prepared with GA_F_OPS as a dict: the two kernels' times, jobs coded, moves read, runs written
        and, from the last collect, how many reads got their runs from the device and from the host"""
        if not hasattr(self.L, "ga_batch_ops_stats"):
            raise RuntimeError("this library has no ga_batch_ops_stats")
        st = GaBatchOpsStats()
        _check(self.L, self.L.ga_batch_ops_stats(self.h, C.byref(st)), "ga_batch_ops_stats")
        return {k: getattr(st, k) for k, _ in st._fields_}

    def path_seq_stats(self):
        """ga_batch_path_seq_stats_t of a batch prepared with GA_F_PATHSEQ as a dict: the two kernels' times, jobs walked, moves read, bases
        written and, from the last collect, how many reads got their bases from the device and from the host"""
        if not hasattr(self.L, "ga_batch_path_seq_stats"):
            raise RuntimeError("this library has no ga_batch_path_seq_stats")
        st = GaBatchPathSeqStats()
        _check(self.L, self.L.ga_batch_path_seq_stats(self.h, C.byref(st)), "ga_batch_path_seq_stats")
        return {k: getattr(st, k) for k, _ in st._fields_}

    def seeds(self):
        """the SeedResult a seeded batch was planned from (what Graph.find_seeds would have returned); an error for other batches"""
        out = C.POINTER(GaSeedSetLoci if self.loci else GaSeedSet)()
        _check(self.L, self.L.ga_batch_seeds(self.h, C.byref(out)), "ga_batch_seeds")
        try:
            return _seed_result(out.contents, self.n_reads, bool(self.loci))
        finally:
            self.L.ga_seed_set_free(out)

    def plan(self):
        """the job plan of any batch, for tests and tools: dict(jobs=..., seeds=..., fills=...) of numpy record arrays with the fields of
        ga_batch_plan_copy"""
        counts = (C.c_size_t * 3)()
        nul = [None]
        _check(self.L, self.L.ga_batch_plan_copy(self.h, *(nul * 4), 0, *(nul * 6), 0, *(nul * 6), 0, counts), "ga_batch_plan_copy")
        nj, ns, nf = (int(c) for c in counts)
        jobs = np.zeros(nj, dtype=[("rows_off", "<u8"), ("n_rows", "<u4"), ("seed_node", "<u4"), ("trace_rows", "<u4")])
        seeds = np.zeros(ns, dtype=[("pos", "<u8"), ("seedNodeIndex", "<u4"), ("early", "<i4"), ("valid", "u1"), ("bwJob", "<i8"), ("fwJob", "<i8")])
        fills = np.zeros(nf, dtype=[("read", "<u8"), ("off", "<u8"), ("n", "<u8"), ("padded", "<u8"), ("pos", "<u8"), ("backward", "u1")])
        cols = []
        for arr, cap in ((jobs, nj), (seeds, ns), (fills, nf)):
            tmp = [np.ascontiguousarray(arr[name]) for name in arr.dtype.names]
            cols.append(tmp)
        args = [c.ctypes.data_as(C.c_void_p) for c in cols[0]] + [nj] + [c.ctypes.data_as(C.c_void_p) for c in cols[1]] + [ns] + \
               [c.ctypes.data_as(C.c_void_p) for c in cols[2]] + [nf]
        _check(self.L, self.L.ga_batch_plan_copy(self.h, *args, None), "ga_batch_plan_copy")
        for arr, tmp in zip((jobs, seeds, fills), cols):
            for name, col in zip(arr.dtype.names, tmp):
                arr[name] = col
        return dict(jobs=jobs, seeds=seeds, fills=fills)

    def prepare_stats(self):
        """ga_batch_prepare_stats_t of a seeded batch as a dict"""
        st = GaBatchPrepareStats()
        _check(self.L, self.L.ga_batch_prepare_stats(self.h, C.byref(st)), "ga_batch_prepare_stats")
        return {k: getattr(st, k) for k, _ in st._fields_}

    def collect_gam(self, halve_node_ids=True):
        """align results as the bytes of a GAM file (what the reference's driver writes, Aligner.cpp:301-314)"""
        out = C.POINTER(GaResults)()
        _check(self.L, self.L.ga_batch_collect(self.h, C.byref(out)), "ga_batch_collect")
        try:
            buf, n = C.c_void_p(), C.c_size_t()
            _check(self.L, self.L.ga_results_encode_gam(out, self._arr, int(halve_node_ids), C.byref(buf), C.byref(n)), "ga_results_encode_gam")
            data = C.string_at(buf, n.value)
            self.L.ga_bytes_free(buf)
            return data
        finally:
            self.L.ga_results_free(out)

    def collect(self, summary=False, unsplit=False):
        """summary=True: per-read numpy record array only (status, failed, score, n_mappings, ...), no Python lists;
        unsplit=True: results of a graph loaded with split=... on the nodes of the GFA file (ga_results_unsplit).  A batch prepared
        with GA_F_OPS: every read's dict also has ops (uint32 array of shape (n, 2): type, length) and op_counts (dict of the four
        summed lengths); with summary=True the return value is (records, op_counts array of shape (reads, 4), list of ops arrays).
        A batch prepared with GA_F_PATHSEQ: every read's dict also has path_seq (bytes: the graph's bases along the alignment, the
        backward part's first) and path_seq_backward (how many of them are the backward part's); with summary=True two more values
        follow the others: the list of path_seq and an array of path_seq_backward"""
        want_ops = bool(self.flags & GA_F_OPS)
        want_path = bool(self.flags & GA_F_PATHSEQ)
        struct = GaResultsPathSeq if want_path else GaResultsOps if want_ops else GaResults
        out = C.POINTER(struct)()
        _check(self.L, self.L.ga_batch_collect(self.h, C.byref(out)), "ga_batch_collect")
        if unsplit:
            merged = C.POINTER(struct)()
            try:
                _check(self.L, self.L.ga_results_unsplit(self.g.h, out, C.byref(merged)), "ga_results_unsplit")
            finally:
                self.L.ga_results_free(out)
            out = merged
        try:
            if summary:
                R = out.contents
                dt = np.dtype([("status", "<i4"), ("failed", "<i4"), ("score", "<i4"), ("reserved", "<i4"), ("alignment_start", "<u8"),
                               ("alignment_end", "<u8"), ("query_position", "<u8"), ("first_mapping", "<u8"), ("n_mappings", "<u8"),
                               ("first_trace", "<u8"), ("n_trace", "<u8"), ("column_updates", "<u8")])
                assert dt.itemsize == C.sizeof(GaReadResult)
                buf = C.string_at(R.reads, R.n_reads * dt.itemsize) if R.n_reads else b""
                recs = np.frombuffer(buf, dtype=dt).copy()
                if not want_ops and not want_path:
                    return recs
                extra = _unpack_ops(R) if want_ops else ()
                return (recs,) + tuple(extra) + (_unpack_path_seq(R) if want_path else ())
            reads = _unpack(out.contents)
            if want_ops:
                counts, runs = _unpack_ops(out.contents)
                for i, r in enumerate(reads):
                    r["ops"] = runs[i]
                    r["op_counts"] = dict(match=int(counts[i, 0]), mismatch=int(counts[i, 1]), insertion=int(counts[i, 2]), deletion=int(counts[i, 3]))
            if want_path:
                seqs, n_backward = _unpack_path_seq(out.contents)
                for i, r in enumerate(reads):
                    r["path_seq"] = seqs[i]
                    r["path_seq_backward"] = int(n_backward[i])
            return reads
        finally:
            self.L.ga_results_free(out)

    def close(self):
        """free the batch now (its device buffers and its copy of the reads go back to the graph's pools)"""
        if self.h:
            self.L.ga_batch_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def status_string(status, lib_path=None):
    return load(lib_path).ga_status_string(int(status)).decode()


def decode_seed_gam(data, lib_path=None):
    """[(read name, (node, pos, reverse)), ...] from the bytes of a seed GAM file (Aligner.cpp:253-271)"""
    L = load(lib_path)
    arr, n = C.POINTER(GaNamedSeed)(), C.c_size_t()
    _check(L, L.ga_gam_decode_seeds(data, len(data), C.byref(arr), C.byref(n)), "ga_gam_decode_seeds")
    out = [(arr[i].read_name.decode(), (arr[i].seed.node_id, arr[i].seed.read_pos, bool(arr[i].seed.reverse))) for i in range(n.value)]
    L.ga_bytes_free(arr)
    return out


def _unpack_ops(R):
    """(counts of shape (reads, 4): match, mismatch, insertion, deletion; per read its runs as a uint32 array of shape (n, 2): type, length)"""
    n = R.n_reads
    counts = np.zeros((n, 4), dtype=np.int64)
    runs = []
    words = np.ctypeslib.as_array(R.ops, shape=(R.n_ops,)) if R.n_ops else np.zeros(0, dtype=np.uint32)
    for i in range(n):
        ro = R.read_ops[i]
        counts[i] = (ro.n_match, ro.n_mismatch, ro.n_insertion, ro.n_deletion)
        w = np.array(words[ro.first_op:ro.first_op + ro.n_ops], dtype=np.uint32)
        runs.append(np.stack([w & 7, w >> 3], axis=1).astype(np.uint32) if len(w) else np.zeros((0, 2), dtype=np.uint32))
    return counts, runs


def _unpack_path_seq(R):
    """(per read its path sequence as bytes, array of the backward parts' lengths)"""
    n = R.n_reads
    seqs, n_backward = [], np.zeros(n, dtype=np.int64)
    for i in range(n):
        rp = R.read_path_seq[i]
        seqs.append(C.string_at(C.addressof(R.path_bases.contents) + rp.first_base, rp.n_bases) if rp.n_bases else b"")
        n_backward[i] = rp.n_backward
    return seqs, n_backward


def ops_string(ops):
    """runs (type, length) as a string such as 254=1X3I2D, with | for the split between the backward and the forward part"""
    return "".join("|" if int(t) == 5 else "%d%s" % (int(n), OP_CODES[int(t)]) for t, n in ops)


def _unpack(R):
    reads = []
    edit = C.string_at(R.edit_bytes, R.n_edit_bytes) if R.n_edit_bytes else b""
    for i in range(R.n_reads):
        r = R.reads[i]
        maps = []
        for k in range(r.first_mapping, r.first_mapping + r.n_mappings):
            m = R.mappings[k]
            maps.append((m.node_id, m.is_reverse, m.offset, m.rank, m.from_length, m.to_length,
                         edit[m.edit_seq_off:m.edit_seq_off + m.to_length].decode()))
        tr = np.zeros((r.n_trace, 7), dtype=np.int64)
        for k in range(r.n_trace):
            t = R.trace[r.first_trace + k]
            tr[k] = (t.node_id, t.offset, t.reverse, t.read_pos, t.type, ord(t.graph_char), ord(t.read_char))
        reads.append(dict(status=r.status, failed=bool(r.failed), score=r.score, alignment_start=r.alignment_start, alignment_end=r.alignment_end,
                          query_position=r.query_position, mappings=maps, trace=tr, columns=r.column_updates, kernel_pass=r.reserved))
    return reads
