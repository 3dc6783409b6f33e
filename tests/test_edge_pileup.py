"""Edge support as a pileup kind (GA_PILEUP_EDGES), without a GPU.  The slot table comes from the library (ga_graph_edge_slots needs no
device: here the host emulation's build of the host code answers) and must be edge_model.slot_table; the edge-support program of
graphaligner_amd/csrc/ga_edges.h -- the shared walk of ga_ops.h with the crossing sink -- is compiled for the host (tests/emul/edges.mk, a
small library of its own) and run over fabricated move streams on small graphs given as in-lists, against edge_stream_model.replay,
with guard words behind the counters; the mirror-slot table of the host library is held against edge_stream_model.mirror_slots; and the
host emulation of the back end, which has no pileups, must refuse the kind.  Whole batches run on the GPU in test_edge_pileup_gpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from graphaligner_amd import binding
import edge_cases as ec
import edge_model as em
import edge_stream_model as esm
import ops_model as om
import parity_common as pc

STREAM_SO = os.path.join(pc.ROOT, "tests", "_build", "libga_edges_emul.so")
GUARD = 0xDEADBEEF
N_GUARD = 64


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(pc.ROOT, "tests", "emul"), "-f", "edges.mk"])
    L = C.CDLL(STREAM_SO)
    L.ga_emul_edges_stream.restype = C.c_long
    L.ga_emul_edges_stream.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                       C.c_uint32, C.c_int, C.c_void_p, C.c_uint64]
    L.ga_emul_edges_mirror.restype = C.c_long
    L.ga_emul_edges_mirror.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


# ---- the slot table from the library ----------------------------------------------------------------------------------------------------
def _library_slots(gg):
    f, t = gg.edge_slots()
    assert f.dtype == np.int64 and len(f) == len(t) == gg.edge_slot_count()
    return list(zip(f.tolist(), t.tolist()))


def test_slot_table_from_the_library():
    """Graph.edge_slots() on the emulated back end is edge_model.slot_table on the eight graphs of test_edge_support.py's cases, on a graph
    with a repeated edge and on one with a repeated node id; a sub-range is the slice of the whole and a range past the slots is refused"""
    emul = pc.emul_lib_path()
    seen = 0
    for name, case in ec.graph_cases().items():
        gg = case.graph(emul)
        got = _library_slots(gg)
        assert got == case.slots, (name, len(got), len(case.slots))
        assert len(set(got)) == len(got) and len(got) > 0, name
        seen += 1
    assert seen == 8
    nodes = [(1, "ACGTAC"), (2, "GGT"), (3, "TTACG"), (2, "AAAAAAA")]                 # (the second node 2 is ignored)
    edges = [(1, False, 2, False), (2, False, 3, False), (1, False, 2, False), (1, False, 3, True), (3, True, 3, False), (2, False, 3, False)]
    gg = binding.Graph(nodes, edges, lib_path=emul)
    want = em.slot_table([n for n, _ in nodes], edges)
    got = _library_slots(gg)
    assert got == want and len(want) == 2 * len({e for e in edges}) - 1      # (3- -> 3+ is its own mirror: one directed edge)
    assert gg.node_columns(2 * 2) == (1 + 2 * 6, 3)
    whole = gg.edge_slots()
    for first, n in ((0, 1), (1, 3), (len(want) - 1, 1), (len(want), 0), (2, 0)):
        f, t = gg.edge_slots(first, n)
        assert (f == whole[0][first:first + n]).all() and (t == whole[1][first:first + n]).all(), (first, n)
    buf = np.zeros(4, dtype=np.int64)
    p = buf.ctypes.data_as(C.c_void_p)
    assert gg.L.ga_graph_edge_slots(gg.h, len(want) - 1, 2, p, p) == 100
    assert gg.L.ga_graph_edge_slots(gg.h, len(want) + 1, 0, p, p) == 100
    assert gg.L.ga_graph_edge_slots(gg.h, 0, 1, None, p) == 100
    assert gg.L.ga_graph_edge_slot_count(gg.h, None) == 100


def _digraph(lib_path, nodes, edges, upload=True):
    """a graph through the digraph-level calls (ga_graph_add_node / ga_graph_add_edge with digraph ids), as binding.Graph holds one"""
    gg = binding.Graph.__new__(binding.Graph)
    gg.L = binding.load(lib_path)
    gg.h = gg.L.ga_graph_create()
    for did, seq in nodes:
        assert gg.L.ga_graph_add_node(gg.h, did, seq.encode(), len(seq), did & 1) == 0
    for f, t in edges:
        assert gg.L.ga_graph_add_edge(gg.h, f, t) == 0
    assert gg.L.ga_graph_finalize(gg.h, 0) == 0
    if upload:
        assert gg.L.ga_graph_upload(gg.h, 0) == 0
    return gg


def test_graph_of_one_strand():
    """a graph whose other strand was never added: every interior node's twin is none.  Its slot table is its in-lists, before and after
    the upload, and making a pileup of kind "edges" -- which builds the mirror-slot table from those twins before the back end is asked
    -- ends in the back end's refusal, not in a read outside the lists; so does it on a graph where only some nodes have both strands"""
    emul = pc.emul_lib_path()
    nodes = [(2, "ACGTACG"), (4, "TTG"), (6, "CCATA")]
    edges = [(2, 4), (4, 6), (2, 6), (4, 6)]
    for upload in (False, True):
        gg = _digraph(emul, nodes, edges, upload)
        assert _library_slots(gg) == [(2, 4), (4, 6), (2, 6)]
    with pytest.raises(RuntimeError, match=r"\(100\)"):
        gg.pileup("edges")
    mixed = _digraph(emul, nodes + [(3, "CGTACGT"), (7, "TATGG")], edges + [(7, 3), (7, 4), (2, 7)])
    assert _library_slots(mixed) == [(2, 4), (7, 4), (4, 6), (2, 6), (7, 3), (2, 7)]
    with pytest.raises(RuntimeError, match=r"\(100\)"):
        mixed.pileup("edges")


def test_back_end_without_pileups_refuses_the_kind():
    """the host emulation has no pileups: "edges" is refused with GA_E_INVALID like the other two kinds, a kind that is none is refused
    before the back end is asked, and the slot table is there all the same"""
    g, reads, seeds = ec.oc.round_edge_batch(8)
    gg = binding.Graph(g.nodes, g.edges, lib_path=pc.emul_lib_path())
    for kind in ("edges", "bases", "depth"):
        with pytest.raises(RuntimeError, match=r"\(100\)"):
            gg.pileup(kind)
    with pytest.raises(ValueError):
        gg.pileup("slots")
    h = C.c_void_p()
    for kind in (0, 3, 16, 31, 33, -1):
        assert gg.L.ga_pileup_create(gg.h, kind, C.byref(h)) == 100
    assert gg.L.ga_pileup_download(None, 0, 0, None) == 100
    assert gg.edge_slot_count() == len(em.slot_table([n for n, _ in g.nodes], g.edges))
    assert binding.PILEUP_PLANES_OF_KIND == {binding.GA_PILEUP_BASES: 8, binding.GA_PILEUP_DEPTH: 1, binding.GA_PILEUP_EDGES: 1}


# ---- fabricated streams: the walk and the adds alone, through the emulation library's test entry point, against edge_stream_model ------
def _arrays(graph):
    node_len, in_lists, twin = graph
    off, nbr = esm.csr(in_lists)
    return np.array(node_len, dtype=np.uint32), off, nbr, np.array(twin, dtype=np.uint32)


def _run_stream(lib, moves, graph, arrays, start, start_row, trace_rows, backward):
    lens, off, nbr, twin = arrays
    entries = int(off[-1])
    mv = np.array(list(moves) + [0], dtype=np.uint8)
    out = np.full(entries + N_GUARD, GUARD, dtype=np.uint32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    n = lib.ga_emul_edges_stream(ptr(mv), len(moves), len(lens), ptr(lens), ptr(off), ptr(nbr), ptr(twin), start[0], start[1], start_row, trace_rows,
                                 int(backward), ptr(out), entries)
    assert n >= 0
    assert (out[entries:] == GUARD).all(), "the words behind the counters were written"
    return out[:entries].astype(np.int64), n


STREAM_KINDS = ["diag", "left", "up", "alternating", "random"]
STREAM_LENGTHS = (0, 1, 63, 64, 65, 4096, 4097)


def _codes(kind, n, rng):
    D_, L_, U_ = om.MOVE_DIAG, om.MOVE_LEFT, om.MOVE_UP
    if kind in ("diag", "left", "up"):
        return [{"diag": D_, "left": L_, "up": U_}[kind]] * n
    if kind == "alternating":
        return [(D_, L_, U_)[i % 3] for i in range(n)]
    return [int(x) for x in rng.choice([D_, D_, D_, L_, U_], size=n)]


def _graphs():
    """name -> (graph, start cell, choose(node, in-degree, rng) -> the ordinal a crossing takes, whether crossings must be counted: True,
    False, or "forward" when only a forward job can count any)"""
    out = {}
    n = 5000
    # a chain of 1-bp nodes: a crossing at every column step, 64 per round
    out["1-bp-chain"] = (esm.doubled([1] * n, [(i, i + 1) for i in range(n - 1)]), (1 + 2 * (n - 1), 0), lambda node, deg, rng: 0, True)
    # one long node: none
    out["one-long-node"] = (esm.doubled([5000], []), (1, 4999), lambda node, deg, rng: 0, False)
    # a chain whose nodes also have a skip edge: ordinals 0 and 1 (3-bp nodes, so a round has crossings and steps inside nodes)
    out["skip-chain"] = (esm.doubled([3] * n, [(i, i + 1) for i in range(n - 1)] + [(i, i + 2) for i in range(n - 2)]), (1 + 2 * (n - 1), 2),
                         lambda node, deg, rng: int(rng.integers(deg)), True)
    # a node with 6 in-neighbours entered through ordinals 4 and 5 (past the four of the node record: the in_nbr path), again and again:
    # a ring  hub <- six 2-bp spokes <- hub
    out["six-in-neighbours"] = (esm.doubled([2] + [2] * 6, [(1 + k, 0) for k in range(6)] + [(0, 1 + k) for k in range(6)]), (1, 1),
                                lambda node, deg, rng: int(rng.integers(4, 6)) if deg == 6 else 0, True)
    # a one-base self-loop (ordinal 1 of the loop node is the loop itself) behind a long node, and a 40-bp one
    for name, loop_len in (("one-base-self-loop", 1), ("40-bp-self-loop", 40)):
        out[name] = (esm.doubled([6000, loop_len, 7], [(0, 1), (1, 1), (1, 2)]), (1 + 2 * 2, 6),
                     lambda node, deg, rng: (1 if rng.integers(64) else 0) if deg == 2 else 0, True)
    # a mirror edge that is missing: a backward job's crossing of it counts nowhere
    out["mirror-edge-missing"] = (esm.doubled([2] * 400, [(i, i + 1) for i in range(399)], drop_mirror_of={(i, i + 1) for i in range(0, 399, 3)}),
                                  (1 + 2 * 399, 1), lambda node, deg, rng: 0, True)
    # interior nodes without a twin (0xffffffff in the middle of the table, not only on the dummy nodes): a graph of one strand alone,
    # where a backward job counts nothing at all, and a chain where every third node's two copies do not know each other
    out["one-strand"] = (esm.one_strand([2] * 2500, [(i, i + 1) for i in range(2499)]), (2500, 1), lambda node, deg, rng: 0, "forward")
    out["some-twins-missing"] = (esm.doubled([2] * 2500, [(i, i + 1) for i in range(2499)], no_twin_of=set(range(1, 2500, 3))),
                                 (1 + 2 * 2499, 1), lambda node, deg, rng: 0, True)
    return out


GRAPHS = _graphs()
NO_FULL_MIRROR = ("mirror-edge-missing", "one-strand", "some-twins-missing")


def test_mirror_slot_table(lib):
    """the host library's table (ga_edge_mirror_slots) on every fabricated graph: the slot of the other strand's copy of each edge, none
    where the mirror edge or an interior node's twin is missing, and the mirror of the mirror is the slot itself"""
    for name, (graph, _, _, _) in GRAPHS.items():
        lens, off, nbr, twin = _arrays(graph)
        got = np.full(int(off[-1]) + 1, GUARD, dtype=np.uint32)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        assert lib.ga_emul_edges_mirror(len(lens), ptr(lens), ptr(off), ptr(nbr), ptr(twin), ptr(got)) == int(off[-1]), name
        want = esm.mirror_slots(graph)
        assert got[-1] == GUARD and (got[:-1] == want).all(), (name, np.flatnonzero(got[:-1] != want)[:5])
        have = np.flatnonzero(want != esm.NONE)
        assert (want[want[have]] == have).all(), name
        assert (len(have) < len(want)) == (name in NO_FULL_MIRROR), name
        if name == "one-strand":
            assert len(want) == 2499 and not len(have)
        if name == "some-twins-missing":
            assert 0 < len(have) < len(want) and (np.array(graph[2])[1:-1] == esm.NONE).sum() == 2 * len(range(1, 2500, 3))


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
@pytest.mark.parametrize("graph_name", list(GRAPHS))
@pytest.mark.parametrize("kind", STREAM_KINDS)
def test_fabricated_streams(lib, kind, graph_name, backward):
    graph, start, choose, must_count = GRAPHS[graph_name]
    arrays = _arrays(graph)
    rng = np.random.default_rng(len(kind) * 37 + len(graph_name) + int(backward))
    counted = 0
    for n in STREAM_LENGTHS:
        moves = esm.route(_codes(kind, n, rng), graph, start, lambda node, deg: choose(node, deg, rng))
        if graph_name != "mirror-edge-missing":
            assert len(moves) == n, (graph_name, n, len(moves))          # (the graph is long enough for every stream length)
        rows = sum(1 for m in moves if m & 3 != om.MOVE_LEFT)
        for cut in (0, 1, 37, 64):            # trace_rows cutting inside a round: the first `cut` rows of the stream are dropped
            start_row = rows
            trace_rows = max(start_row + 1 - cut, 0)
            got, items = _run_stream(lib, moves, graph, arrays, start, start_row, trace_rows, backward)
            want, want_items = esm.replay(moves, graph, start, start_row, trace_rows, backward)
            assert items == want_items and int(got.sum()) == want_items, (kind, graph_name, backward, n, cut, items, want_items)
            assert (got == want).all(), (kind, graph_name, backward, n, cut, np.flatnonzero(got != want)[:5])
            counted += want_items
    expect = must_count is True or (must_count == "forward" and not backward)
    assert (counted > 0) == (expect and kind != "up"), (kind, graph_name, backward, counted)


def test_what_the_fabricated_graphs_reach(lib):
    """the streams above are not vacuous in the ways the cases name: 64 crossings in a round of the 1-bp chain, both ordinals of the skip
    chain, ordinals 4 and 5 of the hub, no count for the one-base loop's own edge and counts for the 40-bp loop's, and on the graph with
    missing mirror edges a backward job counts less than a forward one; with interior twins missing likewise, and nothing on one strand alone"""
    rng = np.random.default_rng(7)
    graph, start, choose, _ = GRAPHS["1-bp-chain"]
    got, n = _run_stream(lib, esm.route([om.MOVE_DIAG] * 130, graph, start, lambda a, b: 0), graph, _arrays(graph), start, 130, 131, False)
    assert n == 129 and got.max() == 1                        # (the stream's last cell has no item: the last crossing is not counted)
    graph, start, choose, _ = GRAPHS["skip-chain"]
    moves = esm.route([om.MOVE_DIAG] * 4000, graph, start, lambda node, deg: choose(node, deg, rng))
    got, n = _run_stream(lib, moves, graph, _arrays(graph), start, 4000, 4001, False)
    _, in_lists, _ = graph
    first = np.concatenate([[0], np.cumsum([len(x) for x in in_lists])])
    ordinal = np.concatenate([np.arange(len(x)) for x in in_lists])
    assert got[ordinal == 0].sum() > 100 and got[ordinal == 1].sum() > 100
    graph, start, choose, _ = GRAPHS["six-in-neighbours"]
    moves = esm.route([om.MOVE_DIAG] * 4000, graph, start, lambda node, deg: choose(node, deg, rng))
    got, n = _run_stream(lib, moves, graph, _arrays(graph), start, 4000, 4001, False)
    hub = int(first[1])
    assert got[hub + 4] > 100 and got[hub + 5] > 100 and not got[hub:hub + 4].any()
    for name, loop_counts in (("one-base-self-loop", False), ("40-bp-self-loop", True)):
        graph, start, choose, _ = GRAPHS[name]
        moves = esm.route([om.MOVE_DIAG] * 4000, graph, start, lambda node, deg: choose(node, deg, rng))
        for backward in (False, True):
            got, n = _run_stream(lib, moves, graph, _arrays(graph), start, 4000, 4001, backward)
            _, in_lists, _ = graph
            first = np.concatenate([[0], np.cumsum([len(x) for x in in_lists])])
            loop_node = 4 if backward else 3                  # (the loop node's reverse copy for a backward job)
            loop_slot = int(first[loop_node]) + in_lists[loop_node].index(loop_node)
            assert (got[loop_slot] > 3) == loop_counts and n > 0, (name, backward, got)
    graph, start, choose, _ = GRAPHS["mirror-edge-missing"]
    moves = esm.route([om.MOVE_DIAG] * 700, graph, start, lambda a, b: 0)
    fw = _run_stream(lib, moves, graph, _arrays(graph), start, 700, 701, False)[1]
    bw = _run_stream(lib, moves, graph, _arrays(graph), start, 700, 701, True)[1]
    assert 0 < bw < fw
    for name, none_backward in (("one-strand", True), ("some-twins-missing", False)):
        graph, start, choose, _ = GRAPHS[name]
        moves = esm.route([om.MOVE_DIAG] * 4000, graph, start, lambda a, b: 0)
        fw = _run_stream(lib, moves, graph, _arrays(graph), start, 4000, 4001, False)[1]
        bw = _run_stream(lib, moves, graph, _arrays(graph), start, 4000, 4001, True)[1]
        assert fw > 1900 and (bw == 0 if none_backward else 0 < bw < fw), (name, fw, bw)
