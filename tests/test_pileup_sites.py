"""Site queries on the CPU: the program of graphaligner_amd/csrc/ga_sites.h compiled for the host (tests/emul/sites.mk: a library of its own
with a component hook over fabricated planes and tables, and a stub back end behind the product's host code) must equal site_model, the
rule in numpy, exactly -- at the smallest shapes where the program can go wrong: tile and round edges, 64 nodes in a round, a twin in
another tile, wrapping sums, the three thresholds at equality, ranges, caps, the four mirror cases of edge slots.  The host code's
refusals and the records' fields are checked through the stub back end; the emulated back end, which has no pileups, must refuse.
Whole batches run on the GPU in test_pileup_sites_gpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from graphaligner_amd import binding
import parity_common as pc
import site_model as sm

SITES_SO = os.path.join(pc.ROOT, "tests", "_build", "libga_sites_emul.so")
NONE = 0x7fffffff
FORWARD = 0x80000000
KIND_ID = {"bases": 8, "depth": 1, "edges": 32}


def ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(pc.ROOT, "tests", "emul"), "-f", "sites.mk"])
    L = C.CDLL(SITES_SO)
    L.ga_emul_sites_tile.restype = C.c_uint32
    L.ga_emul_sites_query.restype = C.c_long
    L.ga_emul_sites_query.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                      C.c_void_p, C.c_uint64, C.c_void_p]
    return L


@pytest.fixture(scope="module")
def T(lib):
    t = int(lib.ga_emul_sites_tile())
    assert t >= 64 and t % 64 == 0
    return t


class Tables:
    """a fabricated graph: (digraph id, length) per node in index order between the two dummy nodes"""

    def __init__(self, nodes):
        ids = [0] + [i for i, _ in nodes] + [0]
        lens = [1] + [n for _, n in nodes] + [1]
        self.node_start, self.twin, self.forward = sm.tables_of_graph(ids, lens)
        self.n_nodes = len(ids)
        self.columns = int(self.node_start[-1])
        t = np.where((self.twin >= 0), self.twin, NONE).astype(np.uint32)
        self.fold_table = (t | np.where(self.forward, FORWARD, 0).astype(np.uint32)).astype(np.uint32)
        self.node_start_u64 = self.node_start.astype(np.uint64)


def bigraph_tables(lengths):
    nodes = []
    for k, n in enumerate(lengths):
        nodes += [(2 * (k + 1), n), (2 * (k + 1) + 1, n)]
    return Tables(nodes)


def run(lib, planes, kind, fold=False, min_depth=1, min_alt=0, alt_frac=(0, 1), first=0, n=None, max_sites=0, tables=None, mirror=None, waves=3):
    planes = np.ascontiguousarray(planes, dtype=np.uint32)
    entries = planes.shape[1]
    n = entries - first if n is None else n
    p32 = np.array([1 if fold else 0, alt_frac[0], alt_frac[1]], dtype=np.uint32)
    p64 = np.array([min_depth, min_alt, first, n, max_sites], dtype=np.uint64)
    cap = n + 1
    recs = np.full((cap, 10), 0xABABABAB, dtype=np.uint32)
    total = C.c_uint64(0)
    mir = None if mirror is None else np.ascontiguousarray(mirror, dtype=np.uint32)
    got = lib.ga_emul_sites_query(ptr(planes), entries, KIND_ID[kind], tables.n_nodes if tables else 0, ptr(tables.node_start_u64) if tables else None,
                                  ptr(tables.fold_table) if tables else None, ptr(mir), ptr(p32), ptr(p64), waves, ptr(recs), cap, C.byref(total))
    assert got >= 0, "the program refused or wrote outside its buffers"
    assert (recs[got:] == 0xABABABAB).all()
    r = recs[:got]
    entry = r[:, 0].astype(np.int64) | (r[:, 1].astype(np.int64) << 32)
    return entry, r[:, 2:].copy(), int(total.value), r.tobytes()


def check(lib, planes, kind, tables=None, mirror=None, **q):
    """the program against the model; returns the sites' entries"""
    want_e, want_F = sm.sites(planes, kind, fold=q.get("fold", False), min_depth=q.get("min_depth", 1), min_alt=q.get("min_alt", 0), alt_frac=q.get("alt_frac", (0, 1)),
                              first=q.get("first", 0), n=q.get("n"), node_start=tables.node_start if tables else None, twin=tables.twin if tables else None,
                              forward=tables.forward if tables else None, mirror=mirror)
    cap = q.get("max_sites", 0)
    keep = len(want_e) if not cap else min(cap, len(want_e))
    for waves in (1, 3):
        e, F, total, _ = run(lib, planes, kind, tables=tables, mirror=mirror, waves=waves, **q)
        assert total == len(want_e), (kind, q, waves)
        assert np.array_equal(e, want_e[:keep]), (kind, q, waves)
        assert np.array_equal(F, want_F[:keep]), (kind, q, waves)
    return want_e


# ---- entry counts and tile edges -------------------------------------------------------------------------------------------------------
def test_every_entry_a_site_around_the_tile_size(lib, T):
    for n in (T - 1, T, T + 1, 2 * T + 1):
        e = check(lib, np.ones((1, n), dtype=np.uint32), "depth")
        assert len(e) == n


def test_sites_at_round_and_tile_edges(lib, T):
    for at in ((63, 64), (T - 1, T)):
        planes = np.zeros((1, 2 * T + 1), dtype=np.uint32)
        planes[0, list(at)] = 3
        e = check(lib, planes, "depth")
        assert e.tolist() == list(at)


def test_empty_tile_between_two_full_ones_and_no_site_at_all(lib, T):
    planes = np.ones((1, 3 * T), dtype=np.uint32)
    planes[0, T:2 * T] = 0
    e = check(lib, planes, "depth")
    assert len(e) == 2 * T and e[T - 1] == T - 1 and e[T] == 2 * T
    assert len(check(lib, np.zeros((8, 2 * T + 5), dtype=np.uint32), "bases")) == 0
    assert len(check(lib, np.ones((8, 2 * T + 5), dtype=np.uint32), "bases", min_depth=8)) == 0


# ---- nodes and mirrors -----------------------------------------------------------------------------------------------------------------
def _random_planes(rng, K, columns):
    planes = rng.integers(0, 4, size=(K, columns)).astype(np.uint32)
    planes[:, rng.random(columns) < 0.4] = 0
    planes[:, 0] = 0
    planes[:, -1] = 0
    return planes


QUERIES = [dict(min_depth=1, min_alt=0), dict(min_depth=1, min_alt=1), dict(min_depth=2, min_alt=1, alt_frac=(1, 4)), dict(min_depth=5, min_alt=2, alt_frac=(1, 3))]


@pytest.mark.parametrize("kind", ["bases", "depth"])
def test_one_base_nodes_64_in_a_round(lib, T, kind):
    tables = bigraph_tables([1] * (T + 40))
    planes = _random_planes(np.random.default_rng(1), KIND_ID[kind], tables.columns)
    for q in QUERIES:
        for fold in (True, False):
            e = check(lib, planes, kind, tables=tables, fold=fold, **q)
        if q["min_depth"] == 1 and q["min_alt"] == 0:
            assert len(e) > 64


@pytest.mark.parametrize("kind", ["bases", "depth"])
def test_node_longer_than_a_tile_with_its_twin_in_another(lib, T, kind):
    tables = bigraph_tables([5, T + 100, 1, 1, 70, 3 * T + 7, 64, 63, 2])
    planes = _random_planes(np.random.default_rng(2), KIND_ID[kind], tables.columns)
    for q in QUERIES:
        check(lib, planes, kind, tables=tables, fold=True, **q)
        check(lib, planes, kind, tables=tables, fold=False, **q)
    both = sm.both_strands(planes, kind, check(lib, planes, kind, tables=tables, fold=True), tables.node_start, tables.twin)
    assert both.any()


def test_graph_of_one_strand_unfolded_and_folded_to_nothing(lib, T):
    tables = Tables([(2 * k, 1 + k % 90) for k in range(1, 60)])
    planes = _random_planes(np.random.default_rng(3), 8, tables.columns)
    assert len(check(lib, planes, "bases", tables=tables, fold=False)) > 0
    assert len(check(lib, planes, "bases", tables=tables, fold=True)) == 0       # (no node has a twin: no candidate; the host refuses such a graph)


# ---- folded counts ---------------------------------------------------------------------------------------------------------------------
def _primes(n):
    out, k = [], 2
    while len(out) < n:
        if all(k % p for p in out if p * p <= k):
            out.append(k)
        k += 1
    return out


def test_distinct_primes_show_the_permutation(lib):
    tables = bigraph_tables([3, 4])
    planes = np.array(_primes(8 * tables.columns), dtype=np.uint32).reshape(8, tables.columns)
    e, F, total, _ = run(lib, planes, "bases", fold=True, tables=tables)
    check(lib, planes, "bases", tables=tables, fold=True)
    assert e.tolist() == [1, 2, 3, 7, 8, 9, 10] and total == 7
    # column 1 = node 1 offset 0; its partner is the twin's last column, 4 + 3 - 1 = 6
    c, c2 = 1, 6
    assert F[0].tolist() == [int(planes[0, c] + planes[0, c2]), int(planes[1, c] + planes[4, c2]), int(planes[2, c] + planes[3, c2]), int(planes[3, c] + planes[2, c2]),
                             int(planes[4, c] + planes[1, c2]), int(planes[5, c] + planes[5, c2]), int(planes[6, c] + planes[6, c2]), int(planes[7, c] + planes[7, c2])]
    # column 8 = node 3 (start 7, length 4) offset 1; its partner 11 + 4 - 1 - 1 = 13
    assert F[4, 1] == planes[1, 8] + planes[4, 13] and F[4, 7] == planes[7, 8] + planes[7, 13]


def test_counter_of_all_ones_folded_with_two_wraps(lib):
    tables = bigraph_tables([2])
    planes = np.zeros((1, tables.columns), dtype=np.uint32)
    planes[0, 1], planes[0, 4] = 0xffffffff, 2               # column 1 and its partner 3 + 2 - 1 - 0
    e, F, _, _ = run(lib, planes, "depth", fold=True, tables=tables)
    check(lib, planes, "depth", tables=tables, fold=True)
    assert e.tolist() == [1] and F[0, 0] == 1
    b = np.zeros((8, tables.columns), dtype=np.uint32)
    b[1, 1], b[4, 4] = 0xffffffff, 2
    e, F, _, _ = run(lib, b, "bases", fold=True, tables=tables)
    check(lib, b, "bases", tables=tables, fold=True)
    assert e.tolist() == [1] and F[0].tolist() == [0, 1, 0, 0, 0, 0, 0, 0]


# ---- threshold arithmetic --------------------------------------------------------------------------------------------------------------
def test_each_condition_at_equality_and_one_below(lib):
    planes = np.zeros((8, 3), dtype=np.uint32)
    planes[:, 1] = [6, 1, 0, 1, 0, 0, 2, 3]                  # D = 10, X = max(4, 3) = 4
    planes[:, 2] = [7, 0, 0, 0, 0, 0, 1, 5]                  # D = 8, X = max(1, 5) = 5: the insertions decide
    def at(**q):
        return check(lib, planes, "bases", **q).tolist()
    assert at(min_depth=10) == [1] and at(min_depth=11) == [] and at(min_depth=8) == [1, 2] and at(min_depth=9) == [1]
    assert at(min_alt=4) == [1, 2] and at(min_alt=5) == [2] and at(min_alt=6) == []
    assert at(alt_frac=(2, 5)) == [1, 2] and at(alt_frac=(41, 100)) == [2]        # 4 * 5 = 2 * 10;  4 * 100 < 41 * 10
    assert at(alt_frac=(5, 8)) == [2] and at(alt_frac=(51, 80)) == []             # 5 * 8 = 5 * 8;   5 * 80 < 51 * 8
    d = np.array([[0, 4, 5]], dtype=np.uint32)
    assert check(lib, d, "depth", min_depth=5).tolist() == [2] and check(lib, d, "depth", min_depth=4).tolist() == [1, 2]
    assert check(lib, d, "depth", min_depth=1, min_alt=1).tolist() == []          # (X is 0 for the kinds without alleles)
    assert check(lib, d, "depth", min_depth=1, alt_frac=(1, 65535)).tolist() == []


def test_depth_near_seven_times_two_to_the_32(lib):
    planes = np.zeros((8, 2), dtype=np.uint32)
    planes[:7, 1] = 0xffffffff
    D = 7 * 0xffffffff
    assert check(lib, planes, "bases", min_depth=D).tolist() == [1]
    assert check(lib, planes, "bases", min_depth=D + 1).tolist() == []
    assert check(lib, planes, "bases", min_alt=6 * 0xffffffff).tolist() == [1]
    assert check(lib, planes, "bases", min_alt=6 * 0xffffffff + 1).tolist() == []
    # X / D = 6 / 7: 65535 * 6 / 7 = 56172.86
    assert check(lib, planes, "bases", alt_frac=(56172, 65535)).tolist() == [1]
    assert check(lib, planes, "bases", alt_frac=(56173, 65535)).tolist() == []


# ---- ranges and caps -------------------------------------------------------------------------------------------------------------------
def test_ranges_inside_a_node_and_a_round_and_an_empty_one(lib, T):
    tables = bigraph_tables([200, 3, T + 11])
    planes = _random_planes(np.random.default_rng(4), 8, tables.columns)
    for first, n in ((17, 30), (17, 100), (150, T + 200), (1, tables.columns - 2), (tables.columns - 1, 1), (tables.columns, 0), (40, 0)):
        for fold in (True, False):
            e = check(lib, planes, "bases", tables=tables, fold=fold, first=first, n=n)
            assert ((e >= first) & (e < first + n)).all()
            if n == 0:
                assert len(e) == 0


def test_max_sites(lib, T):
    planes = np.zeros((1, 2 * T + 40), dtype=np.uint32)
    planes[0, ::3] = 1
    total = len(check(lib, planes, "depth"))
    assert total > T // 3 + 10
    for cap in (1, total - 1, total, total + 5, 0, T // 3 + 5):
        check(lib, planes, "depth", max_sites=cap)


# ---- edges -----------------------------------------------------------------------------------------------------------------------------
def test_edge_slots_four_mirror_cases(lib, T):
    n = T + 70
    rng = np.random.default_rng(5)
    mirror = np.full(n, 0xffffffff, dtype=np.uint32)         # none
    mirror[5] = 5                                            # its own mirror
    pairs = [(1, 9), (10, 2), (63, 64), (T - 1, T), (T + 1, 7)]
    for a, b in pairs:
        mirror[a], mirror[b] = b, a
    counts = rng.integers(0, 3, size=(1, n)).astype(np.uint32)
    counts[0, [5, 1, 9, 63, 64, T - 1]] = [4, 1, 2, 1, 0, 0xffffffff]
    counts[0, T] = 3
    for t in (1, 2, 3, 5):
        e = check(lib, counts, "edges", mirror=mirror, fold=True, min_depth=t)
        check(lib, counts, "edges", mirror=mirror, fold=False, min_depth=t)
        assert not set(e.tolist()) & {9, 10, 64, T, T + 1}       # (the larger slot of a pair is no candidate)
    e, F, _, _ = run(lib, counts, "edges", fold=True, mirror=mirror)
    by = dict(zip(e.tolist(), F[:, 0].tolist()))
    assert by[5] == 4 and by[1] == 3 and by[63] == 1 and by[T - 1] == 2      # (own mirror: counted once; 0xffffffff + 3 wraps to 2)
    assert sm.both_strands(counts, "edges", e, mirror=mirror).any()


# ---- determinism -----------------------------------------------------------------------------------------------------------------------
def test_same_query_twice_gives_identical_bytes(lib, T):
    tables = bigraph_tables([T // 2, 1, 1, 1, T + 3])
    planes = _random_planes(np.random.default_rng(6), 8, tables.columns)
    a = run(lib, planes, "bases", fold=True, tables=tables, waves=3)
    b = run(lib, planes, "bases", fold=True, tables=tables, waves=3)
    c = run(lib, planes, "bases", fold=True, tables=tables, waves=7)
    assert a[2] > 0 and a[3] == b[3] == c[3]


# ---- the product's host code against the stub back end ---------------------------------------------------------------------------------
def _digraph(nodes, edges, overlap=0):
    """a graph through the digraph-level calls of the stub library: nodes (digraph id, sequence, reverse)"""
    L = binding.load(SITES_SO)
    g = binding.Graph.__new__(binding.Graph)
    g.L = L
    g.h = L.ga_graph_create()
    for i, seq, rev in nodes:
        assert L.ga_graph_add_node(g.h, i, seq.encode(), len(seq), rev) == 0
    for a, b in edges:
        assert L.ga_graph_add_edge(g.h, a, b) == 0
    assert L.ga_graph_finalize(g.h, overlap) == 0
    assert L.ga_graph_upload(g.h, 0) == 0
    return g


def _poke(pile, planes):
    planes = np.ascontiguousarray(planes, dtype=np.uint32)
    pile.L.ga_emul_sites_poke.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    assert pile.L.ga_emul_sites_poke(pile.h, ptr(planes), planes.size) == 0


def _rc(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def test_records_through_the_host_code(lib, T):
    rng = np.random.default_rng(7)
    seqs = ["".join(rng.choice(list("ACGT"), size=n)) for n in (5, 1, 70, 1, T + 9)]
    nodes = [(k + 1, s) for k, s in enumerate(seqs)]
    edges = [(k + 1, False, k + 2, False) for k in range(len(seqs) - 1)]
    gg = binding.Graph(nodes, edges, lib_path=SITES_SO)
    ids = [0] + [i for k in range(len(seqs)) for i in (2 * (k + 1), 2 * (k + 1) + 1)] + [0]
    lens = [1] + [len(s) for s in seqs for _ in (0, 1)] + [1]
    node_start, twin, forward = sm.tables_of_graph(ids, lens)
    text = "-" + "".join(s + _rc(s) for s in seqs) + "-"
    for kind in ("bases", "depth"):
        pile = gg.pileup(kind)
        planes = _random_planes(rng, pile.planes, pile.entries)
        _poke(pile, planes)
        assert np.array_equal(pile.counts(), planes)
        for fold in (True, False):
            for q in QUERIES:
                want_e, want_F = sm.sites(planes, kind, fold=fold, node_start=node_start, twin=twin, forward=forward, **q)
                got = pile.sites(fold=fold, **q)
                assert got.total == len(want_e) and got.entries_scanned == pile.entries
                assert len(want_e) > 0 or (kind == "depth" and q["min_alt"] > 0)
                assert np.array_equal(got["entry"].astype(np.int64), want_e) and np.array_equal(got["counts"], want_F)
                node = np.searchsorted(node_start, want_e, side="right") - 1
                assert np.array_equal(got["node_id"], np.array(ids)[node] // 2) and np.array_equal(got["reverse"], np.array(ids)[node] % 2)
                assert np.array_equal(got["offset"], want_e - node_start[node])
                assert b"".join(got["graph_char"].tolist()).decode() == "".join(text[c] for c in want_e)
                if fold:
                    assert not got["reverse"].any()
        cut = pile.sites(fold=True, max_sites=3, first=2, n=pile.entries - 4)
        assert len(cut) == 3 and cut.total > 3
        assert pile.sites(fold=True).tobytes() == pile.sites(fold=True).tobytes()
    # edges: the folded query against Pileup.edge_support() of the same counters
    pile = gg.pileup("edges")
    counts = rng.integers(0, 4, size=(1, pile.entries)).astype(np.uint32)
    _poke(pile, counts)
    support = pile.edge_support()
    frm, to = gg.edge_slots()
    for t in (1, 2, 4):
        assert pile.supported_edges(t) == {k: v for k, v in support.items() if v >= t}
    assert len(pile.supported_edges(1)) > 0
    got = pile.sites(fold=False)
    assert np.array_equal(got["entry"], np.flatnonzero(counts[0])) and np.array_equal(got["from_id"], frm[got["entry"]]) and np.array_equal(got["to_id"], to[got["entry"]])


def test_refusals_of_the_host_code(lib):
    gg = binding.Graph([(1, "ACGTAC"), (2, "GGA")], [(1, False, 2, False)], lib_path=SITES_SO)
    pile = gg.pileup("bases")
    _poke(pile, np.ones((8, pile.entries), dtype=np.uint32))
    assert pile.sites().total > 0

    def refused(p, **q):
        with pytest.raises(RuntimeError, match=r"ga_pileup_sites failed.*\(100\)"):
            p.sites(**q)
    refused(pile, min_depth=0)
    refused(pile, alt_frac=(0, 0))
    refused(pile, alt_frac=(1, 65536))
    assert pile.sites(alt_frac=(65535, 65535)).total >= 0
    refused(pile, alt_frac=(3, 2))
    refused(pile, first=pile.entries + 1, n=0)
    refused(pile, first=pile.entries - 1, n=2)
    refused(pile, first=0, n=pile.entries + 1)
    assert pile.sites(first=pile.entries, n=0).total == 0
    q = binding.GaSiteParams()
    q.flags, q.alt_den, q.min_depth, q.n_entries = 2, 1, 1, pile.entries
    res = C.c_void_p()
    assert pile.L.ga_pileup_sites(pile.h, C.byref(q), C.byref(res)) == 100 and not res.value          # (a flag that is none)
    # fold on a graph with an overlap: unfolded answers, fold is refused
    ov = binding.Graph(gfa="S\t1\tACGTACGT\nS\t2\tACGTTTGA\nL\t1\t+\t2\t+\t4M\n", lib_path=SITES_SO)
    for kind in ("bases", "depth"):
        p = ov.pileup(kind)
        _poke(p, np.ones((p.planes, p.entries), dtype=np.uint32))
        assert p.sites(fold=False).total == p.entries
        refused(p, fold=True)
    e = ov.pileup("edges")
    assert e.sites(fold=True).total == 0                      # (edge slots fold through the mirror table: no precondition)
    # a twin of another length; a twin that is not the reverse complement; a graph of one strand
    for nodes in ([(2, "ACGTA", 0), (3, "ACGT", 1)], [(2, "ACGT", 0), (3, "AAAA", 1)], [(2, "ACGT", 0), (4, "ACGT", 0)]):
        d = _digraph(nodes, [])
        p = d.pileup("depth")
        _poke(p, np.ones((1, p.entries), dtype=np.uint32))
        assert p.sites(fold=False).total == p.entries
        refused(p, fold=True)
        refused(p, fold=True)                                 # (the finding is remembered)
    ok = _digraph([(2, "ACGGA", 0), (3, "TCCGT", 1)], [])
    p = ok.pileup("depth")
    _poke(p, np.ones((1, p.entries), dtype=np.uint32))
    got = p.sites(fold=True)
    assert got["entry"].tolist() == [1, 2, 3, 4, 5] and (got["counts"][:, 0] == 2).all()


def test_back_end_without_pileups_refuses():
    """the emulated back end stays as it is: it makes no pileup, so there is none to query, and the call itself refuses (100)"""
    emul = pc.emul_lib_path()
    gg = binding.Graph([(1, "ACGTAC")], [], lib_path=emul)
    with pytest.raises(RuntimeError, match=r"\(100\)"):
        gg.pileup("bases")
    q = binding.GaSiteParams()
    q.alt_den, q.min_depth = 1, 1
    res = C.c_void_p()
    assert gg.L.ga_pileup_sites(None, C.byref(q), C.byref(res)) == 100
    assert binding.GA_SITES_FOLD == 1


# ---- the whole-batch cases of the GPU tests, from the oracle alone ---------------------------------------------------------------------
def test_gpu_cases_are_not_vacuous():
    """no device: the expected planes of every case of test_pileup_sites_gpu.py from the oracle's TraceItem lists.  Every case and kind has
    a site; every fold case has a site to which both strands contribute; the (2, 1, 1/4) query selects fewer sites than (1, 1) somewhere"""
    import site_cases as sc
    fewer = False
    for name in sc.NAMES:
        c = sc.case(name)
        gg = c.graph(pc.emul_lib_path())
        n1, n2 = sc.vacuity(c, gg, lambda kind: c.model_planes(gg, kind))
        assert n2 <= n1
        fewer = fewer or n2 < n1
        print(name, c.kinds, n1, n2)
    assert fewer
