"""ga_graph_set_seed_coordinate (the topology coordinate of the seeding rule) against the model of tests/seed_coord_model.py: every
node's lin and the statistics on chains, cycles, self-loops, in-list orders, an inversion, a node of length 0, a node of in-degree 5
and the larger synthetic graphs in path order and shuffled; the edge rule, independence of the node order and determinism; seeds
under the new coordinate against the seed models; what the feature is for (support on a shuffled graph); the interface; the driver's
--seed-coord.  CPU: the seeding program and the alignment programs built for the host (tests/emul)."""
import io
import os
import sys

import numpy as np
import pytest

from graphaligner_amd import aligner, binding, compare, synth
import parity_common as pc
import seed_common as sc
import seed_coord_common as scc
import seed_coord_model as scm
import seed_loci_common as slc
import seed_model
import seed_walk_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return pc.emul_lib_path()


def run_case(lib, nodes, edges, **index):
    G = binding.Graph(nodes, edges, lib_path=lib)
    return scc.check_coordinate(G, nodes, edges, **index)


# ---- equality with the model: the smallest shapes at which a phase can go wrong ---------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 257, 1025])
def test_chains(lib, n):
    """doubling rounds 0 to 11 and the edge of a 256-lane block; node indices permuted"""
    nodes, edges = scc.chain(n, seed=n)
    for order in (nodes, scc.shuffled(nodes, n), nodes[::-1]):
        lin, stats = run_case(lib, order, edges)
        assert stats["trees"] == 2 and stats["cycles_cut"] == 0
        assert stats["extent_sum"] == 2 * sum(len(s) for _, s in nodes)
        assert stats["cycle_rounds"] == scm.ceil_log2(n) and stats["depth_rounds"] == (0 if n == 1 else scm.ceil_log2(n - 1) + 1)


@pytest.mark.parametrize("n,tail", [(2, 0), (3, 0), (3, 1), (64, 0), (64, 1), (64, 70), (100, 0), (100, 70)])
def test_cycles(lib, n, tail):
    """one cycle per strand, cut at its smallest node index; on the forward strand the tail leads into the cycle, on the reverse strand
    it hangs off it"""
    nodes, edges = scc.cycle(n, tail, seed=n + tail)
    for order in (nodes, scc.shuffled(nodes, n + tail), nodes[n // 2:] + nodes[:n // 2]):       # (the last: the smallest index mid-cycle)
        lin, stats = run_case(lib, order, edges)
        assert stats["cycles_cut"] == 2 and stats["cycle_rounds"] == scm.ceil_log2(2 * len(nodes) + 2)
        # forward strand: the tail's first node is a root of its own and the cycle's cut node another; reverse strand: one tree
        assert stats["trees"] == (3 if tail else 2)


def test_tail_indices_below_the_cycle(lib):
    """the tail's nodes come first in the file, so each of them is the smallest index on its own walk: a cut made without the marks
    would cut there"""
    nodes, edges = scc.cycle(5, 7, seed=3)
    order = nodes[5:] + nodes[:5]
    lin, stats = run_case(lib, order, edges)
    assert stats["cycles_cut"] == 2 and stats["trees"] == 3
    index_of = {nid: 1 + 2 * i for i, (nid, _) in enumerate(order)}
    tail_ids = [nid for nid, _ in nodes[5:]]
    assert max(index_of[t] for t in tail_ids) < min(index_of[c] for c, _ in nodes[:5])
    # the forward tail is one chain from its own root: consecutive nodes differ by the length of the one before
    seq = dict(nodes)
    for a, b in zip(tail_ids, tail_ids[1:]):
        assert lin[index_of[b]] == lin[index_of[a]] + len(seq[a])


def test_two_cycles_and_an_acyclic_component(lib):
    a_nodes, a_edges = scc.cycle(6, 2, first_id=1, seed=1)
    b_nodes, b_edges = scc.cycle(9, 0, first_id=20, seed=2)
    c_nodes, c_edges = scc.chain(5, seed=9)
    c_nodes = [(nid + 40, s) for nid, s in c_nodes]
    c_edges = [(f + 40, fs, t + 40, te) for f, fs, t, te in c_edges]
    nodes, edges = a_nodes + b_nodes + c_nodes, a_edges + b_edges + c_edges
    for order in (nodes, scc.shuffled(nodes, 4)):
        lin, stats = run_case(lib, order, edges)
        assert stats["cycles_cut"] == 4 and stats["trees"] == 7


def test_self_loops(lib):
    """in-list [self, prev]: prev is the parent; in-list [self]: a root"""
    nodes = [(1, scc.dna(20, 1)), (2, scc.dna(30, 2)), (3, scc.dna(25, 3))]
    edges = [(2, False, 2, False), (1, False, 2, False), (3, False, 3, False)]
    lin, stats = run_case(lib, nodes, edges)
    n_nodes, lens, ins = scm.in_lists_of(nodes, edges)
    assert ins[3] == [3, 1] and ins[5] == [5] and ins[2] == [4] and ins[4] == [4]
    assert stats["cycles_cut"] == 0 and stats["trees"] == 4                     # 1 -> 2, 2' -> 1', 3, 3'
    assert lin[3] == lin[1] + 20 and lin[2] == lin[4] + 30


def test_in_list_order_decides(lib):
    """a node with two in-neighbours of different length, its finished in-list handed over in both orders: two coordinates"""
    nodes = [(1, scc.dna(10, 1)), (2, scc.dna(33, 2)), (3, scc.dna(12, 3)), (4, scc.dna(15, 4))]
    edges = [(1, False, 2, False), (1, False, 3, False), (2, False, 4, False), (3, False, 4, False)]
    got = []
    for in_list in ([4, 6], [6, 4]):
        given = {8: in_list}
        G = scc.graph_with_lists(lib, nodes, edges, given, {8: []})
        lin, stats = scc.check_coordinate(G, nodes, edges, given=given)
        got.append(int(lin[7] - lin[1]))
    assert got == [10 + 33, 10 + 12]


def test_inversion_zero_length_and_in_degree_five(lib):
    # an inversion edge: 1+ -> 2-, so the tree of 1+ holds nodes of both strand flags
    nodes = [(1, scc.dna(20, 1)), (2, scc.dna(30, 2)), (3, scc.dna(7, 3))]
    edges = [(1, False, 2, True), (2, False, 3, False)]
    lin, stats = run_case(lib, nodes, edges)
    assert lin[4] == lin[1] + 20 and lin[2] == lin[3] + 30
    # a node of length 0 in the middle of a chain
    nodes = [(1, scc.dna(20, 1)), (2, ""), (3, scc.dna(9, 3))]
    edges = [(1, False, 2, False), (2, False, 3, False)]
    lin, stats = run_case(lib, nodes, edges)
    assert lin[3] == lin[5] == lin[1] + 20
    # in-degree 5: the in-list itself is read, not the four entries of the node's record; the first entry is a self-loop
    nodes = [(i, scc.dna(10 + i, i)) for i in range(1, 8)]
    edges = [(6, False, 6, False)] + [(i, False, 6, False) for i in (3, 1, 2, 4, 5)] + [(6, False, 7, False)]
    for order in (nodes, scc.shuffled(nodes, 2)):
        lin, stats = run_case(lib, order, edges)
        index_of = {nid: 1 + 2 * i for i, (nid, _) in enumerate(order)}
        assert lin[index_of[6]] == lin[index_of[3]] + 13
    # in-degree 4 with the self-loop first: the four entries of the node's record decide
    edges4 = [(6, False, 6, False)] + [(i, False, 6, False) for i in (3, 1, 2)]
    lin, stats = run_case(lib, nodes, edges4)
    assert lin[11] == lin[5] + 13


# ---- larger synthetic graphs, in path order and shuffled ---------------------------------------------------------------------------
def big_cases():
    g = synth.bubble_graph(40000, node_len=32)
    yield "bubbles32", g.nodes, g.edges, dict(k=15)
    g8 = synth.bubble_graph(40000, node_len=8)
    yield "bubbles8-walks", g8.nodes, g8.edges, dict(k=15, max_walks=64)
    c = synth.cyclic_graph(3000, node_len=16)
    yield "cyclic", c.nodes, c.edges, dict(k=15)
    yield "circle", g.nodes, scc.closed(g), dict(k=15)
    p = synth.pangenome_graph(60000, chromosomes=3, node_len=32)
    yield "pangenome", p.nodes, p.edges, dict(k=15)


@pytest.mark.parametrize("name", ["bubbles32", "bubbles8-walks", "cyclic", "circle", "pangenome"])
def test_larger_graphs(lib, name):
    nodes, edges, index = [(n, e, i) for c, n, e, i in big_cases() if c == name][0]
    rel = []
    for order in (nodes, scc.shuffled(nodes)):
        lin, stats = run_case(lib, order, edges, **index)
        if name == "pangenome":
            # six trees, their bases in the order of their roots' node indices
            assert stats["trees"] == 6 and stats["cycles_cut"] == 0
            _, _, parent, lens = scm.of_graph(order, edges)
            roots = [v for v in range(1, len(parent) - 1) if parent[v] is None]
            assert len(roots) == 6 and all(lin[a] < lin[b] for a, b in zip(roots, roots[1:]))
        if name == "circle":
            assert stats["cycles_cut"] == 2
        if name == "cyclic":
            # (its back edges and self-loops come last in the in-lists: cycles of the graph, none of the parent relation)
            assert stats["cycles_cut"] == 0
        # node-order independence: lin(v) - lin(root(v)) by node id does not depend on the order of the node list, unless a cycle is
        # cut (the cut follows the smallest index)
        _, _, parent, _ = scm.of_graph(order, edges)
        index_of = {}
        for i, (nid, _) in enumerate(order):
            index_of[2 * nid], index_of[2 * nid + 1] = 1 + 2 * i, 2 + 2 * i
        rel.append({d: int(lin[v] - lin[scc.root_of(parent, v)]) for d, v in index_of.items()})
    if name != "circle":
        assert rel[0] == rel[1]


def test_determinism_and_file_order_restored(lib):
    g = synth.cyclic_graph(3000, node_len=16)
    nodes = scc.shuffled(g.nodes)
    G = binding.Graph(nodes, g.edges, lib_path=lib)
    G.build_seed_index()
    file_lin = G.seed_coordinate()
    model = seed_model.Model(nodes)
    assert file_lin[1:-1].tolist() == [model.lin[i] for i in range(1, len(file_lin) - 1)] and file_lin[0] == 0 and file_lin[-1] == 0
    assert G.seed_coord_stats() == dict(kind=0, trees=0, cycles_cut=0, cycle_rounds=0, depth_rounds=0, extent_sum=0, build_ms=0.0)
    G.set_seed_coordinate("topology")
    a = G.seed_coordinate()
    st = G.set_seed_coordinate(1)
    b = G.seed_coordinate()
    assert (a == b).all() and st["kind"] == 1 and not (a == file_lin).all()
    assert G.set_seed_coordinate("file")["kind"] == 0
    assert (G.seed_coordinate() == file_lin).all()


# ---- seeds under the new coordinate -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world(lib):
    """the graph of the issue's table: bubble_graph(40000, node_len=32), its node list shuffled, and the 20 reads"""
    g = synth.bubble_graph(40000, node_len=32)
    nodes = scc.shuffled(g.nodes)
    reads = synth.simulate_reads(g, 20, 3000, seed=5)[0]
    G = binding.Graph(nodes, g.edges, lib_path=lib)
    G.build_seed_index()
    P = binding.Graph(g.nodes, g.edges, lib_path=lib)
    P.build_seed_index(coordinate="topology")
    return g, nodes, reads, G, P


def test_seeds_equal_the_model_on_the_shuffled_graph(world):
    g, nodes, reads, G, P = world
    G.set_seed_coordinate("topology")
    model, lin, _ = scm.with_topology(seed_model.Model(nodes), nodes, g.edges)
    assert (G.seed_coordinate() == np.array(lin)).all()
    both = sc.spiked_reads(g) + reads
    res = sc.check_reads(G, model, both)
    grouped = slc.check_reads(G, model, both)
    assert sum(1 for r, s in zip(both, res.seeds) if len(r) >= 1000 and s) >= 30
    assert sum(1 for r, s in zip(both, grouped.seeds) if len(r) >= 1000 and s) >= 30


def test_first_seed_does_not_depend_on_the_node_order(world):
    """the 20 reads: first seed (node id, position, strand) and its support on the shuffled graph equal those on the graph in path
    order, both under the topology coordinate"""
    g, nodes, reads, G, P = world
    G.set_seed_coordinate("topology")
    for loci in (False, True):
        a, b = G.find_seeds(reads, loci=loci), P.find_seeds(reads, loci=loci)
        assert all(s for s in a.seeds)
        assert scc.first_seeds(a) == scc.first_seeds(b)


def test_file_order_on_a_shuffled_graph_is_what_this_is_for(world):
    """the motivating condition: on the shuffled graph the mean support of the first seed under file order is below half of that
    under topology (8.3 against 99.0 when this was written), and under file order every read pays a second seed"""
    g, nodes, reads, G, P = world
    G.set_seed_coordinate("file")
    old = G.find_seeds(reads)
    G.set_seed_coordinate("topology")
    new = G.find_seeds(reads)
    print("mean support of the first seed: file order %.1f, topology %.1f; reads with two seeds: %d and %d of %d" % (
        scc.mean_first_support(old), scc.mean_first_support(new), sum(1 for s in old.seeds if len(s) > 1), sum(1 for s in new.seeds if len(s) > 1), len(reads)))
    assert all(s for s in new.seeds)
    assert scc.mean_first_support(old) < 0.5 * scc.mean_first_support(new)


def test_seeds_on_the_walk_index_under_topology(lib):
    g = synth.bubble_graph(30000, node_len=8, seed=3)
    nodes = scc.shuffled(g.nodes)
    G = binding.Graph(nodes, g.edges, lib_path=lib)
    G.build_seed_index(max_walks=64, coordinate="topology")
    model, _, _ = scm.with_topology(seed_walk_model.WalkModel(nodes, g.edges), nodes, g.edges)
    reads = synth.simulate_reads(g, 6, 3000, seed=5)[0]
    res = slc.check_reads(G, model, reads)
    assert all(res.seeds)


# ---- interface --------------------------------------------------------------------------------------------------------------------------
def test_invalid_calls_and_rebuild(lib):
    g = synth.bubble_graph(6000, node_len=32, seed=3)
    reads = synth.simulate_reads(g, 3, 1000, seed=5)[0]
    G = binding.Graph(g.nodes, g.edges, lib_path=lib)
    L = G.L
    assert L.ga_graph_set_seed_coordinate(G.h, 1) == 100 and L.ga_graph_set_seed_coordinate(G.h, 0) == 100        # no index yet
    assert L.ga_graph_set_seed_coordinate(None, 1) == 100
    st = binding.GaSeedCoordStats()
    import ctypes as C
    assert L.ga_graph_seed_coord_stats(G.h, C.byref(st)) == 100 and L.ga_graph_seed_coordinate_copy(G.h, None, 0) == 100
    G.build_seed_index()
    for kind in (2, -1, 7):
        assert L.ga_graph_set_seed_coordinate(G.h, kind) == 100
    assert L.ga_graph_seed_coord_stats(G.h, None) == 100 and L.ga_graph_seed_coordinate_copy(G.h, None, 4) == 100
    with pytest.raises(ValueError):
        G.build_seed_index(coordinate="path")
    before = G.find_seeds(reads)
    grouped_before = G.find_seeds(reads, loci=True)
    file_lin = G.seed_coordinate()
    assert G.set_seed_coordinate("topology")["kind"] == 1
    G.find_seeds(reads, loci=True)
    assert G.set_seed_coordinate("file")["kind"] == 0
    after = G.find_seeds(reads)
    assert (before.seeds, before.support, before.n_hits, before.truncated) == (after.seeds, after.support, after.n_hits, after.truncated)
    assert slc.plain(grouped_before) == slc.plain(G.find_seeds(reads, loci=True))
    # a rebuilt index is in file order again, with either build
    G.set_seed_coordinate("topology")
    for walks in (0, 8):
        G.build_seed_index(max_walks=walks)
        assert G.seed_coord_stats()["kind"] == 0 and (G.seed_coordinate() == file_lin).all()
        G.set_seed_coordinate("topology")
    # a short copy
    lin = np.full(5, -7, dtype=np.int64)
    assert L.ga_graph_seed_coordinate_copy(G.h, lin.ctypes.data_as(C.c_void_p), 3) == 0
    assert lin[3] == -7 and (lin[:3] == G.seed_coordinate()[:3]).all()


def test_the_older_host_builds_refuse_topology():
    """back ends without the topology pass (the profiles emul_seed, emul_seed_walks and emul_seed_loci of parity_common.PROFILES):
    GA_E_INVALID through the back end's default; file order is what they have, and asking for it is accepted"""
    g = synth.bubble_graph(6000, node_len=32, seed=3)
    reads = synth.simulate_reads(g, 2, 1000, seed=5)[0]
    for profile in ("emul_seed", "emul_seed_walks", "emul_seed_loci"):
        with pc.emul_profile(profile):
            G = binding.Graph(g.nodes, g.edges, lib_path=pc.emul_lib_path())
        assert G.L.ga_graph_set_seed_coordinate(G.h, 0) == 100                 # no index yet
        G.build_seed_index()
        before = G.find_seeds(reads)
        with pytest.raises(RuntimeError, match=r"ga_graph_set_seed_coordinate failed: .*\(100\)"):
            G.set_seed_coordinate("topology")
        with pytest.raises(RuntimeError, match=r"ga_graph_set_seed_coordinate failed: .*\(100\)"):
            G.build_seed_index(coordinate="topology")
        assert G.set_seed_coordinate("file")["kind"] == 0
        after = G.find_seeds(reads)
        assert any(after.seeds) and (before.seeds, before.support) == (after.seeds, after.support)


# ---- usability ----------------------------------------------------------------------------------------------------------------------------
def test_seeds_under_topology_are_usable(lib):
    """the harness of test_find_seeds.py::test_seeds_are_usable on the shuffled graph with the topology coordinate: good matches from
    own seeds >= good matches from true seeds - one read per hundred.  The figures go to profiles/seed_coord_accuracy_cpu.json."""
    g = synth.bubble_graph(40000, node_len=32)
    nodes = scc.shuffled(g.nodes)
    truth = []
    reads, seeds = synth.simulate_reads(g, 100, 3000, seed=5, truth=truth)
    row = scc.accuracy(nodes, g.edges, reads, seeds, truth, pc.emul_lib_path(), lib, "topology")
    row.pop("seed_kernel_ms")
    row.pop("coord_build_ms")
    print("seed accuracy on the shuffled graph (host emulation):", row)
    sc.record("seed_coord_accuracy_cpu.json", "shuffled bubble_graph(40000, node_len=32), 100 x 3000 bp, seed=5, topology", row)
    assert row["good_own_seeds"] >= row["good_true_seeds"] - row["allowance"], row
    assert row["good_true_seeds"] >= 90, row


# ---- driver -------------------------------------------------------------------------------------------------------------------------------
def test_driver_seed_coord(tmp_path, lib, monkeypatch):
    """--find-seeds --seed-coord topology on a GFA file whose S lines are shuffled: the GAM's alignments pass the 0.7 rule against
    the truth; --seed-coord without --find-seeds and an unknown kind are refused"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_aligner_driver import _decode_gam
    g = synth.bubble_graph(30000, node_len=32, seed=21)
    truth = []
    reads, _ = synth.simulate_reads(g, 6, 1200, seed=77, mid_seed=True, truth=truth)
    names = ["r%d" % i for i in range(len(reads))]
    path_order = list(g.nodes)
    g.nodes = scc.shuffled(g.nodes)
    (tmp_path / "g.gfa").write_text(g.gfa())
    g.nodes = path_order
    with open(tmp_path / "reads.fastq", "w") as f:
        for n, r in zip(names, reads):
            f.write("@%s\n%s\n+\n%s\n" % (n, r, "I" * len(r)))
    base = ["-g", str(tmp_path / "g.gfa"), "-f", str(tmp_path / "reads.fastq"), "-a", str(tmp_path / "out.gam"), "-t", "1", "-b", "35"]
    for bad in (["-s", "x.gam", "--seed-coord", "topology"], ["-s", "x.gam", "--seed-coord", "file"], ["--find-seeds", "--seed-coord", "path"]):
        err = io.StringIO()
        with pytest.raises(SystemExit):
            aligner.parse_args(base + bad, err=err)
        assert "--seed-coord must be file or topology and goes with --find-seeds" in err.getvalue()
    assert aligner.parse_args(base + ["--find-seeds"]).seedCoord == "file"
    assert aligner.parse_args(base + ["--find-seeds", "--seed-coord", "file"]).seedCoord == "file"
    p = aligner.parse_args(base + ["--find-seeds", "--seed-loci", "--seed-coord", "topology"])
    assert p.findSeeds and p.seedCoord == "topology"
    p.outputDir = str(tmp_path)
    out, err = io.StringIO(), io.StringIO()
    monkeypatch.setenv("GA_EMUL_WITHOUT", "seeded")            # the two-call path: prepare_seeded is refused, find_seeds and prepare follow
    written = aligner.align_reads(p, lib_path=lib, out=out, err=err)
    assert "seed coordinate: topology, 2 trees, 0 cycles cut" in out.getvalue(), out.getvalue()
    assert "seeds found for 6 of 6 reads" in out.getvalue(), out.getvalue()
    got = _decode_gam(str(tmp_path / "out.gam"))
    assert [a["name"] for a in got] == [n for n, _ in written]
    sizes = {nid: len(seq) for nid, seq in g.nodes}
    predicted = {a["name"]: [m[0] for m in a["mappings"]] for a in got}     # (the GAM carries bigraph ids)
    res = compare.compare({n: t for n, t in zip(names, truth)}, predicted, sizes)
    assert res["good"] == 6 and res["bad"] == 0, (res, out.getvalue())
