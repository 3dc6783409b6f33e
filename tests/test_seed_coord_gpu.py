"""The topology coordinate on the MI355X through the product library: ga_graph_set_seed_coordinate against the model of
tests/seed_coord_model.py, node for node, on a chain of a quarter of a million nodes per strand (open, and closed into a circle), on
the six-tree pangenome graph and the small cycle and self-loop cases of tests/test_seed_coord.py; seeds under the new coordinate
against the seed model; determinism; the usability of the seeds at scale.  Everything read here lies inside the repository."""
import numpy as np
import pytest

from graphaligner_amd import binding, synth
import seed_common as sc
import seed_coord_common as scc
import seed_coord_model as scm
import seed_loci_common as slc
import seed_model
import seed_walk_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu test needs a GPU")


@pytest.fixture(scope="module")
def long_chain():
    g = synth.linear_graph(2_000_000, node_len=8)
    g.nodes = scc.shuffled(g.nodes)
    return g


def gfa_graph(g, edges):
    """(the graph goes in as GFA text: a quarter of a million nodes one call each would take longer than the test)"""
    kept = g.edges
    g.edges = edges
    try:
        return binding.Graph(gfa=g.gfa())
    finally:
        g.edges = kept


@pytest.mark.parametrize("circle", [False, True], ids=["open", "circle"])
def test_long_chain_gpu(long_chain, circle):
    """about 500 000 digraph nodes in two chains of about 250 000: 18 doubling rounds over some 2 000 blocks, node indices shuffled.
    Closed into a circle both passes run to their bound and each strand's cycle is cut at its smallest index."""
    g = long_chain
    edges = scc.closed(g) if circle else g.edges
    G = gfa_graph(g, edges)
    lin, stats = scc.check_coordinate(G, g.nodes, edges, k=15)
    n = len(g.nodes)
    assert stats["trees"] == 2 and stats["cycles_cut"] == (2 if circle else 0)
    assert stats["cycle_rounds"] >= 18 and stats["depth_rounds"] >= 18
    assert stats["extent_sum"] == 2 * 2_000_000
    again = G.set_seed_coordinate("topology")
    assert (G.seed_coordinate() == lin).all() and {k: again[k] for k in scc.STAT_KEYS} == stats
    print("coordinate of %d nodes: %.2f ms, %d + %d rounds" % (2 * n + 2, again["build_ms"], again["cycle_rounds"], again["depth_rounds"]))


def test_trees_cycles_and_self_loops_gpu():
    p = synth.pangenome_graph(60000, chromosomes=3, node_len=32)
    for order in (p.nodes, scc.shuffled(p.nodes)):
        G = binding.Graph(order, p.edges)
        lin, stats = scc.check_coordinate(G, order, p.edges, k=15)
        assert stats["trees"] == 6 and stats["cycles_cut"] == 0
    for n, tail in ((2, 0), (3, 1), (64, 70), (100, 0)):
        nodes, edges = scc.cycle(n, tail, seed=n + tail)
        for order in (nodes, scc.shuffled(nodes, n + tail), nodes[n // 2:] + nodes[:n // 2]):
            lin, stats = scc.check_coordinate(binding.Graph(order, edges), order, edges)
            assert stats["cycles_cut"] == 2 and stats["trees"] == (3 if tail else 2)
    # tail indices below the cycle's
    nodes, edges = scc.cycle(5, 7, seed=3)
    order = nodes[5:] + nodes[:5]
    lin, stats = scc.check_coordinate(binding.Graph(order, edges), order, edges)
    assert stats["cycles_cut"] == 2 and stats["trees"] == 3
    # self-loops: [self, prev] and [self]; in-degree 5 with the self-loop first
    nodes = [(1, scc.dna(20, 1)), (2, scc.dna(30, 2)), (3, scc.dna(25, 3))]
    edges = [(2, False, 2, False), (1, False, 2, False), (3, False, 3, False)]
    lin, stats = scc.check_coordinate(binding.Graph(nodes, edges), nodes, edges)
    assert stats["trees"] == 4 and lin[3] == lin[1] + 20
    nodes = [(i, scc.dna(10 + i, i)) for i in range(1, 8)]
    edges = [(6, False, 6, False)] + [(i, False, 6, False) for i in (3, 1, 2, 4, 5)] + [(6, False, 7, False)]
    lin, stats = scc.check_coordinate(binding.Graph(nodes, edges), nodes, edges)
    assert lin[11] == lin[5] + 13
    # the bubble graph closed into a circle, and a graph with cycles that the parent relation does not follow
    g = synth.bubble_graph(40000, node_len=32)
    for order in (g.nodes, scc.shuffled(g.nodes)):
        lin, stats = scc.check_coordinate(binding.Graph(order, scc.closed(g)), order, scc.closed(g), k=15)
        assert stats["cycles_cut"] == 2
    c = synth.cyclic_graph(3000, node_len=16)
    order = scc.shuffled(c.nodes)
    scc.check_coordinate(binding.Graph(order, c.edges), order, c.edges, k=15)


def test_seeds_equal_the_model_gpu():
    """shuffled bubble_graph(30000, node_len=8) with the walk index: ga_find_seeds and ga_find_seeds_loci under the topology coordinate
    against the model, read for read; kind 0 afterwards gives the seeds from before"""
    g = synth.bubble_graph(30000, node_len=8, seed=3)
    nodes = scc.shuffled(g.nodes)
    G = binding.Graph(nodes, g.edges)
    G.build_seed_index(max_walks=64)
    reads = sc.spiked_reads(g)
    before = G.find_seeds(reads)
    file_lin = G.seed_coordinate()
    G.set_seed_coordinate("topology")
    model, lin, stats = scm.with_topology(seed_walk_model.WalkModel(nodes, g.edges), nodes, g.edges)
    assert (G.seed_coordinate() == np.array(lin)).all()
    res = sc.check_reads(G, model, reads)
    grouped = slc.check_reads(G, model, reads)
    assert sum(1 for r, s in zip(reads, res.seeds) if len(r) >= 1000 and s) >= 12
    assert sum(1 for r, s in zip(reads, grouped.seeds) if len(r) >= 1000 and s) >= 12
    # determinism: the coordinate twice, the seeds twice
    a = G.seed_coordinate()
    G.set_seed_coordinate("topology")
    assert (a == G.seed_coordinate()).all()
    assert slc.plain(grouped) == slc.plain(G.find_seeds(reads, loci=True))
    # file order again: the array and the seeds from before the call
    G.set_seed_coordinate("file")
    assert (G.seed_coordinate() == file_lin).all()
    after = G.find_seeds(reads)
    assert (before.seeds, before.support, before.n_hits, before.truncated) == (after.seeds, after.support, after.n_hits, after.truncated)
    G.build_seed_index(max_walks=64, coordinate="topology")
    G.build_seed_index()
    assert G.seed_coord_stats()["kind"] == 0


def test_support_on_a_shuffled_graph_gpu():
    """the table of DESIGN.md section 10b on the device: the 20 reads on shuffled bubble_graph(40000, node_len=32)"""
    g = synth.bubble_graph(40000, node_len=32)
    nodes = scc.shuffled(g.nodes)
    reads = synth.simulate_reads(g, 20, 3000, seed=5)[0]
    G = binding.Graph(nodes, g.edges)
    G.build_seed_index()
    old = G.find_seeds(reads)
    G.set_seed_coordinate("topology")
    new = sc.check_reads(G, scm.with_topology(seed_model.Model(nodes), nodes, g.edges)[0], reads)
    P = binding.Graph(g.nodes, g.edges)
    P.build_seed_index(coordinate="topology")
    assert scc.first_seeds(new) == scc.first_seeds(P.find_seeds(reads))
    assert scc.mean_first_support(old) < 0.5 * scc.mean_first_support(new)


def test_seeds_under_topology_are_usable_gpu():
    """2 000 reads x 5 kb on bubble_graph(2000000, node_len=32) with its node list shuffled, aligned from the grouped seeds found under
    the topology coordinate against the same reads aligned from their true seeds (product library for both), judged against the truth by
    the reference's 0.7 rule; every read counts in both runs.  Required: good matches from own seeds >= good matches from true seeds -
    one read per hundred.  File order on the same shuffled graph is recorded beside it.  The figures go to
    profiles/seed_coord_accuracy_gpu.json."""
    g = synth.bubble_graph(2_000_000, node_len=32)
    nodes = scc.shuffled(g.nodes)
    truth = []
    reads, seeds = synth.simulate_reads(g, 2000, 5000, seed=5, truth=truth)
    rows = {}
    for coordinate in ("topology", "file"):
        row = scc.accuracy(nodes, g.edges, reads, seeds, truth, None, None, coordinate, loci=True, good_true=rows["topology"]["good_true_seeds"] if rows else None)
        print("seed accuracy on the shuffled graph (MI355X):", row)
        sc.record("seed_coord_accuracy_gpu.json", "shuffled bubble_graph(2000000, node_len=32), 2000 x 5000 bp, seed=5, %s" % coordinate, row)
        rows[coordinate] = row
    row = rows["topology"]
    assert row["good_own_seeds"] >= row["good_true_seeds"] - row["allowance"], row
    assert row["good_true_seeds"] >= 1900, row
