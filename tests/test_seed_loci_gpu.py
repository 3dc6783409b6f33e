"""One seed per locus on the MI355X through the product library: ga_find_seeds_loci against the model of tests/seed_loci_model.py
(exact equality of every field) on the cases of tests/test_seed_loci.py, one call with more reads than wave slots, and the usability
of the grouped seeds at scale.  Everything read here lies inside the repository."""
import numpy as np
import pytest

from graphaligner_amd import binding, synth
import seed_common as sc
import seed_loci_common as slc
import seed_model
import seed_walk_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu test needs a GPU")


def test_loci_equal_the_model_gpu():
    g = synth.bubble_graph(30000, node_len=32, seed=3)
    G = binding.Graph(g.nodes, g.edges)
    G.build_seed_index()
    model = seed_model.Model(g.nodes)
    reads = sc.spiked_reads(g)
    by_len = {len(r): i for i, r in enumerate(reads)}
    before = G.find_seeds(reads)
    for params in slc.PARAM_SETS:
        res = slc.check_reads(G, model, reads, **params)
        for n in (150, 385, 10, 0):
            assert res.seeds[by_len[n]] == [] and res.n_loci[by_len[n]] == 0
        if "max_hits" in params:
            assert any(res.truncated) and max(res.n_hits) == 16
        if not params:
            assert sum(1 for r, s in zip(reads, res.seeds) if len(r) >= 1000 and s) >= 12
    # determinism: twice, and with the reads in reversed order
    a, b, c = G.find_seeds(reads, loci=True), G.find_seeds(reads, loci=True), G.find_seeds(reads[::-1], loci=True)
    assert slc.plain(a) == slc.plain(b)
    assert slc.plain(a) == tuple(x[::-1] for x in slc.plain(c))
    # ga_find_seeds gives what it gave before the grouped calls
    after = sc.check_reads(G, model, reads)
    assert (before.seeds, before.support, before.n_hits, before.truncated) == (after.seeds, after.support, after.n_hits, after.truncated)
    assert after.n_loci is None


def test_loci_on_the_walk_index_gpu():
    g = synth.bubble_graph(30000, node_len=8, seed=3)
    G = binding.Graph(g.nodes, g.edges)
    G.build_seed_index(max_walks=64)
    reads = sc.spiked_reads(g)
    res = slc.check_reads(G, seed_walk_model.WalkModel(g.nodes, g.edges), reads)
    assert sum(1 for r, s in zip(reads, res.seeds) if len(r) >= 1000 and s) >= 12
    cyc = synth.cyclic_graph(3000, node_len=16)
    Cy = binding.Graph(cyc.nodes, cyc.edges)
    Cy.build_seed_index(max_walks=64)
    res = slc.check_reads(Cy, seed_walk_model.WalkModel(cyc.nodes, cyc.edges), synth.walk_reads(cyc, 6, 1200, seed=3)[0], max_seeds=4)
    assert any(res.seeds)


def test_zigzag_gap_and_repeat_gpu():
    nodes, reads, params, inside = slc.zigzag_case()
    G = binding.Graph(nodes, [])
    G.build_seed_index(k=params["k"], sample_shift=params["sample_shift"])
    slc.check_zigzag(slc.check_reads(G, seed_model.Model(nodes, params["k"], params["sample_shift"]), reads, **params), reads, inside)
    g, reads = slc.gap_case()
    G = binding.Graph(g.nodes, g.edges)
    G.build_seed_index()
    slc.check_gap(slc.check_reads(G, seed_model.Model(g.nodes), reads))
    g, reads = slc.repeat_case()
    G = binding.Graph(g.nodes, g.edges)
    G.build_seed_index()
    slc.check_repeat(slc.check_reads(G, seed_model.Model(g.nodes), reads, max_seeds=2))


def test_a_long_read_gets_one_seed_gpu():
    g = synth.bubble_graph(60000, node_len=32, seed=3)
    reads = synth.simulate_reads(g, 40, 5000, seed=5)[0]
    G = binding.Graph(g.nodes, g.edges)
    G.build_seed_index()
    old = G.find_seeds(reads)
    new = slc.check_reads(G, seed_model.Model(g.nodes), reads)
    n = len(reads)
    assert sum(1 for s in old.seeds if len(s) == 2) >= n / 4
    assert sum(1 for s in new.seeds if len(s) == 2) <= max(1, n // 100)
    for i in range(n):
        assert bool(new.seeds[i]) == bool(old.seeds[i]) and new.seeds[i][:1] == old.seeds[i][:1]


def test_twenty_thousand_reads_in_one_call_loci():
    """more reads than wave slots, so that a slot's per-hit buffers serve many reads; lengths mixed so that the longest-first hand-out
    reorders them; a sample of 500 against the model"""
    g = synth.linear_graph(300_000)
    reads = []
    for n, length, sd in ((5000, 500, 1), (5000, 900, 2), (5000, 1500, 3), (5000, 2500, 4)):
        reads += synth.simulate_reads(g, n, length, seed=sd)[0]
    order = np.random.default_rng(7).permutation(len(reads))
    reads = [reads[i] for i in order]
    G = binding.Graph(g.nodes, g.edges)
    G.build_seed_index()
    sample = sorted(np.random.default_rng(8).choice(len(reads), 500, replace=False).tolist())
    res = slc.check_reads(G, seed_model.Model(g.nodes), reads, which=sample)
    assert len(res.seeds) == 20000 and sum(1 for s in res.seeds if s) >= 18000


def test_grouped_seeds_are_usable_gpu():
    """2 000 reads x 5 kb on bubble_graph(2000000, node_len=32) aligned from the grouped seeds against the same reads aligned from their
    true seeds (product library for both), judged against the truth by the reference's 0.7 rule; every read counts in both runs.
    Required: good matches from grouped seeds >= good matches from true seeds - one read per hundred, and fewer seeds in total with
    `loci` than without.  The figures go to profiles/seed_loci_accuracy_gpu.json."""
    g = synth.bubble_graph(2_000_000, node_len=32)
    truth = []
    reads, seeds = synth.simulate_reads(g, 2000, 5000, seed=5, truth=truth)
    row = slc.accuracy(g, reads, seeds, truth, None, None)
    print("grouped seed accuracy (MI355X):", row)
    sc.record("seed_loci_accuracy_gpu.json", "bubble_graph(2000000, node_len=32), 2000 x 5000 bp, seed=5", row)
    assert row["good_own_seeds"] >= row["good_true_seeds"] - row["allowance"], row
    assert row["good_true_seeds"] >= 1900, row
    assert row["seeds"] < row["seeds_ungrouped"], row
