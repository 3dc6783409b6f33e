"""Seeding on the MI355X through the product library: the index and the seeds against the model of tests/seed_model.py (exact
equality), the usability of the seeds at scale, one call with more reads than wave slots, and the promise that building an index
does not disturb alignment from caller-given seeds.  Everything read here lies inside the repository."""
import numpy as np
import pytest

from graphaligner_amd import binding, synth
import seed_common as sc
import seed_model
from test_seed_index import GRAPHS, index_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu test needs a GPU")


def test_index_equals_the_model_gpu():
    for name, k, s in index_cases():
        g = GRAPHS[name]()
        sc.check_index(g.nodes, g.edges, k, s, None)
    nodes, edges = sc.big_node_graph(100000)
    for k in (11, 15, 31):
        for s in (0, 2, 5):
            sc.check_index(nodes, edges, k, s, None)


def test_seeds_equal_the_model_gpu():
    g = synth.bubble_graph(30000, node_len=32, seed=3)
    G = binding.Graph(g.nodes, g.edges)
    G.build_seed_index()
    model = seed_model.Model(g.nodes)
    reads = sc.spiked_reads(g)
    res = sc.check_reads(G, model, reads)
    assert sum(1 for r, s in zip(reads, res.seeds) if len(r) >= 1000 and s) >= 12
    for params in (dict(max_seeds=1), dict(max_seeds=3), dict(max_hits=16), dict(min_support=1, window=100, diag_tol=5), dict(max_occ=1)):
        r2 = sc.check_reads(G, model, reads, **params)
        if "max_hits" in params:
            assert any(r2.truncated) and max(r2.n_hits) == 16
    clean = [r[:386] for r in synth.simulate_reads(g, 8, 386, sub=0.0, ins=0.0, dele=0.0, seed=40)[0]]
    r3 = sc.check_reads(G, model, clean, min_support=1)
    assert any(r3.seeds)
    # determinism: twice, and with the reads in reversed order
    a, b, c = G.find_seeds(reads), G.find_seeds(reads), G.find_seeds(reads[::-1])
    assert (a.seeds, a.support, a.n_hits, a.truncated) == (b.seeds, b.support, b.n_hits, b.truncated)
    assert (a.seeds, a.support, a.n_hits, a.truncated) == (c.seeds[::-1], c.support[::-1], c.n_hits[::-1], c.truncated[::-1])
    # the poly-A case and other (k, s)
    base = synth.random_genome(3000, 8).tobytes().decode()
    nodes = [(1, base[:1500]), (2, "A" * 600), (3, base[1500:])]
    P = binding.Graph(nodes, [(1, False, 2, False), (2, False, 3, False)])
    P.build_seed_index(k=15, sample_shift=0)
    pm = seed_model.Model(nodes, 15, 0)
    pr = ["A" * 500, base[200:900] + "A" * 300 + base[1600:2200]]
    assert sc.check_reads(P, pm, pr, max_occ=1).n_hits[0] == 0
    assert sc.check_reads(P, pm, pr, max_occ=1000, max_hits=64).truncated[0]
    lin = synth.linear_graph(20000)
    for k, s in ((11, 0), (31, 3)):
        Gk = binding.Graph(lin.nodes, lin.edges)
        Gk.build_seed_index(k=k, sample_shift=s)
        sc.check_reads(Gk, seed_model.Model(lin.nodes, k, s), sc.spiked_reads(lin, seed=11))


@pytest.mark.parametrize("name", ["bubbles", "linear"])
def test_seeds_are_usable_gpu(name):
    """2 000 reads x 5 kb aligned from the seeds found here against the same reads aligned from their true seeds (product library for
    both), judged against the truth by the reference's 0.7 rule; every read counts in both runs.  Required: good matches from own seeds
    >= good matches from true seeds - one read per hundred.  The figures go to profiles/seed_accuracy_gpu.json."""
    g = synth.bubble_graph(2_000_000, node_len=32) if name == "bubbles" else synth.linear_graph(1_000_000)
    truth = []
    reads, seeds = synth.simulate_reads(g, 2000, 5000, seed=5, truth=truth)
    row = sc.accuracy(g, reads, seeds, truth, None, None)
    print("seed accuracy (MI355X, %s):" % name, row)
    label = "bubble_graph(2000000, node_len=32)" if name == "bubbles" else "linear_graph(1000000)"
    sc.record("seed_accuracy_gpu.json", label + ", 2000 x 5000 bp, seed=5", row)
    assert row["good_own_seeds"] >= row["good_true_seeds"] - row["allowance"], row
    assert row["good_true_seeds"] >= 1900, row


def test_twenty_thousand_reads_in_one_call():
    """more reads than wave slots, lengths mixed so that the longest-first hand-out reorders them; a sample of 500 against the model"""
    g = synth.linear_graph(300_000)
    reads = []
    for n, length, sd in ((5000, 500, 1), (5000, 900, 2), (5000, 1500, 3), (5000, 2500, 4)):
        reads += synth.simulate_reads(g, n, length, seed=sd)[0]
    order = np.random.default_rng(7).permutation(len(reads))
    reads = [reads[i] for i in order]
    G = binding.Graph(g.nodes, g.edges)
    G.build_seed_index()
    sample = sorted(np.random.default_rng(8).choice(len(reads), 500, replace=False).tolist())
    res = sc.check_reads(G, seed_model.Model(g.nodes), reads, which=sample)
    assert len(res.seeds) == 20000 and sum(1 for s in res.seeds if s) >= 18000


def test_index_does_not_disturb_alignment_from_given_seeds():
    g = synth.bubble_graph(200_000, node_len=32, seed=11)
    reads, seeds = synth.simulate_reads(g, 200, 3000, seed=5, mid_seed=True)
    G = binding.Graph(g.nodes, g.edges)

    def run():
        out = G.align(reads, seeds, 35, flags=binding.GA_F_TRACE)
        return [(r["status"], r["failed"], r["score"], r["alignment_start"], r["alignment_end"], r["mappings"], r["trace"].tobytes()) for r in out]
    before = run()
    G.build_seed_index()
    G.find_seeds(reads)
    after = run()
    assert before == after
    assert sum(1 for r in after if r[0] == 0 and not r[1]) >= 190
