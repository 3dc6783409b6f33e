"""The walk index (ga_graph_build_seed_index_walks: k-mers of walks across edges, for graphs of short nodes) on the MI355X through the
product library: index and statistics against the model of tests/seed_walk_model.py (exact equality), the seeds it gives against the
model, their usability at scale on graphs of 8-bp nodes, and the promise that a walk index does not disturb alignment from
caller-given seeds.  Everything read here lies inside the repository."""
import pytest

from graphaligner_amd import binding, synth
import seed_common as sc
import seed_walk_common as swc
import seed_walk_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu test needs a GPU")


def test_walk_index_equals_the_model_gpu():
    skipped = 0
    for name, k, s, max_walks in swc.walk_index_cases():
        g = swc.GRAPHS[name]()
        _, _, _, ws = swc.check_walk_index(g.nodes, g.edges, k, s, max_walks, None)
        skipped += ws["tail_starts_skipped"]
    assert skipped > 0                                                      # (the cap was met on the way)


def test_walk_seeds_equal_the_model_gpu():
    g = synth.bubble_graph(30000, node_len=8, seed=3)
    G = binding.Graph(g.nodes, g.edges)
    G.build_seed_index(max_walks=64)
    model = seed_walk_model.WalkModel(g.nodes, g.edges)
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
    # a cyclic graph and another (k, s), with the cap met
    cyc = synth.cyclic_graph(3000, node_len=16)
    C = binding.Graph(cyc.nodes, cyc.edges)
    C.build_seed_index(k=31, sample_shift=0, max_walks=4)
    assert C.seed_index_walk_stats()["tail_starts_skipped"] > 0
    sc.check_reads(C, seed_walk_model.WalkModel(cyc.nodes, cyc.edges, 31, 0, 4), synth.walk_reads(cyc, 6, 1200, seed=3)[0])


@pytest.mark.parametrize("name", ["bubbles8", "dense8"])
def test_walk_seeds_are_usable_gpu(name):
    """2 000 reads x 5 kb on graphs of 8-bp nodes, aligned from the seeds the walk index gives against the same reads aligned from
    their true seeds (product library for both), judged against the truth by the reference's 0.7 rule; every read counts in both runs.
    Required: the in-node index gives no read a seed; good matches from own seeds >= good matches from true seeds - one read per
    hundred (20); good matches from true seeds >= 1 900.  The figures go to profiles/seed_walks_accuracy_gpu.json."""
    if name == "bubbles8":
        g, label = synth.bubble_graph(2_000_000, node_len=8), "bubble_graph(2000000, node_len=8)"
    else:
        g, label = synth.SynthGraph(synth.random_genome(1_000_000, 6), node_len=8, snp_every=8, seed=2), "SynthGraph(random_genome(1000000, 6), node_len=8, snp_every=8, seed=2)"
    truth = []
    reads, seeds = synth.simulate_reads(g, 2000, 5000, seed=5, truth=truth)
    row = swc.accuracy_walks(g, reads, seeds, truth, None, None, 64)
    print("walk seed accuracy (MI355X, %s):" % name, row)
    sc.record("seed_walks_accuracy_gpu.json", label + ", 2000 x 5000 bp, seed=5, max_walks=64", row)
    assert row["reads_with_seed_in_node_index"] == 0, row
    assert row["good_own_seeds"] >= row["good_true_seeds"] - row["allowance"], row
    assert row["good_true_seeds"] >= 1900, row


def test_walk_index_does_not_disturb_alignment_from_given_seeds():
    g = synth.bubble_graph(200_000, node_len=32, seed=11)
    reads, seeds = synth.simulate_reads(g, 200, 3000, seed=5, mid_seed=True)
    G = binding.Graph(g.nodes, g.edges)

    def run():
        out = G.align(reads, seeds, 35, flags=binding.GA_F_TRACE)
        return [(r["status"], r["failed"], r["score"], r["alignment_start"], r["alignment_end"], r["mappings"], r["trace"].tobytes()) for r in out]
    before = run()
    G.build_seed_index(max_walks=64)
    G.find_seeds(reads)
    after = run()
    assert before == after
    assert sum(1 for r in after if r[0] == 0 and not r[1]) >= 190
