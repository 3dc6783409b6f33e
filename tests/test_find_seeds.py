"""ga_find_seeds against the model of tests/seed_model.py (seeds, support, hit count, truncation, for every read), its determinism,
the usability of the seeds (reads aligned from them against reads aligned from their true seeds) and the driver's --find-seeds.
CPU: the seeding program and the alignment programs built for the host (tests/emul)."""
import io
import os
import sys

import pytest

from graphaligner_amd import aligner, binding, compare, synth
import parity_common as pc
import seed_common as sc
import seed_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def world():
    lib = pc.emul_lib_path()
    g = synth.bubble_graph(30000, node_len=32, seed=3)
    G = binding.Graph(g.nodes, g.edges, lib_path=lib)
    G.build_seed_index()
    return g, G, seed_model.Model(g.nodes)


def test_seeds_equal_the_model(world):
    g, G, model = world
    reads = sc.spiked_reads(g)
    res = sc.check_reads(G, model, reads)
    by_len = {len(r): s for r, s in zip(reads, res.seeds)}
    assert by_len[150] == [] and by_len[385] == [] and by_len[10] == [] and by_len[0] == []      # the 193-bp rule
    assert sum(1 for r, s in zip(reads, res.seeds) if len(r) >= 1000 and s) >= 12                  # and the test is not vacuous
    for params in (dict(max_seeds=1), dict(max_seeds=3), dict(max_hits=16), dict(min_support=1, window=100, diag_tol=5), dict(max_occ=1)):
        r2 = sc.check_reads(G, model, reads, **params)
        if "max_hits" in params:
            assert any(r2.truncated) and max(r2.n_hits) == 16
        if params.get("max_seeds") == 3:
            assert max(len(s) for s in r2.seeds) <= 3
    # a read of 386 bp can have a seed: one is found with the noise filters off on an error-free read
    clean = synth.simulate_reads(g, 8, 386, sub=0.0, ins=0.0, dele=0.0, seed=40)[0]
    clean = [r[:386] for r in clean]
    r3 = sc.check_reads(G, model, clean, min_support=1)
    assert all(len(r) == 386 for r in clean) and any(r3.seeds) and all(p == 193 for s in r3.seeds for _, p, _ in s)


def test_other_k_and_sampling():
    lib = pc.emul_lib_path()
    g = synth.linear_graph(20000)
    reads = sc.spiked_reads(g, seed=11)
    for k, s in ((11, 0), (31, 3), (21, 5)):
        G = binding.Graph(g.nodes, g.edges, lib_path=lib)
        G.build_seed_index(k=k, sample_shift=s)
        sc.check_reads(G, seed_model.Model(g.nodes, k, s), reads)


def test_repeats_are_filtered():
    """a poly-A read against a graph with a long poly-A node and max_occ = 1: every k-mer of the read has many entries, nothing is used"""
    lib = pc.emul_lib_path()
    base = synth.random_genome(3000, 8).tobytes().decode()
    nodes = [(1, base[:1500]), (2, "A" * 600), (3, base[1500:])]
    edges = [(1, False, 2, False), (2, False, 3, False)]
    G = binding.Graph(nodes, edges, lib_path=lib)
    G.build_seed_index(k=15, sample_shift=0)
    model = seed_model.Model(nodes, 15, 0)
    reads = ["A" * 500, base[200:900] + "A" * 300 + base[1600:2200]]
    res = sc.check_reads(G, model, reads, max_occ=1)
    assert res.n_hits[0] == 0 and res.seeds[0] == [] and res.seeds[1] != []
    res = sc.check_reads(G, model, reads, max_occ=8)
    assert res.n_hits[0] == 0
    res = sc.check_reads(G, model, reads, max_occ=1000, max_hits=64)         # everything used: the buffer overflows
    assert res.truncated[0] and res.n_hits[0] == 64


def test_determinism(world):
    g, G, model = world
    reads = sc.spiked_reads(g, seed=21)
    a = G.find_seeds(reads)
    b = G.find_seeds(reads)
    c = G.find_seeds(reads[::-1])
    assert (a.seeds, a.support, a.n_hits, a.truncated) == (b.seeds, b.support, b.n_hits, b.truncated)
    assert (a.seeds, a.support, a.n_hits, a.truncated) == (c.seeds[::-1], c.support[::-1], c.n_hits[::-1], c.truncated[::-1])


def test_seeds_are_usable():
    """Reads aligned from the seeds found here against the same reads aligned from their true seeds, both judged against the
    simulation's truth by the reference's 0.7 rule; every read counts in both runs.  Required: good matches from own seeds >= good
    matches from true seeds - one read per hundred (a read whose best-ranked locus is a chance repeat).  The figures go to
    profiles/seed_accuracy_cpu.json."""
    g = synth.bubble_graph(40000, node_len=32, seed=11)
    truth = []
    reads, seeds = synth.simulate_reads(g, 100, 3000, seed=5, truth=truth)
    row = sc.accuracy(g, reads, seeds, truth, pc.emul_lib_path(), pc.emul_lib_path())
    row.pop("seed_kernel_ms")
    print("seed accuracy (host emulation):", row)
    sc.record("seed_accuracy_cpu.json", "bubble_graph(40000, node_len=32, seed=11), 100 x 3000 bp, seed=5", row)
    assert row["good_own_seeds"] >= row["good_true_seeds"] - row["allowance"], row
    assert row["good_true_seeds"] >= 90, row


def test_driver_finds_its_own_seeds(tmp_path, monkeypatch):
    """--find-seeds on files of the kind test_aligner_driver writes: the GAM's alignments pass the 0.7 rule against the truth; without
    the option the old message still comes"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_aligner_driver import _decode_gam
    g = synth.bubble_graph(30000, node_len=32, seed=21)
    truth = []
    reads, _ = synth.simulate_reads(g, 6, 1200, seed=77, mid_seed=True, truth=truth)
    names = ["r%d/x:%d" % (i, i) for i in range(len(reads))] + ["short", "orphan"]
    reads = reads + [reads[0][:100], "ACGT" * 120]                       # too short for a seed; a read that is not in the graph
    (tmp_path / "g.gfa").write_text(g.gfa())
    with open(tmp_path / "reads.fastq", "w") as f:
        for n, r in zip(names, reads):
            f.write("@%s\n%s\n+\n%s\n" % (n, r, "I" * len(r)))
    base = ["-g", str(tmp_path / "g.gfa"), "-f", str(tmp_path / "reads.fastq"), "-a", str(tmp_path / "out.gam"), "-t", "1", "-b", "35"]
    err = io.StringIO()
    with pytest.raises(SystemExit):
        aligner.parse_args(base, err=err)
    assert "either initial full band or seed file must be set" in err.getvalue()
    with pytest.raises(SystemExit):
        aligner.parse_args(base + ["--find-seeds", "-s", "x.gam"], err=err)
    p = aligner.parse_args(base + ["--find-seeds", "--seed-k", "15", "--seed-max", "2"])
    assert p.findSeeds and p.seedK == 15 and p.seedMax == 2
    p.outputDir = str(tmp_path)
    out, err = io.StringIO(), io.StringIO()
    monkeypatch.setenv("GA_EMUL_WITHOUT", "seeded")            # the two-call path: prepare_seeded is refused, find_seeds and prepare follow
    written = aligner.align_reads(p, lib_path=pc.emul_lib_path(), out=out, err=err)
    for n in ("short", "orphan"):
        assert "read %s has no seed hits" % n in out.getvalue() and "read %s has no seed hits" % n in err.getvalue()
    got = _decode_gam(str(tmp_path / "out.gam"))
    assert [a["name"] for a in got] == [n for n, _ in written]
    sizes = {nid: len(seq) for nid, seq in g.nodes}
    predicted = {a["name"]: [m[0] for m in a["mappings"]] for a in got}     # (the GAM carries bigraph ids)
    res = compare.compare({n: t for n, t in zip(names[:6], truth)}, predicted, sizes)
    assert res["good"] == 6 and res["bad"] == 0, (res, out.getvalue())
