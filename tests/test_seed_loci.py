"""ga_find_seeds_loci (one seed per locus) against the model of tests/seed_loci_model.py: seeds, support, the three locus fields,
n_loci, hit count and truncation for every read; the hand-made cases of the rule (zigzag, gap, repeat); determinism; that the call
leaves ga_find_seeds alone; what the feature is for (a long read gets one seed where it got two); the usability of the seeds and the
driver's --seed-loci.  CPU: the seeding program and the alignment programs built for the host (tests/emul)."""
import ctypes as C
import io
import os
import sys

import pytest

from graphaligner_amd import aligner, binding, compare, synth
import parity_common as pc
import seed_common as sc
import seed_loci_common as slc
import seed_model
import seed_walk_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def world():
    lib = pc.emul_lib_path()
    g = synth.bubble_graph(30000, node_len=32, seed=3)
    G = binding.Graph(g.nodes, g.edges, lib_path=lib)
    G.build_seed_index()
    return g, G, seed_model.Model(g.nodes)


@pytest.mark.parametrize("params", slc.PARAM_SETS, ids=lambda p: ",".join("%s=%s" % kv for kv in p.items()) or "defaults")
def test_loci_equal_the_model(world, params):
    g, G, model = world
    reads = sc.spiked_reads(g)
    res = slc.check_reads(G, model, reads, **params)
    by_len = {len(r): i for i, r in enumerate(reads)}
    for n in (150, 385, 10, 0):                                               # the 193-bp rule, and the empty read
        assert res.seeds[by_len[n]] == [] and res.n_loci[by_len[n]] == 0
    assert sum(1 for r, s in zip(reads, res.seeds) if len(r) >= 1000 and s) >= 12                  # the test is not vacuous
    if "max_hits" in params:
        assert any(res.truncated) and max(res.n_hits) == 16
    if "max_seeds" in params:
        assert max(len(s) for s in res.seeds) <= params["max_seeds"]
    if "window" in params:
        assert max(res.n_loci) > 3                                            # a narrow window and diagonal: many loci per read


def test_loci_on_the_walk_index():
    lib = pc.emul_lib_path()
    g = synth.bubble_graph(30000, node_len=8, seed=3)
    G = binding.Graph(g.nodes, g.edges, lib_path=lib)
    G.build_seed_index(max_walks=64)
    reads = sc.spiked_reads(g)
    res = slc.check_reads(G, seed_walk_model.WalkModel(g.nodes, g.edges), reads)
    assert sum(1 for r, s in zip(reads, res.seeds) if len(r) >= 1000 and s) >= 12
    cyc = synth.cyclic_graph(3000, node_len=16)
    Cy = binding.Graph(cyc.nodes, cyc.edges, lib_path=lib)
    Cy.build_seed_index(max_walks=64)
    res = slc.check_reads(Cy, seed_walk_model.WalkModel(cyc.nodes, cyc.edges), synth.walk_reads(cyc, 6, 1200, seed=3)[0], max_seeds=4)
    assert any(res.seeds)


def test_zigzag_is_one_locus():
    nodes, reads, params, inside = slc.zigzag_case()
    G = binding.Graph(nodes, [], lib_path=pc.emul_lib_path())
    G.build_seed_index(k=params["k"], sample_shift=params["sample_shift"])
    res = slc.check_reads(G, seed_model.Model(nodes, params["k"], params["sample_shift"]), reads, **params)
    slc.check_zigzag(res, reads, inside)


def test_gap_is_two_loci_and_one_seed():
    g, reads = slc.gap_case()
    G = binding.Graph(g.nodes, g.edges, lib_path=pc.emul_lib_path())
    G.build_seed_index()
    slc.check_gap(slc.check_reads(G, seed_model.Model(g.nodes), reads))


def test_repeat_gives_one_seed_per_copy():
    g, reads = slc.repeat_case()
    G = binding.Graph(g.nodes, g.edges, lib_path=pc.emul_lib_path())
    G.build_seed_index()
    slc.check_repeat(slc.check_reads(G, seed_model.Model(g.nodes), reads, max_seeds=2))


def test_determinism(world):
    g, G, model = world
    reads = sc.spiked_reads(g, seed=21)
    a = G.find_seeds(reads, loci=True)
    b = G.find_seeds(reads, loci=True)
    c = G.find_seeds(reads[::-1], loci=True)
    assert slc.plain(a) == slc.plain(b)
    assert slc.plain(a) == tuple(x[::-1] for x in slc.plain(c))


def test_find_seeds_is_left_alone(world):
    g, G, model = world
    reads = sc.spiked_reads(g, seed=31)
    fresh = binding.Graph(g.nodes, g.edges, lib_path=pc.emul_lib_path())
    fresh.build_seed_index()
    before = fresh.find_seeds(reads)
    fresh.find_seeds(reads, loci=True)
    after = fresh.find_seeds(reads)
    assert (before.seeds, before.support, before.n_hits, before.truncated) == (after.seeds, after.support, after.n_hits, after.truncated)
    assert after.locus_hits is None and after.locus_span is None and after.n_loci is None
    sc.check_reads(fresh, model, reads)
    # the four new pointers of the set are null in what ga_find_seeds returns
    L = fresh.L
    arr = (binding.GaRead * 1)()
    keep = reads[0].encode()
    arr[0].name, arr[0].sequence, arr[0].length = b"", keep, len(keep)
    out = C.POINTER(binding.GaSeedSetLoci)()
    assert L.ga_find_seeds(fresh.h, arr, 1, None, C.byref(out)) == 0
    S = out.contents
    assert not S.locus_hits and not S.locus_first_p and not S.locus_last_p and not S.n_loci and bool(S.n_hits)
    L.ga_seed_set_free(out)


def test_the_older_host_builds_refuse():
    """back ends without findLoci (the profiles emul_seed and emul_seed_walks of parity_common.PROFILES): GA_E_INVALID through the
    back end's default, and their own call works as before"""
    g = synth.bubble_graph(6000, node_len=32, seed=3)
    reads = synth.simulate_reads(g, 2, 1000, seed=5)[0]
    for profile in ("emul_seed", "emul_seed_walks"):
        with pc.emul_profile(profile):
            G = binding.Graph(g.nodes, g.edges, lib_path=pc.emul_lib_path())
        G.build_seed_index()
        with pytest.raises(RuntimeError, match=r"ga_find_seeds_loci failed: .*\(100\)"):
            G.find_seeds(reads, loci=True)
        assert any(G.find_seeds(reads).seeds)
    with pytest.raises(TypeError):
        G.find_seeds(reads, locus=True)


def test_a_long_read_gets_one_seed():
    """The point of the feature.  Without `loci` at least a quarter of the reads get two seeds (22 of 40 when this was written): the
    second is the first one's place again, further along the drifting diagonal.  With it at most max(1, n // 100) do, every read
    that had a seed still has one, and the first seed is the ungrouped first seed."""
    g = synth.bubble_graph(60000, node_len=32, seed=3)
    reads = synth.simulate_reads(g, 40, 5000, seed=5)[0]
    G = binding.Graph(g.nodes, g.edges, lib_path=pc.emul_lib_path())
    G.build_seed_index()
    old = G.find_seeds(reads)
    new = slc.check_reads(G, seed_model.Model(g.nodes), reads)
    n = len(reads)
    two_old, two_new = sum(1 for s in old.seeds if len(s) == 2), sum(1 for s in new.seeds if len(s) == 2)
    print("reads with two seeds: %d of %d ungrouped, %d grouped" % (two_old, n, two_new))
    assert two_old >= n / 4
    assert two_new <= max(1, n // 100)
    for i in range(n):
        assert bool(new.seeds[i]) == bool(old.seeds[i])
        assert new.seeds[i][:1] == old.seeds[i][:1] and new.support[i][:1] == old.support[i][:1]


def test_grouped_seeds_are_usable():
    """the harness and the inputs of test_find_seeds.py::test_seeds_are_usable with loci=True: good matches from grouped seeds >= good
    matches from true seeds - one read per hundred.  The figures go to profiles/seed_loci_accuracy_cpu.json."""
    g = synth.bubble_graph(40000, node_len=32, seed=11)
    truth = []
    reads, seeds = synth.simulate_reads(g, 100, 3000, seed=5, truth=truth)
    row = slc.accuracy(g, reads, seeds, truth, pc.emul_lib_path(), pc.emul_lib_path())
    row.pop("seed_kernel_ms")
    row.pop("seed_kernel_ms_ungrouped")
    print("grouped seed accuracy (host emulation):", row)
    sc.record("seed_loci_accuracy_cpu.json", "bubble_graph(40000, node_len=32, seed=11), 100 x 3000 bp, seed=5", row)
    assert row["good_own_seeds"] >= row["good_true_seeds"] - row["allowance"], row
    assert row["good_true_seeds"] >= 90, row
    assert row["seeds"] <= row["seeds_ungrouped"], row


def test_driver_seed_loci(tmp_path, monkeypatch):
    """--find-seeds --seed-loci on files of the kind test_find_seeds.py::test_driver_finds_its_own_seeds writes: the GAM's alignments
    pass the 0.7 rule against the truth; --seed-loci without --find-seeds is refused"""
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
        aligner.parse_args(base + ["-s", "x.gam", "--seed-loci"], err=err)
    assert "--seed-loci goes with --find-seeds" in err.getvalue()
    assert not aligner.parse_args(base + ["--find-seeds"]).seedLoci
    p = aligner.parse_args(base + ["--find-seeds", "--seed-loci"])
    assert p.findSeeds and p.seedLoci
    p.outputDir = str(tmp_path)
    out, err = io.StringIO(), io.StringIO()
    monkeypatch.setenv("GA_EMUL_WITHOUT", "seeded")            # the two-call path: prepare_seeded is refused, find_seeds and prepare follow
    written = aligner.align_reads(p, lib_path=pc.emul_lib_path(), out=out, err=err)
    for n in ("short", "orphan"):
        assert "read %s has no seed hits" % n in out.getvalue() and "read %s has no seed hits" % n in err.getvalue()
    assert "one seed per locus: 6 seeds from 6 loci" in out.getvalue(), out.getvalue()
    got = _decode_gam(str(tmp_path / "out.gam"))
    assert [a["name"] for a in got] == [n for n, _ in written]
    sizes = {nid: len(seq) for nid, seq in g.nodes}
    predicted = {a["name"]: [m[0] for m in a["mappings"]] for a in got}     # (the GAM carries bigraph ids)
    res = compare.compare({n: t for n, t in zip(names[:6], truth)}, predicted, sizes)
    assert res["good"] == 6 and res["bad"] == 0, (res, out.getvalue())
