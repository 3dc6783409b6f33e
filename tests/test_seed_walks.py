"""The walk index (ga_graph_build_seed_index_walks / ga_graph_seed_index_walk_stats: k-mers of walks that leave a node through its
out-edges, for graphs of nodes shorter than k) against the model of tests/seed_walk_model.py, entry for entry and seed for seed; the
rule's corner cases on hand-made graphs; the usability of the seeds on a graph of 8-bp nodes; the driver's --seed-walks.
CPU: the seeding program of graphaligner_amd/csrc/ga_seed.h and the alignment programs built for the host
(tests/emul); tests/test_seed_walks_gpu.py repeats the comparisons through the product library."""
import ctypes as C
import io
import os
import sys

import pytest

from graphaligner_amd import aligner, binding, compare, synth
import parity_common as pc
import seed_common as sc
import seed_model
import seed_walk_common as swc
import seed_walk_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def rc(s):
    return "".join(COMP[c] for c in reversed(s))


def text(n, seed):
    return synth.random_genome(n, seed).tobytes().decode()


def entries(G):
    keys, idx, offs = G.seed_index_entries()
    return list(zip(keys.tolist(), idx.tolist(), offs.tolist()))


@pytest.mark.parametrize("name,k,s,max_walks", list(swc.walk_index_cases()))
def test_walk_index_equals_the_model(name, k, s, max_walks):
    g = swc.GRAPHS[name]()
    _, _, st, ws = swc.check_walk_index(g.nodes, g.edges, k, s, max_walks, pc.emul_lib_path())
    if name == "short8":
        # the in-node index of this graph is (nearly) empty (test_seed_index.py); here nearly every base starts a k-mer
        assert ws["tail_starts_skipped"] == 0 and st["kmers_seen"] > 0.9 * 2 * sum(len(seq) for _, seq in g.nodes)
    if name == "linear":
        # one walk per tail start but the last k - 1 of either strand
        assert ws["tail_starts_skipped"] == 0 and ws["duplicates_dropped"] == 0
        assert st["kmers_seen"] == 2 * (sum(len(seq) for _, seq in g.nodes) - k + 1)


# ---- hand-made graphs -------------------------------------------------------------------------------------------------------------
def test_two_branches_of_equal_text_give_one_entry():
    a, b = text(20, 1), text(20, 2)
    nodes = [(1, a), (2, "ACGT"), (3, "ACGT"), (4, b)]
    edges = [(1, False, 2, False), (1, False, 3, False), (2, False, 4, False), (3, False, 4, False)]
    G, model, st, ws = swc.check_walk_index(nodes, edges, 11, 0, 64, pc.emul_lib_path())
    # the tail starts of node 1 (index 1), offsets 10..19, have two walks each with the same text
    assert ws["duplicates_dropped"] >= 10 and ws["tail_starts_skipped"] == 0
    mine = [e for e in entries(G) if e[1] == 1 and e[2] >= 10]
    assert [e[2] for e in sorted(mine, key=lambda e: e[2])] == list(range(10, 20))
    for key, _, o in mine:
        assert key == seed_walk_model.key_of((a[o:] + "ACGT" + b)[:11])
    # with max_walks 1 those starts have one walk too many
    _, _, _, ws1 = swc.check_walk_index(nodes, edges, 11, 0, 1, pc.emul_lib_path())
    assert ws1["tail_starts_skipped"] >= 10


def test_a_dead_end_inside_k_bases_gives_nothing():
    a = text(20, 3)
    nodes = [(1, a), (2, "ACG")]
    G, model, st, ws = swc.check_walk_index(nodes, [(1, False, 2, False)], 11, 0, 64, pc.emul_lib_path())
    # forward node 1: offsets 0..9 lie inside it; 10, 11, 12 reach 11 bases with the 3 of node 2; later ones end before
    assert sorted(e[2] for e in entries(G) if e[1] == 1) == list(range(13))
    assert ws["tail_starts"] == 2 * (10 + 3) and ws["walk_kmers"] == 3 + 3          # reverse strand: node 2' (3 bp) walks into node 1'
    assert st["kmers_seen"] == 2 * 10 + 6


def test_an_edge_with_a_reverse_flag():
    a, b = text(20, 4), text(20, 5)
    nodes = [(1, a), (2, b)]
    G, model, st, ws = swc.check_walk_index(nodes, [(1, False, 2, True)], 11, 0, 64, pc.emul_lib_path())
    # node 1 forward (index 1) goes on into node 2 reversed; node 2 forward (index 3) into node 1 reversed
    got = {(n, o): key for key, n, o in entries(G)}
    for o in range(10, 20):
        assert got[(1, o)] == seed_walk_model.key_of((a[o:] + rc(b))[:11])
        assert got[(3, o)] == seed_walk_model.key_of((b[o:] + rc(a))[:11])
        assert (2, o) not in got and (4, o) not in got                             # the reverse copies have no out-edge
    assert ws["walk_kmers"] == 20


def test_a_self_loop_on_a_three_bp_node():
    a, b = text(20, 6), text(20, 7)
    nodes = [(1, a), (2, "ACG"), (3, b)]
    edges = [(1, False, 2, False), (2, False, 2, False), (2, False, 3, False)]
    G, model, st, ws = swc.check_walk_index(nodes, edges, 11, 0, 64, pc.emul_lib_path())
    keys_of_loop_node = set(key for key, n, o in entries(G) if n == 3 and o == 0)
    # from the loop node's first base: around the loop 0, 1, 2 times and out, or three more times around
    want = set(seed_walk_model.key_of(("ACG" * r + b)[:11]) for r in (1, 2, 3)) | {seed_walk_model.key_of(("ACG" * 4)[:11])}
    assert keys_of_loop_node == want


def fan(order):
    nodes = [(1, text(20, 8))] + [(2 + i, text(20, 20 + i)) for i in range(5)]
    edges = [(1, False, 2 + i, False) for i in order]
    return nodes, edges


def test_a_fan_over_the_cap_is_skipped_and_counted():
    nodes, edges = fan(range(5))
    lib = pc.emul_lib_path()
    G, _, _, ws = swc.check_walk_index(nodes, edges, 11, 0, 4, lib)
    assert ws["tail_starts_skipped"] == 10                                          # node 1's ten tail starts have five walks each
    assert [e for e in entries(G) if e[1] == 1 and e[2] >= 10] == []
    assert [e for e in entries(G) if e[1] == 4 and e[2] >= 10] != []                # the branches' reverse copies have one walk each
    G, _, _, ws = swc.check_walk_index(nodes, edges, 11, 0, 5, lib)
    assert ws["tail_starts_skipped"] == 0 and ws["walk_kmers"] == 10 * 5 + 5 * 10
    assert sorted(set(e[2] for e in entries(G) if e[1] == 1 and e[2] >= 10)) == list(range(10, 20))


@pytest.mark.parametrize("max_walks", [4, 64])
def test_the_order_of_the_neighbours_does_not_matter(max_walks):
    lib = pc.emul_lib_path()
    got = []
    for order in ((0, 1, 2, 3, 4), (3, 0, 4, 2, 1)):
        nodes, edges = fan(order)
        G, _, _, ws = swc.check_walk_index(nodes, edges, 11, 0, max_walks, lib)
        got.append((entries(G), ws))
    assert got[0] == got[1]
    # and on a graph with bubbles: the same edges back to front
    g = swc.GRAPHS["cyclic16"]()
    a, _, _, wa = swc.check_walk_index(g.nodes, g.edges, 15, 0, max_walks, lib)
    b, _, _, wb = swc.check_walk_index(g.nodes, g.edges[::-1], 15, 0, max_walks, lib)
    assert entries(a) == entries(b) and wa == wb


# ---- properties of the rule -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,n_entries", [(15, 6885), (31, 7822)])
def test_the_index_does_not_depend_on_where_the_nodes_are_cut(k, n_entries):
    """the same sequence and variants cut into 8-bp and into 32-bp nodes: the same keys, as long as no tail start is skipped"""
    lib = pc.emul_lib_path()
    keys = []
    for node_len in (8, 32):
        g = synth.bubble_graph(12000, node_len=node_len, seed=3)
        G = binding.Graph(g.nodes, g.edges, lib_path=lib)
        G.build_seed_index(k=k, sample_shift=2, max_walks=64)
        assert G.seed_index_walk_stats()["tail_starts_skipped"] == 0
        keys.append(sorted(G.seed_index_entries()[0].tolist()))
    assert keys[0] == keys[1]
    assert len(keys[0]) == n_entries


def test_the_cap_is_exercised():
    g = synth.cyclic_graph(3000, node_len=16)
    lib = pc.emul_lib_path()
    _, _, _, ws = swc.check_walk_index(g.nodes, g.edges, 31, 0, 4, lib)
    assert ws["tail_starts_skipped"] > 0
    _, _, _, ws = swc.check_walk_index(g.nodes, g.edges, 31, 0, 64, lib)
    assert ws["tail_starts_skipped"] == 0


@pytest.mark.parametrize("name", ["bubbles32", "linear", "cyclic16"])
def test_the_in_node_entries_are_those_of_the_old_index(name):
    g = swc.GRAPHS[name]()
    G = binding.Graph(g.nodes, g.edges, lib_path=pc.emul_lib_path())
    G.build_seed_index(k=15, sample_shift=2)
    old = entries(G)
    G.build_seed_index(k=15, sample_shift=2, max_walks=64)
    length = lambda index: len(g.nodes[(index - 1) // 2][1])
    assert old != [] and [e for e in entries(G) if e[2] + 15 <= length(e[1])] == old
    assert all(e[2] + 15 <= length(e[1]) for e in old)


def test_bad_arguments_are_refused_and_a_rebuild_replaces_the_index():
    lib = pc.emul_lib_path()
    L = binding.load(lib)
    g = synth.bubble_graph(6000, node_len=8, seed=3)
    G = binding.Graph(g.nodes, g.edges, lib_path=lib)
    ws = binding.GaSeedWalkStats()
    assert L.ga_graph_seed_index_walk_stats(G.h, C.byref(ws)) == 100                # no index yet: GA_E_INVALID
    for k, s, w in ((15, 2, 0), (15, 2, 257), (10, 2, 64), (32, 2, 64), (15, 9, 64)):
        assert L.ga_graph_build_seed_index_walks(G.h, k, s, w) == 100
    assert L.ga_graph_seed_index_walk_stats(G.h, C.byref(ws)) == 100                # a refused build leaves no index
    a = G.build_seed_index(k=15, sample_shift=2)
    assert a["entries"] == 0 and a["kmers_seen"] == 0                               # nodes of 8 bp: nothing inside a node
    assert L.ga_graph_seed_index_walk_stats(G.h, C.byref(ws)) == 100                # an in-node index
    with pytest.raises(RuntimeError):
        G.seed_index_walk_stats()
    b = G.build_seed_index(k=15, sample_shift=2, max_walks=64)
    wb = G.seed_index_walk_stats()
    assert b["entries"] > 0 and wb["max_walks"] == 64 and b["kmers_seen"] == wb["walk_kmers"]
    assert L.ga_graph_seed_index_walk_stats(G.h, None) == 100
    c = G.build_seed_index(k=11, sample_shift=0, max_walks=4)
    assert c["k"] == 11 and c["entries"] > b["entries"] and G.seed_index_walk_stats()["max_walks"] == 4
    d = G.build_seed_index(k=15, sample_shift=2)                                    # and back
    assert (d["entries"], d["kmers_seen"], d["distinct_keys"]) == (0, 0, 0)
    assert L.ga_graph_seed_index_walk_stats(G.h, C.byref(ws)) == 100
    # before finalize / upload
    h = L.ga_graph_create()
    assert L.ga_graph_add_bigraph_node(h, 1, b"ACGTACGTACGTACGTACGT", 20) == 0
    assert L.ga_graph_build_seed_index_walks(h, 15, 2, 64) == 103                   # GA_E_NOT_FINALIZED
    assert L.ga_graph_finalize(h, 0) == 0
    assert L.ga_graph_build_seed_index_walks(h, 15, 2, 64) == 101                   # GA_E_NO_DEVICE: not uploaded
    L.ga_graph_destroy(h)
    # a back end that only knows the in-node build refuses through the back end's default
    with pc.emul_profile("emul_seed"):
        O = binding.Graph(g.nodes, g.edges, lib_path=pc.emul_lib_path())
    assert O.L.ga_graph_build_seed_index_walks(O.h, 15, 2, 64) == 100


# ---- seeds ------------------------------------------------------------------------------------------------------------------------
def test_walk_seeds_equal_the_model():
    lib = pc.emul_lib_path()
    g = synth.bubble_graph(30000, node_len=8, seed=3)
    G = binding.Graph(g.nodes, g.edges, lib_path=lib)
    G.build_seed_index(max_walks=64)
    model = seed_walk_model.WalkModel(g.nodes, g.edges)
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
    clean = [r[:386] for r in synth.simulate_reads(g, 8, 386, sub=0.0, ins=0.0, dele=0.0, seed=40)[0]]
    r3 = sc.check_reads(G, model, clean, min_support=1)
    assert all(len(r) == 386 for r in clean) and any(r3.seeds) and all(p == 193 for s in r3.seeds for _, p, _ in s)
    # determinism: twice, and with the reads in reversed order
    a, b, c = G.find_seeds(reads), G.find_seeds(reads), G.find_seeds(reads[::-1])
    assert (a.seeds, a.support, a.n_hits, a.truncated) == (b.seeds, b.support, b.n_hits, b.truncated)
    assert (a.seeds, a.support, a.n_hits, a.truncated) == (c.seeds[::-1], c.support[::-1], c.n_hits[::-1], c.truncated[::-1])
    # the in-node index of this graph has nothing to offer
    G.build_seed_index()
    assert not any(G.find_seeds(reads).seeds)
    # a cyclic graph and another (k, s), with the cap met
    cyc = synth.cyclic_graph(3000, node_len=16)
    Cy = binding.Graph(cyc.nodes, cyc.edges, lib_path=lib)
    Cy.build_seed_index(k=31, sample_shift=0, max_walks=4)
    assert Cy.seed_index_walk_stats()["tail_starts_skipped"] > 0
    sc.check_reads(Cy, seed_walk_model.WalkModel(cyc.nodes, cyc.edges, 31, 0, 4), synth.walk_reads(cyc, 6, 1200, seed=3)[0])


def test_walk_seeds_are_usable():
    """100 reads x 3 kb on a graph of 8-bp nodes, aligned from the seeds the walk index gives against the same reads aligned from
    their true seeds, both judged against the simulation's truth by the reference's 0.7 rule; every read counts in both runs.
    Required: the in-node index gives no read a seed; good matches from own seeds >= good matches from true seeds - one read per
    hundred; good matches from true seeds >= 90.  The figures go to profiles/seed_walks_accuracy_cpu.json."""
    g = synth.bubble_graph(40000, node_len=8, seed=11)
    truth = []
    reads, seeds = synth.simulate_reads(g, 100, 3000, seed=5, truth=truth)
    row = swc.accuracy_walks(g, reads, seeds, truth, pc.emul_lib_path(), pc.emul_lib_path(), 64)
    row.pop("seed_kernel_ms")
    print("walk seed accuracy (host emulation):", row)
    sc.record("seed_walks_accuracy_cpu.json", "bubble_graph(40000, node_len=8, seed=11), 100 x 3000 bp, seed=5, max_walks=64", row)
    assert row["reads_with_seed_in_node_index"] == 0 and row["in_node_index_entries"] == 0, row
    assert row["good_own_seeds"] >= row["good_true_seeds"] - row["allowance"], row
    assert row["good_true_seeds"] >= 90, row


def test_driver_seed_walks(tmp_path, monkeypatch):
    """--find-seeds --seed-walks 64 on a GFA of 8-bp nodes: the GAM's alignments pass the 0.7 rule against the truth; without
    --seed-walks the same command finds no seed for any read"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_aligner_driver import _decode_gam
    g = synth.bubble_graph(30000, node_len=8, seed=21)
    truth = []
    reads, _ = synth.simulate_reads(g, 6, 1200, seed=77, mid_seed=True, truth=truth)
    names = ["r%d/x:%d" % (i, i) for i in range(len(reads))]
    (tmp_path / "g.gfa").write_text(g.gfa())
    with open(tmp_path / "reads.fastq", "w") as f:
        for n, r in zip(names, reads):
            f.write("@%s\n%s\n+\n%s\n" % (n, r, "I" * len(r)))
    base = ["-g", str(tmp_path / "g.gfa"), "-f", str(tmp_path / "reads.fastq"), "-a", str(tmp_path / "out.gam"), "-t", "1", "-b", "35"]
    err = io.StringIO()
    for bad in (["--find-seeds", "--seed-walks", "257"], ["--find-seeds", "--seed-walks", "-1"], ["-s", "x.gam", "--seed-walks", "64"]):
        with pytest.raises(SystemExit):
            aligner.parse_args(base + bad, err=err)
    assert "--seed-walks" in err.getvalue()
    assert aligner.parse_args(base + ["--find-seeds"]).seedWalks == 0
    # without the option: today's behaviour
    p = aligner.parse_args(base + ["--find-seeds"])
    p.outputDir = str(tmp_path)
    out, err = io.StringIO(), io.StringIO()
    monkeypatch.setenv("GA_EMUL_WITHOUT", "seeded")            # the two-call path: prepare_seeded is refused, find_seeds and prepare follow
    aligner.align_reads(p, lib_path=pc.emul_lib_path(), out=out, err=err)
    for n in names:
        assert "read %s has no seed hits" % n in out.getvalue()
    assert "seed index: 0 entries" in out.getvalue() and "tail starts" not in out.getvalue()
    # with it
    p = aligner.parse_args(base + ["--find-seeds", "--seed-walks", "64"])
    assert p.findSeeds and p.seedWalks == 64
    p.outputDir = str(tmp_path)
    out, err = io.StringIO(), io.StringIO()
    written = aligner.align_reads(p, lib_path=pc.emul_lib_path(), out=out, err=err)
    assert "has no seed hits" not in out.getvalue()
    assert "walks: 0 of " in out.getvalue() and "tail starts skipped (more than 64 walks)" in out.getvalue()
    got = _decode_gam(str(tmp_path / "out.gam"))
    assert [a["name"] for a in got] == [n for n, _ in written]
    sizes = {nid: len(seq) for nid, seq in g.nodes}
    predicted = {a["name"]: [m[0] for m in a["mappings"]] for a in got}     # (the GAM carries bigraph ids)
    res = compare.compare({n: t for n, t in zip(names, truth)}, predicted, sizes)
    assert res["good"] == 6 and res["bad"] == 0, (res, out.getvalue())
