"""Seeded batches (ga_batch_prepare_seeded) on the host build of tests/emul: the plan against the two-call path
(ga_find_seeds / ga_find_seeds_loci, then ga_batch_prepare) and against the model of tests/seed_plan_model.py, field by field; every
clause of the rule on hand-made inputs; the results against the two-call path's; the interface's refusals; the driver."""
import ctypes as C
import gzip
import io
import os

import numpy as np
import pytest

from graphaligner_amd import aligner, binding, synth
import parity_common as pc
import seed_common as sc
import seed_loci_common as slc
import seed_plan_common as spc
import seed_plan_model as spm

MODES = [dict(loci=False, max_seeds=1), dict(loci=False, max_seeds=2), dict(loci=False, max_seeds=4), dict(loci=True)]
MODE_IDS = ["hits-1", "hits-2", "hits-4", "loci"]


@pytest.fixture(scope="module")
def world():
    g = synth.bubble_graph(40000, node_len=32, seed=11)
    G = binding.Graph(g.nodes, g.edges, lib_path=pc.emul_lib_path())
    G.build_seed_index()
    return g, G, spm.bigraph_nodes(g.nodes)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_plan_three_ways(world, mode):
    g, G, dnodes = world
    reads = synth.simulate_reads(g, 12, 3000, seed=5)[0]
    plan, found = spc.check_plan(G, dnodes, 0, reads, **mode)
    assert len(plan["jobs"]) >= 24 and all(found.seeds)                       # the test is not vacuous
    plan, found = spc.check_plan(G, dnodes, 0, spc.mixed_reads(g, 12), **mode)
    assert [i for i, s in enumerate(found.seeds) if not s] == [0, 7, 8, 15]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257])
def test_plan_read_counts(world, n):
    """read counts either side of a wave, a block of 256 slots and the scans' tiles"""
    g, G, dnodes = world
    reads = synth.simulate_reads(g, n, 500, seed=40 + n)[0]
    plan, found = spc.check_plan(G, dnodes, 0, reads, loci=n % 2 == 0)
    assert sum(1 for s in found.seeds if s) >= (n + 1) // 2


def test_plan_shortest_reads_on_the_walk_index():
    g = synth.bubble_graph(30000, node_len=8, seed=3)
    G = binding.Graph(g.nodes, g.edges, lib_path=pc.emul_lib_path())
    G.build_seed_index(max_walks=64)
    clean = synth.simulate_reads(g, 1, 2000, sub=0.0, ins=0.0, dele=0.0, seed=8)[0][0]
    for mode in (dict(loci=False), dict(loci=True)):
        plan, found = spc.check_plan(G, spm.bigraph_nodes(g.nodes), 0, [clean[:386], clean[:387], clean[:385]], **mode)
        assert found.seeds[0] and found.seeds[1] and not found.seeds[2]
        assert found.seeds[0][0][1] == 193 and rows(plan["jobs"])[0][:2] == (0, 256)


def rows(a):
    return spc.rows(a)


# ---- every clause of the rule --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clean_world(world):
    g, G, dnodes = world
    return g, G, dnodes, synth.simulate_reads(g, 3, 2500, sub=0.0, ins=0.0, dele=0.0, seed=77)[0]


@pytest.fixture(scope="module")
def overlap16_world():
    nodes, edges, a = spc.overlap_graph(16)
    G = binding.Graph(nodes, edges, overlap=16, lib_path=pc.emul_lib_path())
    G.build_seed_index()
    return G, spm.bigraph_nodes(nodes), [a[300:1900], a[2300:3700]]


@pytest.mark.parametrize("case", list(spc.STAR_CASES), ids=list(spc.STAR_CASES))
def test_character_without_complement(clean_world, overlap16_world, case):
    """a character that ReverseComplement asserts on, at every place the rule tells apart.  A found seed's k-mer covers [p, p + k), so
    the two places around p + ovl lie outside it only on a graph whose overlap is at least k: those two run with dbg_overlap = 16"""
    where, ovl, jobs_made = spc.STAR_CASES[case]
    if ovl:
        G, dnodes, clean = overlap16_world
    else:
        g, G, dnodes, clean = clean_world
    spc.check_star_case(G, dnodes, ovl, clean, where, jobs_made)


def test_one_strand_node_and_unequal_strands():
    dnodes, (a, b, c) = spc.strand_graph()
    G = spc.DigraphGraph(dnodes, lib_path=pc.emul_lib_path())
    G.build_seed_index()
    reads = [a[200:1700], b[200:1700], c[200:1700], a[100:1900]]
    model_nodes = [(did, len(seq)) for did, seq in dnodes]
    plan, found = spc.check_plan(G, model_nodes, 0, reads, max_seeds=1)
    assert [s[0][0] for s in found.seeds] == [1, 2, 3, 1] and not any(s[0][2] for s in found.seeds)
    early = [s[2] for s in rows(plan["seeds"])]
    assert early == [spm.OK, spm.BAD_SEED, spm.ASSERTION, spm.OK]
    assert len(plan["jobs"]) == 4 and rows(plan["seeds"])[3][4:] == (2, 3)
    got, _ = spc.check_results(G, reads, max_seeds=1)
    assert [r["status"] for r in got] == [0, spm.BAD_SEED, spm.ASSERTION, 0]


def test_overlap_graph():
    """a graph finalised with dbg_overlap = 4: the backward job has p + 4 rows, of which p count; the forward job's last 4 do not"""
    nodes, edges, a = spc.overlap_graph(4)
    G = binding.Graph(nodes, edges, overlap=4, lib_path=pc.emul_lib_path())
    G.build_seed_index()
    reads = [a[300:1900], a[2300:3700]]
    plan, found = spc.check_plan(G, spm.bigraph_nodes(nodes), 4, reads, max_seeds=1)
    assert all(found.seeds)                                                   # (the seeder does give seeds here)
    for i, (rd, sd) in enumerate(zip(reads, found.seeds)):
        p = sd[0][1]
        bw, fw = rows(plan["jobs"])[2 * i], rows(plan["jobs"])[2 * i + 1]
        assert bw[1] == spm.padded(p + 4) and bw[3] == p and fw[1] == spm.padded(len(rd) - p) and fw[3] == len(rd) - p - 4
        assert rows(plan["fills"])[2 * i][2] == p + 4
    spc.check_results(G, reads, max_seeds=1)


def test_two_seeds_second_covered_by_the_first():
    g, reads = slc.repeat_case()
    G = binding.Graph(g.nodes, g.edges, lib_path=pc.emul_lib_path())
    G.build_seed_index()
    reads = [reads[0][:2600]]
    plan, found = spc.check_plan(G, spm.bigraph_nodes(g.nodes), 0, reads, max_seeds=2)
    assert len(found.seeds[0]) == 2 and len(plan["jobs"]) == 4
    got, _ = spc.check_results(G, reads, max_seeds=2)
    assert got[0]["status"] == 0 and not got[0]["failed"]


def test_scan_sums_stay_64_bit():
    """the layout step (slot sizes, the two scans, the writes) over fabricated job sizes whose sum passes 2^32 rows"""
    L = C.CDLL(pc.emul_lib_path())
    n_bw = np.array([0xffffff00, 0, 1, 0, 0xfffffe41, 65, 0], dtype=np.uint32)
    n_fw = np.array([0xfffffe00, 70, 0, 0, 64, 0xffffffc0, 5], dtype=np.uint32)
    n = len(n_bw)
    bw_off, fw_off = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    bw_rows, fw_rows = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    totals = np.zeros(2, dtype=np.uint64)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    L.ga_emul_seed_plan_layout.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32] + [C.c_void_p] * 5
    assert L.ga_emul_seed_plan_layout(ptr(n_bw), ptr(n_fw), n, 0, ptr(bw_off), ptr(fw_off), ptr(bw_rows), ptr(fw_rows), ptr(totals)) == 0
    at, jobs = 0, 0
    none = 2 ** 64 - 1
    for s in range(n):
        for size, off, got_rows in ((int(n_bw[s]), bw_off, bw_rows), (int(n_fw[s]), fw_off, fw_rows)):
            if size:
                assert int(off[s]) == at and int(got_rows[s]) == spm.padded(size), s
                at += spm.padded(size)
                jobs += 1
            else:
                assert int(off[s]) == none and int(got_rows[s]) == 0, s
    assert at > 3 * 2 ** 32 and (int(totals[0]), int(totals[1])) == (jobs, at)


# ---- results ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loci", [False, True], ids=["hits", "loci"])
def test_results_equal_the_two_call_path(world, loci):
    g, G, dnodes = world
    reads = synth.simulate_reads(g, 20, 1000, seed=5)[0]
    got, found = spc.check_results(G, reads, loci=loci)
    assert sum(1 for r in got if r["status"] == 0 and not r["failed"]) >= 18
    got, found = spc.check_results(G, sc.spiked_reads(g), loci=loci)
    assert [r["status"] for r, s in zip(got, found.seeds) if not s] == [spm.ASSERTION] * sum(1 for s in found.seeds if not s)


def test_results_with_trace_items(world):
    g, G, dnodes = world
    reads = synth.simulate_reads(g, 5, 900, seed=15)[0]
    got, _ = spc.check_results(G, reads, flags=binding.GA_F_TRACE)
    assert all(len(r["trace"]) > 800 for r in got)


# ---- interface ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(world):
    g, G, dnodes = world
    reads = synth.simulate_reads(g, 2, 1000, seed=5)[0]
    lib = pc.emul_lib_path()
    bare = binding.Graph(g.nodes[:200], [], lib_path=lib)
    rs = binding.ReadSet(reads, [[]] * 2)
    h = C.c_void_p()
    p = binding.GaSeedParams()
    G.L.ga_seed_params_default(C.byref(p))
    assert G.L.ga_batch_prepare_seeded(bare.h, rs.arr, 2, C.byref(p), 0, 35, 0, 0, C.byref(h)) == 100             # no index
    p.k = 17
    assert G.L.ga_batch_prepare_seeded(G.h, rs.arr, 2, C.byref(p), 0, 35, 0, 0, C.byref(h)) == 100                # not the index's k
    assert G.L.ga_batch_prepare_seeded(G.h, rs.arr, 2, None, 0, 35, 0, 0, C.byref(h)) == 0                        # NULL: the defaults
    G.L.ga_batch_free(h)
    with pytest.raises(binding.SeededUnsupported):
        bare.prepare_seeded(reads)
    plain = G.prepare(reads, G.find_seeds(reads).seeds, 35)
    out = C.c_void_p()
    st = binding.GaBatchPrepareStats()
    assert G.L.ga_batch_seeds(plain.h, C.byref(out)) == 100 and G.L.ga_batch_prepare_stats(plain.h, C.byref(st)) == 100
    assert len(plain.plan()["jobs"]) == 4


def test_older_host_builds_refuse(world):
    g, G, dnodes = world
    reads = synth.simulate_reads(g, 2, 1000, seed=5)[0]
    for profile in ("emul_seed", "emul_seed_loci", "emul_seed_coord"):
        with pc.emul_profile(profile):
            old = binding.Graph(g.nodes, g.edges, lib_path=pc.emul_lib_path())
        old.build_seed_index()
        with pytest.raises(binding.SeededUnsupported):
            old.prepare_seeded(reads)
        assert old.find_seeds(reads).seeds == G.find_seeds(reads).seeds
    with pc.emul_profile("emul"):
        unseeded = binding.Graph(g.nodes, g.edges, lib_path=pc.emul_lib_path())
    with pytest.raises(binding.SeededUnsupported):
        unseeded.prepare_seeded(reads)


def test_the_switch_is_read_per_graph():
    """GA_EMUL_WITHOUT belongs to the graph uploaded under it, not to the process or the library"""
    g = synth.bubble_graph(6000, node_len=32, seed=3)
    reads = synth.simulate_reads(g, 2, 300, seed=5)[0]
    lib = pc.emul_lib_path()
    with pc.emul_profile("emul_seed_coord"):
        without = binding.Graph(g.nodes, g.edges, lib_path=lib)
    with_it = binding.Graph(g.nodes, g.edges, lib_path=lib)
    for graph in (without, with_it):
        graph.build_seed_index()
    with pytest.raises(binding.SeededUnsupported):
        without.prepare_seeded(reads)
    with_it.prepare_seeded(reads).close()
    with pytest.raises(binding.SeededUnsupported):
        without.prepare_seeded(reads)


def test_find_seeds_is_left_alone(world):
    g, G, dnodes = world
    reads = sc.spiked_reads(g, seed=31)
    fresh = binding.Graph(g.nodes, g.edges, lib_path=pc.emul_lib_path())
    fresh.build_seed_index()
    before = spc.plain_seeds(fresh.find_seeds(reads)), spc.plain_seeds(fresh.find_seeds(reads, loci=True))
    fresh.prepare_seeded(reads).close()
    fresh.prepare_seeded(reads, loci=True).close()
    assert (spc.plain_seeds(fresh.find_seeds(reads)), spc.plain_seeds(fresh.find_seeds(reads, loci=True))) == before


@pytest.mark.parametrize("loci", [False, True], ids=["hits", "loci"])
def test_driver_output_is_byte_identical(tmp_path, loci, monkeypatch):
    """--find-seeds through seeded batches against the two-call path (the same back end with seeded batches withheld)"""
    g = synth.bubble_graph(30000, node_len=32, seed=21)
    reads, _ = synth.simulate_reads(g, 6, 1200, seed=77, mid_seed=True)
    names = ["r%d/x:%d" % (i, i) for i in range(len(reads))] + ["short", "orphan"]
    reads = reads + [reads[0][:100], "ACGT" * 120]
    (tmp_path / "g.gfa").write_text(g.gfa())
    (tmp_path / "r.fq").write_text("".join("@%s\n%s\n+\n%s\n" % (n, r, "I" * len(r)) for n, r in zip(names, reads)))
    outs = []
    for tag, without in (("seeded", ""), ("two", "seeded")):
        argv = ["-g", str(tmp_path / "g.gfa"), "-f", str(tmp_path / "r.fq"), "--find-seeds", "-a", str(tmp_path / (tag + ".gam")), "-t", "1", "-b", "35"]
        params = aligner.parse_args(argv + (["--seed-loci"] if loci else []))
        params.outputDir = str(tmp_path)                                   # (the per-read files: the same names both times)
        out, err = io.StringIO(), io.StringIO()
        monkeypatch.setenv("GA_EMUL_WITHOUT", without)
        written = aligner.align_reads(params, lib_path=pc.emul_lib_path(), out=out, err=err)
        # (a GAM file is gzip members, whose headers carry the time of writing: the bytes compared are the members' contents)
        plain = lambda f: gzip.decompress((tmp_path / f).read_bytes()) if f.endswith(".gam") else (tmp_path / f).read_bytes()
        per_read = [(f, plain(f)) for f in sorted(os.listdir(tmp_path)) if f.startswith(("alignment_0_", "trace_0_"))]
        outs.append((out.getvalue().replace(tag + ".gam", "out.gam"), err.getvalue(), plain(tag + ".gam"), len(written), per_read))
        assert len(per_read) == 2 * len(written)
    assert outs[0] == outs[1] and outs[0][3] >= 5
    assert "read short has no seed hits" in outs[0][0]

