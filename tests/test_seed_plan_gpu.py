"""Seeded batches (ga_batch_prepare_seeded) on the MI355X through the product library: plan, seeds and results against the two-call path
(ga_find_seeds / ga_find_seeds_loci, then ga_batch_prepare) on the same device, exactly, and the plan against the model of
tests/seed_plan_model.py; every clause of the rule on the hand-made inputs of tests/test_seed_plan.py; one call of 20 000 reads; two
batches prepared from two host threads; a batch run twice; the plan kernels' rows of the resource table.  Everything read here lies
inside the repository.  (The layout step over fabricated sizes past 2^32 rows has no GPU twin: it needs a test entry point that the
product library does not have; tests/test_seed_plan.py runs it on the host build of the same source.)"""
import json
import os
import threading

import numpy as np
import pytest

from graphaligner_amd import binding, synth
import seed_common as sc
import seed_loci_common as slc
import seed_plan_common as spc
import seed_plan_model as spm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [dict(loci=False, max_seeds=1), dict(loci=False, max_seeds=2), dict(loci=False, max_seeds=4), dict(loci=True)]
MODE_IDS = ["hits-1", "hits-2", "hits-4", "loci"]


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu test needs a GPU")


@pytest.fixture(scope="module")
def world():
    g = synth.bubble_graph(40000, node_len=32, seed=11)
    G = binding.Graph(g.nodes, g.edges)
    G.build_seed_index()
    return g, G, spm.bigraph_nodes(g.nodes)


@pytest.fixture(params=["lanes-first", "ladder-first"])
def first_pass(request, monkeypatch):
    monkeypatch.setenv("GA_LANES", "1" if request.param == "lanes-first" else "0")
    return request.param


# ---- the plan, three ways ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_plan_three_ways_gpu(world, mode):
    g, G, dnodes = world
    reads = synth.simulate_reads(g, 12, 3000, seed=5)[0]
    plan, found = spc.check_plan(G, dnodes, 0, reads, **mode)
    assert len(plan["jobs"]) >= 24 and all(found.seeds)
    plan, found = spc.check_plan(G, dnodes, 0, spc.mixed_reads(g, 12), **mode)
    assert [i for i, s in enumerate(found.seeds) if not s] == [0, 7, 8, 15]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257])
def test_plan_read_counts_gpu(world, n):
    g, G, dnodes = world
    reads = synth.simulate_reads(g, n, 500, seed=40 + n)[0]
    plan, found = spc.check_plan(G, dnodes, 0, reads, loci=n % 2 == 0)
    assert sum(1 for s in found.seeds if s) >= (n + 1) // 2


def test_plan_shortest_reads_on_the_walk_index_gpu():
    g = synth.bubble_graph(30000, node_len=8, seed=3)
    G = binding.Graph(g.nodes, g.edges)
    G.build_seed_index(max_walks=64)
    clean = synth.simulate_reads(g, 1, 2000, sub=0.0, ins=0.0, dele=0.0, seed=8)[0][0]
    for mode in (dict(loci=False), dict(loci=True)):
        plan, found = spc.check_plan(G, spm.bigraph_nodes(g.nodes), 0, [clean[:386], clean[:387], clean[:385]], **mode)
        assert found.seeds[0] and found.seeds[1] and not found.seeds[2]
        assert found.seeds[0][0][1] == 193 and spc.rows(plan["jobs"])[0][:2] == (0, 256)


# ---- every clause of the rule -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(spc.STAR_CASES), ids=list(spc.STAR_CASES))
def test_character_without_complement_gpu(world, case):
    where, ovl, jobs_made = spc.STAR_CASES[case]
    if ovl:
        nodes, edges, a = spc.overlap_graph(16)
        G = binding.Graph(nodes, edges, overlap=16)
        G.build_seed_index()
        dnodes, clean = spm.bigraph_nodes(nodes), [a[300:1900], a[2300:3700]]
    else:
        g, G, dnodes = world
        clean = synth.simulate_reads(g, 3, 2500, sub=0.0, ins=0.0, dele=0.0, seed=77)[0]
    spc.check_star_case(G, dnodes, ovl, clean, where, jobs_made)


def test_one_strand_node_and_unequal_strands_gpu():
    dnodes, (a, b, c) = spc.strand_graph()
    G = spc.DigraphGraph(dnodes)
    G.build_seed_index()
    reads = [a[200:1700], b[200:1700], c[200:1700], a[100:1900]]
    plan, found = spc.check_plan(G, [(did, len(seq)) for did, seq in dnodes], 0, reads, max_seeds=1)
    assert [s[2] for s in spc.rows(plan["seeds"])] == [spm.OK, spm.BAD_SEED, spm.ASSERTION, spm.OK]
    got, _ = spc.check_results(G, reads, max_seeds=1)
    assert [r["status"] for r in got] == [0, spm.BAD_SEED, spm.ASSERTION, 0]


def test_overlap_graph_gpu():
    nodes, edges, a = spc.overlap_graph(4)
    G = binding.Graph(nodes, edges, overlap=4)
    G.build_seed_index()
    reads = [a[300:1900], a[2300:3700]]
    plan, found = spc.check_plan(G, spm.bigraph_nodes(nodes), 4, reads, max_seeds=1)
    assert all(found.seeds)
    for i, (rd, sd) in enumerate(zip(reads, found.seeds)):
        p = sd[0][1]
        bw, fw = spc.rows(plan["jobs"])[2 * i], spc.rows(plan["jobs"])[2 * i + 1]
        assert bw[1] == spm.padded(p + 4) and bw[3] == p and fw[1] == spm.padded(len(rd) - p) and fw[3] == len(rd) - p - 4
    spc.check_results(G, reads, max_seeds=1)


def test_two_seeds_second_covered_by_the_first_gpu():
    g, reads = slc.repeat_case()
    G = binding.Graph(g.nodes, g.edges)
    G.build_seed_index()
    reads = [reads[0][:2600]]
    plan, found = spc.check_plan(G, spm.bigraph_nodes(g.nodes), 0, reads, max_seeds=2)
    assert len(found.seeds[0]) == 2 and len(plan["jobs"]) == 4
    got, _ = spc.check_results(G, reads, max_seeds=2)
    assert got[0]["status"] == 0 and not got[0]["failed"]


# ---- results ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loci", [False, True], ids=["hits", "loci"])
def test_results_equal_the_two_call_path_gpu(world, first_pass, loci):
    g, G, dnodes = world
    reads = synth.simulate_reads(g, 20, 1000, seed=5)[0]
    got, found = spc.check_results(G, reads, loci=loci)
    assert sum(1 for r in got if r["status"] == 0 and not r["failed"]) >= 18
    got, found = spc.check_results(G, sc.spiked_reads(g), loci=loci)
    assert [r["status"] for r, s in zip(got, found.seeds) if not s] == [spm.ASSERTION] * sum(1 for s in found.seeds if not s)


def test_results_with_trace_items_gpu(world, first_pass):
    g, G, dnodes = world
    reads = synth.simulate_reads(g, 5, 900, seed=15)[0]
    got, _ = spc.check_results(G, reads, flags=binding.GA_F_TRACE)
    assert all(len(r["trace"]) > 800 for r in got)


# ---- scale, threads, reruns ---------------------------------------------------------------------------------------------------------------
SUMMARY_FIELDS = ("status", "failed", "score", "n_mappings", "alignment_start", "alignment_end", "query_position")


def test_twenty_thousand_reads_in_one_call_gpu():
    """20 000 reads of 386 bp to 8 kb, reads without a seed shuffled in: the whole plan and all seeds against the two-call path; the
    per-read records of the run for a sample of 500 reads against the two-call path's over those reads"""
    g = synth.bubble_graph(1_000_000, node_len=32, seed=7)
    G = binding.Graph(gfa=g.gfa())
    G.build_seed_index()
    base = synth.simulate_reads(g, 2500, 8000, seed=3)[0]
    rng = np.random.default_rng(12)
    lengths = [386, 387, 8000, 700, 1500, 2600, 4100, 6000]
    reads = []
    for i, r in enumerate(base):
        for k, n in enumerate(lengths):
            n = min(len(r), n + int(rng.integers(0, 300)) if k > 2 else n)
            a = int(rng.integers(0, len(r) - n + 1))
            reads.append(r[a:a + n])
    alien = spc.text(synth.random_genome(3000, 5))
    for i in rng.integers(0, len(reads), size=200):
        reads[int(i)] = reads[int(i)][:300] if i % 2 else alien
    order = rng.permutation(len(reads))
    reads = [reads[int(i)] for i in order]
    assert len(reads) == 20000
    found = G.find_seeds(reads, loci=True)
    seeded = G.prepare_seeded(reads, None, True, 35)
    two = G.prepare(reads, found.seeds, 35)
    assert spc.plain_seeds(seeded.seeds()) == spc.plain_seeds(found)
    a, b = seeded.plan(), two.plan()
    two.close()
    for kind in ("jobs", "seeds", "fills"):
        assert len(a[kind]) == len(b[kind]) and all((a[kind][f] == b[kind][f]).all() for f in a[kind].dtype.names), kind
    st = seeded.prepare_stats()
    assert st["n_jobs"] == len(a["jobs"]) >= 30000 and st["reads_without_seed"] >= 150
    print("seeded prepare of 20 000 reads: %s" % st)
    seeded.run()
    big = seeded.collect(summary=True)
    seeded.close()
    sample = [int(i) for i in rng.choice(len(reads), size=500, replace=False)]
    small = G.prepare([reads[i] for i in sample], [found.seeds[i] for i in sample], 35)
    small.run()
    want = small.collect(summary=True)
    for f in SUMMARY_FIELDS:
        assert (big[f][sample] == want[f]).all(), f
    # (not vacuous: the two shortest length classes, a quarter of the reads, have 193-row directions that the engine may give up on, and one
    # read in a hundred has no seed; of the other classes, five eighths of the reads, most align: at least half the sample must)
    assert int((want["failed"] == 0).sum()) >= 250


def test_two_threads_prepare_on_one_graph_gpu(world):
    """two seeded batches prepared at the same time on one graph (the seeding engine's lock, the batches' own streams), then run and
    collected: each equals its two-call results"""
    g, G, dnodes = world
    sets = [synth.simulate_reads(g, 300, 1500, seed=61)[0], synth.simulate_reads(g, 200, 2500, seed=62)[0]]
    want = [G.align(rd, G.find_seeds(rd, loci=k == 1).seeds, 35) for k, rd in enumerate(sets)]
    for _ in range(3):
        batches, errors = [None, None], []
        gate = threading.Barrier(2)

        def work(k):
            try:
                gate.wait()
                batches[k] = G.prepare_seeded(sets[k], None, k == 1, 35)
            except Exception as e:                                        # noqa: BLE001
                errors.append(e)

        threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        for k in (1, 0):
            batches[k].run()
        for k in range(2):
            spc.same_results(batches[k].collect(), want[k])
            batches[k].close()


def test_a_seeded_batch_runs_twice_gpu(world):
    g, G, dnodes = world
    reads = spc.mixed_reads(g, 30, length=2000, seed=71)
    b = G.prepare_seeded(reads, None, True, 35)
    b.run()
    first = b.collect()
    b.run()
    spc.same_results(b.collect(), first)
    assert sum(1 for r in first if r["status"] == 0 and not r["failed"]) >= 28


def test_plan_kernels_have_no_private_segment():
    """the rows the build keeps for the library under test (build/kernel_resources.json, written with it): read, never rebuilt here"""
    import __graft_entry__ as entry
    assert os.path.exists(entry.RESOURCES_JSON), "no resource table: build() writes it next to the library"
    assert os.path.getmtime(entry.RESOURCES_JSON) + 600 >= os.path.getmtime(entry.PRODUCT_SO), "the resource table is older than the library"
    table = json.load(open(entry.RESOURCES_JSON))
    for name in ("ga_plan_first_bad_kernel", "ga_plan_slot_kernel", "ga_plan_write_kernel", "ga_eq_words_planned_kernel", "ga_eq_words_kernel"):
        assert name in table, name
        assert int(table[name]["ScratchSize [bytes/lane]"]) == 0 and int(table[name]["VGPRs Spill"]) == 0 and int(table[name]["SGPRs Spill"]) == 0, (name, table[name])
