"""Cases for GA_F_OPS shared by tests/test_ops.py (host build of the operations program, tests/emul) and tests/test_ops_gpu.py (the
product on the GPU).  Everywhere the expected value is ops_model.rle(oracle trace types): the oracle's TraceItem list through
oracle_binding, cut into runs by ops_model.  The oracle's results are computed once per process (parity_common's memo) and left unchanged."""
import random

import numpy as np

from graphaligner_amd import binding, synth
import alphabet_cases as ac
import oracle_binding as ob
import ops_model as om
import parity_cases as pcases
import parity_common as pc
import wide_cases as wc

F_OPS = binding.GA_F_OPS


def run_ops(nodes, edges, reads, seeds, bw, ramp=0, overlap=0, lib_path=None, flags=F_OPS, gfa=None):
    """one batch through the staged calls -> (results, ga_batch_ops_stats or None, ga_batch_stats)"""
    g = binding.Graph(gfa=gfa, lib_path=lib_path) if gfa is not None else binding.Graph(nodes, edges, overlap=overlap, lib_path=lib_path)
    b = g.prepare(reads, seeds, bw, ramp, flags)
    b.run()
    devs = b.collect()
    return devs, (b.ops_stats() if flags & F_OPS else None), b.stats()


def compare_ops(devs, oras, ctx):
    """status, failed and runs of every read against the oracle; returns the number of aligned reads"""
    assert len(devs) == len(oras)
    aligned = 0
    for i, (d, o) in enumerate(zip(devs, oras)):
        where = "%s read %d" % (ctx, i)
        assert d["status"] == o["status"], (where, "status", d["status"], o["status"], o["message"])
        assert d["failed"] == o["failed"], (where, "failed")
        want = om.oracle_ops(o)
        got = om.as_pairs(d["ops"])
        assert got == want, (where, "runs", binding.ops_string(got), binding.ops_string(want))
        c = d["op_counts"]
        assert (c["match"], c["mismatch"], c["insertion"], c["deletion"]) == om.counts_of(want), (where, "counts", c)
        aligned += int(o["status"] == 0 and not o["failed"])
    return aligned


def check_batch(nodes, edges, reads, seeds, bw, ramp=0, overlap=0, lib_path=None, ctx=""):
    devs, st, _ = run_ops(nodes, edges, reads, seeds, bw, ramp, overlap, lib_path)
    oras = pc.oracle_results(nodes, edges, reads, seeds, bw, ramp, overlap)
    aligned = compare_ops(devs, oras, ctx)
    assert st["reads_from_device"] + st["reads_from_host"] == aligned, (ctx, st, aligned)
    return devs, oras, st


# ---- 1 and 2: round edges, crossings -------------------------------------------------------------------------------------------
ROUND_LENGTHS = (255, 256, 257, 320, 321)
ROUND_SUBSTITUTIONS = (63, 64, 65, 256, 257)
ROUND_EXPECTED = ["254=", "255=", "256=", "319=", "320=", "62=1X257=", "63=1X256=", "64=1X255=", "255=1X64=", "256=1X63="]


def round_edge_batch(node_len):
    g = synth.linear_graph(2000, node_len=node_len, seed=9)
    genome = g.genome.tobytes().decode()
    reads = [genome[:n] for n in ROUND_LENGTHS]
    for p in ROUND_SUBSTITUTIONS:
        r = list(genome[:321])
        r[p] = "ACGT"[("ACGT".index(r[p]) + 1) % 4]
        reads.append("".join(r))
    seeds = [(int(g.node_at[0]), 0, False)] * len(reads)
    return g, reads, seeds


def case_round_edges(node_len, lib_path=None):
    g, reads, seeds = round_edge_batch(node_len)
    devs, oras, st = check_batch(g.nodes, g.edges, reads, seeds, 35, lib_path=lib_path, ctx="round edges, %d-bp nodes" % node_len)
    assert [binding.ops_string(om.oracle_ops(o)) for o in oras] == ROUND_EXPECTED
    assert [binding.ops_string(d["ops"]) for d in devs] == ROUND_EXPECTED
    assert st["reads_from_host"] == 0 and st["reads_from_device"] == len(reads)
    return st


def random_graph_batches(row, mid_only):
    """the batches of parity_cases.case_random_graphs for one row of RANDOM_GRAPHS: (graph, [(reads, seeds, bw, mid)])"""
    node_len, snp, indel, sv = row
    rng = np.random.default_rng(node_len * 1000 + snp)
    g = synth.SynthGraph(synth.random_genome(25000, 500 + node_len), node_len=node_len, snp_every=snp, indel_every=indel, sv_every=sv, seed=node_len)
    out = []
    for bw, err, length, mid in [(35, 0.04, 2500, False), (35, 0.04, 2500, True), (10, 0.02, 1000, False), (64, 0.1, 1500, True), (2, 0.0, 700, False)]:
        reads, seeds = synth.simulate_reads(g, 12, length, sub=err, ins=err, dele=err, seed=int(rng.integers(1 << 30)), mid_seed=mid)
        if mid or not mid_only:
            out.append((reads, seeds, bw, mid))
    return g, out


def case_crossing_graphs(row, lib_path=None):
    """short nodes with in-degrees 2 and 3: the first two batches of the row (seed at the start, seed in the middle)"""
    g, batches = random_graph_batches(row, mid_only=False)
    aligned = 0
    for reads, seeds, bw, mid in batches[:2]:
        _, oras, _ = check_batch(g.nodes, g.edges, reads, seeds, bw, lib_path=lib_path, ctx="crossings %s bw %d" % (row, bw))
        aligned += sum(1 for o in oras if o["status"] == 0 and not o["failed"])
    assert aligned >= 12, aligned


# ---- 3: in-degree above four -----------------------------------------------------------------------------------------------------
def case_fan_in_degree(lib_path=None):
    branches = 10
    g = synth.FanGraph(head_len=300, stem_len=600, n_branches=branches, branch_len=48, shared=16, tail_len=300, seed=5)
    rng = np.random.default_rng(77)
    noisy = lambda a: synth.add_errors(a, 0.03, 0.03, 0.03, rng).tobytes().decode()
    b = branches - 1
    reads, seeds = [], []
    for _ in range(2):
        reads.append(noisy(np.concatenate([g.head, g.stem, g.branches[b], g.tails[b]])))
        seeds.append((1, 0, False))
    for _ in range(2):
        # seeded in the tail: the backward part walks the other strand, where the stem has every branch as in-neighbour
        pre = noisy(np.concatenate([g.head, g.stem, g.branches[b], g.tails[b][:10]]))
        reads.append(pre + noisy(g.tails[b][10:]))
        seeds.append((3 + branches + b, len(pre), False))
    devs, oras, st = check_batch(g.nodes, g.edges, reads, seeds, 35, lib_path=lib_path, ctx="fan of 10")
    assert all(o["status"] == 0 and not o["failed"] for o in oras)
    assert all(sum(1 for t, _ in om.oracle_ops(o) if t == om.SPLIT) == 1 for o in oras[2:])
    return st


# ---- 4: both parts ---------------------------------------------------------------------------------------------------------------
def case_both_parts(row, lib_path=None):
    g, batches = random_graph_batches(row, mid_only=True)
    aligned = 0
    for reads, seeds, bw, _ in batches:
        devs, st, _ = run_ops(g.nodes, g.edges, reads, seeds, bw, lib_path=lib_path)
        oras = pc.oracle_results(g.nodes, g.edges, reads, seeds, bw)
        for o in oras:
            if o["status"] == 0 and not o["failed"]:
                assert sum(1 for t in o["trace"][:, 4] if t == om.SPLIT) == 1, "a mid-seed read with one part only"
        assert st["reads_from_host"] == 0, st
        aligned += compare_ops(devs, oras, "both parts %s bw %d" % (row, bw))
    assert aligned >= 20, aligned
    return aligned


def case_one_part_and_strands(lib_path=None):
    """a seed at the last base (backward part only), at the first base, and reads of the reverse strand"""
    g = synth.bubble_graph(20000, node_len=32, seed=31)
    reads, seeds = synth.simulate_reads(g, 8, 900, seed=12, both_strands=True, mid_seed=True)
    more, mseeds = synth.simulate_reads(g, 8, 900, seed=13, both_strands=True)
    genome = g.genome.tobytes().decode()
    last = genome[3000:3700]
    reads = reads + more + [last]
    seeds = seeds + mseeds + [(int(g.node_at[3699]), len(last) - 1, False)]
    devs, oras, st = check_batch(g.nodes, g.edges, reads, seeds, 35, lib_path=lib_path, ctx="one part, both strands")
    assert any(s[2] for s in seeds)
    last_runs = om.oracle_ops(oras[-1])
    assert last_runs and all(t != om.SPLIT for t, _ in last_runs)
    return st


def case_gfa_overlap(lib_path=None):
    """parity_cases.case_gfa_overlap's graph with overlap 15: trace_rows < n in every job"""
    rng = np.random.default_rng(3)
    k, node_len = 15, 60
    gs = synth.random_genome(20000, 70 + k).tobytes().decode()
    step = node_len - k
    segs = []
    i, nid = 0, 1
    while i + node_len <= len(gs):
        segs.append((nid, gs[i:i + node_len]))
        i += step
        nid += 1
    links = [(segs[a][0], False, segs[a + 1][0], False) for a in range(len(segs) - 1)]
    gfa = "H\tVN:Z:1.0\n" + "".join("S\t%d\t%s\n" % x for x in segs) + "".join("L\t%d\t+\t%d\t+\t%dM\n" % (f, t, k) for f, _, t, _ in links)
    noisy = lambda a, b: synth.add_errors(np.frombuffer(gs[a:b].encode(), dtype=np.uint8), 0.03, 0.03, 0.03, rng).tobytes().decode()
    reads, seeds = [], []
    for t in range(6):
        a = int(rng.integers(5, len(segs) - 40))
        if t % 2 == 0:
            reads.append(noisy(a * step, a * step + 1200))
            seeds.append((segs[a][0], 0, False))
        else:
            b = a + 10
            pre = noisy(a * step, b * step)
            reads.append(pre + noisy(b * step, b * step + 700))
            seeds.append((segs[b][0], len(pre), False))
    devs, st, _ = run_ops(None, None, reads, seeds, 35, lib_path=lib_path, gfa=gfa)
    og = ob.OracleGraph.from_gfa_segments(segs, links, k)
    oras = [og.align(r, [sd], 35) for r, sd in zip(reads, seeds)]
    aligned = compare_ops(devs, oras, "gfa overlap %d" % k)
    assert aligned >= 5, aligned
    return st


# ---- 5: the one-base self-loop ---------------------------------------------------------------------------------------------------
def self_loop_batch():
    random.seed(3)
    a = "".join(random.choice("ACGT") for _ in range(300))
    b = "".join(random.choice("ACGT") for _ in range(300))
    nodes = [(1, a), (2, "T"), (3, b)]
    edges = [(1, False, 2, False), (2, False, 2, False), (2, False, 3, False)]
    reads = [a + "TTT" + b, a + "TTTTTT" + b]
    return nodes, edges, reads, [(1, 0, False)] * 2


def case_self_loop(lib_path=None):
    nodes, edges, reads, seeds = self_loop_batch()
    oras = pc.oracle_results(nodes, edges, reads, seeds, 35)
    on_loop = []
    for o in oras:
        t = o["trace"]
        hit = [(int(t[i, 0]) == 2 and int(t[i, 1]) == 0 and int(t[i, 4]) == 1) for i in range(len(t))]
        best = run = 0
        for h in hit:
            run = run + 1 if h else 0
            best = max(best, run)
        on_loop.append(best)
    assert all(n >= 2 for n in on_loop), on_loop
    devs, oras, st = check_batch(nodes, edges, reads, seeds, 35, lib_path=lib_path, ctx="one-base self-loop")
    # (the reads run to the graph's end: the list's tail is insertions with single matches between them, cells past the last node)
    assert all(any(t == om.INSERTION for t, _ in om.oracle_ops(o)[-4:]) for o in oras), [binding.ops_string(om.oracle_ops(o)) for o in oras]
    return st


# ---- 6: alphabet -----------------------------------------------------------------------------------------------------------------
def case_alphabet(name, probes, lib_path=None):
    """alphabet_cases' reads: IUPAC and lower-case characters decide MATCH or MISMATCH on the device, a read with a character outside
    IUPAC takes the host path; status and runs equal the oracle's either way"""
    g = ac.graph(name)
    probes = [p for p in probes if ac.reaches_oracle(p)]
    reads = [ac.read_of(g, p) for p in probes]
    seeds = [[ac.seed_of(g, p[1])] for p in probes]
    devs, st, _ = run_ops(g.nodes, g.edges, reads, seeds, ac.BW, lib_path=lib_path)
    oras = [ac.oracle_of(name, p) for p in probes]
    aligned = compare_ops(devs, oras, "alphabet %s" % name)
    # the reads with a byte outside IUPAC that got as far as the item pass were decided there, and so were the reads whose short
    # backward part kept no slice (their forward part stays unshifted); the rest, the great majority, have the kernels' runs
    assert 0 < st["reads_from_host"] < st["reads_from_device"], st
    assert st["reads_from_device"] + st["reads_from_host"] >= aligned
    return st


# ---- 7: ladder jobs --------------------------------------------------------------------------------------------------------------
def case_cyclic(lib_path=None):
    node_len, bw, back_edges, self_loops, max_span = pcases.CYCLIC_GRAPHS[1]
    g = synth.cyclic_graph(5000, node_len=node_len, seed=node_len + bw, back_edges=back_edges, self_loops=self_loops, max_span=max_span)
    reads, seeds = synth.walk_reads(g, 8, 900, seed=900 + node_len, mid_seed=True, first_nodes=max(1, len(g.nodes) // 3))
    devs, oras, st = check_batch(g.nodes, g.edges, reads, seeds, bw, lib_path=lib_path, ctx="cyclic")
    assert sum(1 for o in oras if o["status"] == 0 and not o["failed"]) >= 4
    return st


def case_ramp(lib_path=None):
    node_len, bw, ramp, err = pcases.RAMP_CASES[0]
    rng = np.random.default_rng(node_len * 7 + bw)
    g = synth.SynthGraph(synth.random_genome(30000, 900 + node_len), node_len=node_len, snp_every=60, indel_every=400, seed=node_len)
    reads, seeds = synth.simulate_reads(g, 8, 1500, sub=err, ins=err, dele=err, seed=1500 + bw, mid_seed=False)
    reads = pcases.damaged_reads(reads, rng)
    devs, oras, st = check_batch(g.nodes, g.edges, reads, seeds, bw, ramp=ramp, lib_path=lib_path, ctx="ramp")
    assert sum(1 for o in oras if o["status"] == 0 and not o["failed"]) >= 4
    return st


def case_wide(lib_path=None):
    branches, branch_len, shared, tail_len, bw, ramp, cyclic = wc.CASES["300x64"]
    nodes, edges, reads, seeds = wc.fan_batch(branches, branch_len, shared, tail_len, cyclic)
    devs, oras, st = check_batch(nodes, edges, reads, seeds, bw, ramp=ramp, lib_path=lib_path, ctx="300 branches")
    assert all(o["status"] == 0 for o in oras)
    return st


# ---- 8: several seeds ------------------------------------------------------------------------------------------------------------
def case_several_seeds(lib_path=None):
    g = synth.bubble_graph(30000, node_len=32, seed=23)
    reads, seeds = synth.simulate_reads(g, 6, 1500, seed=4)
    other, oseeds = synth.simulate_reads(g, 6, 1500, seed=40, mid_seed=True)
    multi = [[s, (o[0], 700, o[2]), s, (s[0], 0, not s[2])] for s, o in zip(seeds, oseeds)]
    # a read that fails: a seed on a node the read has nothing to do with gives no alignment, or an unknown node a bad seed
    reads = list(reads) + [reads[0]]
    multi.append([(10 ** 6, 0, False)])
    devs, oras, st = check_batch(g.nodes, g.edges, reads, multi, 35, lib_path=lib_path, ctx="several seeds")
    assert oras[-1]["status"] != 0 and len(devs[-1]["ops"]) == 0
    return st


# ---- 9: one wave, many jobs ------------------------------------------------------------------------------------------------------
def many_jobs_batch():
    g = synth.bubble_graph(20000, node_len=32, seed=57)
    reads, seeds = synth.simulate_reads(g, 129, 260, seed=8, mid_seed=False)
    more, mseeds = synth.simulate_reads(g, 128, 420, seed=9, mid_seed=True, min_part=200)
    return g, reads + more, seeds + mseeds


def case_many_jobs_one_wave(lib_path=None):
    g, reads, seeds = many_jobs_batch()
    assert len(reads) == 257
    gg = binding.Graph(g.nodes, g.edges, lib_path=lib_path)
    b = gg.prepare(reads, seeds, 35, 0, F_OPS)
    oras = pc.oracle_results(g.nodes, g.edges, reads, seeds, 35)
    for again in range(2):
        b.run()
        devs = b.collect()
        aligned = compare_ops(devs, oras, "257 reads on one wave, run %d" % again)
        assert aligned >= 200, aligned
    return b.ops_stats()


# ---- 11: the flag alone changes nothing else -------------------------------------------------------------------------------------
def case_flag_changes_nothing_else(lib_path=None):
    g, batches = random_graph_batches(pcases.RANDOM_GRAPHS[1], mid_only=True)
    reads, seeds, bw, _ = batches[0]
    plain, none, st0 = run_ops(g.nodes, g.edges, reads, seeds, bw, lib_path=lib_path, flags=0)
    flagged, st, st1 = run_ops(g.nodes, g.edges, reads, seeds, bw, lib_path=lib_path)
    both, _, _ = run_ops(g.nodes, g.edges, reads, seeds, bw, lib_path=lib_path, flags=F_OPS | binding.GA_F_TRACE)
    assert none is None and st1["reserved"] == 0
    for a, f, t in zip(plain, flagged, both):
        assert "ops" not in a
        for key in ("status", "failed", "score", "alignment_start", "alignment_end", "query_position", "mappings", "columns"):
            assert a[key] == f[key] == t[key], key
        assert f["trace"].shape[0] == 0
        own = om.rle([int(x) for x in t["trace"][:, 4]])
        assert om.as_pairs(t["ops"]) == own == om.as_pairs(f["ops"])
    # without the flag: no ops in the results, and the statistics are refused
    gg = binding.Graph(g.nodes, g.edges, lib_path=lib_path)
    b = gg.prepare(reads, seeds, bw, 0, 0)
    b.run()
    import ctypes as C
    out = C.POINTER(binding.GaResultsOps)()
    assert b.L.ga_batch_collect(b.h, C.byref(out)) == 0
    try:
        assert not out.contents.read_ops and not out.contents.ops and out.contents.n_ops == 0
    finally:
        b.L.ga_results_free(out)
    stats = binding.GaBatchOpsStats()
    assert b.L.ga_batch_ops_stats(b.h, C.byref(stats)) == 100
    return st


# ---- a seeded batch against the two calls ----------------------------------------------------------------------------------------------
def case_seeded_batch_equals_two_calls(g, reads, min_aligned, lib_path=None):
    """align_reads(..., flags=GA_F_OPS) equals prepare(reads, find_seeds(reads)) with the flag, run for run, and both the oracle"""
    gg = binding.Graph(g.nodes, g.edges, lib_path=lib_path)
    gg.build_seed_index()
    one = gg.align_reads(reads, flags=binding.GA_F_OPS)
    found = gg.find_seeds(reads)
    two = gg.align(reads, found.seeds, 35, 0, binding.GA_F_OPS)
    oras = pc.oracle_results(g.nodes, g.edges, reads, [list(s) for s in found.seeds], 35)
    aligned = compare_ops(one, oras, "seeded batch")
    assert aligned >= min_aligned, aligned
    for a, b in zip(one, two):
        assert om.as_pairs(a["ops"]) == om.as_pairs(b["ops"]) and a["op_counts"] == b["op_counts"]
