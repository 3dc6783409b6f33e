"""Cases for GA_F_PATHSEQ, run on the GPU by tests/test_pathseq_gpu.py (the host emulation of the back end writes no path sequences, so
there is no host twin of these; the walk itself runs on the host in tests/test_pathseq.py).  Everywhere the expected value is
pathseq_model.oracle_path_seq: the oracle's raw cells and TraceItem list through oracle_binding.  The oracle's results are computed once
per process (parity_common's memo) and left unchanged.  No read of any case is skipped."""
import numpy as np

from graphaligner_amd import binding, synth
import ops_cases as oc
import ops_model as om
import oracle_binding as ob
import parity_cases as pcases
import parity_common as pc
import pathseq_model as psm
import wide_cases as wc

F_PATH = binding.GA_F_PATHSEQ
_COMPLEMENT = bytes.maketrans(b"ACGT", b"TGCA")


class ColumnBases:
    """base_at of pathseq_model.oracle_path_seq: the graph's base per column, from the node sequences the graph was made of and the
    library's column table (ga_graph_node_columns).  A digraph node holds the first `length` bases of its strand's sequence: all of
    them, or all but the overlap in a graph with overlaps (BigraphToDigraph.cpp:58-104)"""

    def __init__(self, gg, nodes):
        self.graph_bp = gg.bp
        self.table = bytearray(b"-" * gg.bp)
        for nid, seq in nodes:
            fw = seq.encode() if isinstance(seq, str) else bytes(seq)
            for strand, s in ((0, fw), (1, fw.translate(_COMPLEMENT)[::-1])):
                first, length = gg.node_columns(2 * int(nid) + strand)
                self.table[first:first + length] = s[:length]

    def __call__(self, column):
        return chr(self.table[column])


def run_path(gg, reads, seeds, bw, ramp=0, flags=F_PATH):
    b = gg.prepare(reads, seeds, bw, ramp, flags)
    b.run()
    return b.collect(), b


def compare_path(devs, oras, base_at, ctx):
    """everything the reference's result carries, and the path sequence of every read, against the oracle; returns the aligned reads"""
    assert len(devs) == len(oras)
    aligned = 0
    for i, (d, o) in enumerate(zip(devs, oras)):
        where = "%s read %d" % (ctx, i)
        pc.compare_read(d, pc.expected(o, trace=False), where)
        want, want_backward = psm.oracle_path_seq(o, base_at)
        assert (d["path_seq"], d["path_seq_backward"]) == (want, want_backward), (where, d["path_seq_backward"], want_backward, d["path_seq"][:60], want[:60], len(d["path_seq"]), len(want))
        aligned += int(o["status"] == 0 and not o["failed"])
    return aligned


def check_batch(nodes, edges, reads, seeds, bw, ramp=0, overlap=0, ctx=""):
    gg = binding.Graph(nodes, edges, overlap=overlap)
    devs, b = run_path(gg, reads, seeds, bw, ramp)
    oras = pc.oracle_results(nodes, edges, reads, seeds, bw, ramp, overlap)
    aligned = compare_path(devs, oras, ColumnBases(gg, nodes), ctx)
    st = b.path_seq_stats()
    assert st["reads_from_device"] + st["reads_from_host"] == aligned, (ctx, st, aligned)
    assert st["count_kernel_ms"] > 0 and st["write_kernel_ms"] > 0 and st["bases_written"] > 0 and st["moves_read"] >= st["bases_written"] - st["jobs_walked"], st
    return devs, oras, st


# ---- round edges -----------------------------------------------------------------------------------------------------------------
def round_edge_batch(node_len):
    """ops_cases' reads of 255 .. 321 bp, and reads with one base deleted or inserted at moves 63, 64 and 65 counted from either end"""
    g = synth.linear_graph(2000, node_len=node_len, seed=9)
    genome = g.genome.tobytes().decode()
    reads = [genome[:n] for n in oc.ROUND_LENGTHS]
    for p in (63, 64, 65, 321 - 65, 321 - 64, 321 - 63):
        other = "ACGT"[("ACGT".index(genome[p]) + 2) % 4]
        reads.append(genome[:p] + genome[p + 1:322])              # the graph has a base the read lacks: a deletion
        reads.append(genome[:p] + other + genome[p:320])          # the read has a base the graph lacks: an insertion
    return g, reads, [(int(g.node_at[0]), 0, False)] * len(reads)


def case_round_edges(node_len):
    g, reads, seeds = round_edge_batch(node_len)
    devs, oras, st = check_batch(g.nodes, g.edges, reads, seeds, 35, ctx="round edges, %d-bp nodes" % node_len)
    genome = g.genome.tobytes()
    for d, n in zip(devs, oc.ROUND_LENGTHS):
        assert d["path_seq"] == genome[:n] and d["path_seq_backward"] == 0
    types = set(int(t) for o in oras for t in o["trace"][:, 4])
    assert om.DELETION in types and om.INSERTION in types
    assert st["reads_from_host"] == 0 and st["reads_from_device"] == len(reads) and st["jobs_walked"] == len(reads)
    return st


def case_crossing_graphs(row):
    g, batches = oc.random_graph_batches(row, mid_only=False)
    aligned = 0
    for reads, seeds, bw, mid in batches[:2]:
        _, oras, _ = check_batch(g.nodes, g.edges, reads, seeds, bw, ctx="crossings %s bw %d" % (row, bw))
        aligned += sum(1 for o in oras if o["status"] == 0 and not o["failed"])
    assert aligned >= 12, aligned


def case_fan_in_degree():
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
        pre = noisy(np.concatenate([g.head, g.stem, g.branches[b], g.tails[b][:10]]))
        reads.append(pre + noisy(g.tails[b][10:]))
        seeds.append((3 + branches + b, len(pre), False))
    devs, oras, _ = check_batch(g.nodes, g.edges, reads, seeds, 35, ctx="fan of 10")
    assert all(o["status"] == 0 and not o["failed"] for o in oras)
    assert all(0 < d["path_seq_backward"] < len(d["path_seq"]) for d in devs[2:])


def case_both_parts(row):
    """mid-seed reads: n_backward lies inside the sequence, and the two pieces meet in the seed's node without being stitched"""
    g, batches = oc.random_graph_batches(row, mid_only=True)
    aligned = 0
    for reads, seeds, bw, _ in batches[:2]:
        devs, oras, st = check_batch(g.nodes, g.edges, reads, seeds, bw, ctx="both parts %s bw %d" % (row, bw))
        for d, o in zip(devs, oras):
            if o["status"] == 0 and not o["failed"]:
                assert len(o["bw_trace"]) and len(o["fw_trace"]) and 0 < d["path_seq_backward"] < len(d["path_seq"])
                aligned += 1
        assert st["reads_from_host"] == 0, st
    assert aligned >= 10, aligned


def case_one_part_and_strands():
    g = synth.bubble_graph(20000, node_len=32, seed=31)
    reads, seeds = synth.simulate_reads(g, 8, 900, seed=12, both_strands=True, mid_seed=True)
    more, mseeds = synth.simulate_reads(g, 8, 900, seed=13, both_strands=True)
    genome = g.genome.tobytes().decode()
    last = genome[3000:3700]
    reads = reads + more + [last]
    seeds = seeds + mseeds + [(int(g.node_at[3699]), len(last) - 1, False)]
    devs, oras, _ = check_batch(g.nodes, g.edges, reads, seeds, 35, ctx="one part, both strands")
    assert any(s[2] for s in seeds)
    assert all(d["path_seq_backward"] == 0 and d["path_seq"] for d in devs[8:16])
    assert devs[-1]["path_seq"] and devs[-1]["path_seq_backward"] == len(devs[-1]["path_seq"])


def case_gfa_overlap():
    """ops_cases.case_gfa_overlap's graph with overlap 15: the two strands' nodes are cut differently, so a backward part's bases are
    the mirror node's own (the twin table), not complements"""
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
    gg = binding.Graph(gfa=gfa)
    devs, _ = run_path(gg, reads, seeds, 35)
    og = ob.OracleGraph.from_gfa_segments(segs, links, k)
    oras = [og.align(r, [sd], 35) for r, sd in zip(reads, seeds)]
    aligned = compare_path(devs, oras, ColumnBases(gg, segs), "gfa overlap %d" % k)
    assert aligned >= 5 and any(d["path_seq_backward"] > 0 for d in devs), aligned


def case_self_loop():
    nodes, edges, reads, seeds = oc.self_loop_batch()
    devs, oras, _ = check_batch(nodes, edges, reads, seeds, 35, ctx="one-base self-loop")
    a, b = nodes[0][1], nodes[2][1]
    # a base per turn of the loop: the one-base node's T comes back once per turn the alignment takes (ops_cases.case_self_loop: two at least)
    assert all(a.encode()[-20:] + b"TT" in d["path_seq"] for d in devs)


def case_cyclic():
    node_len, bw, back_edges, self_loops, max_span = pcases.CYCLIC_GRAPHS[1]
    g = synth.cyclic_graph(5000, node_len=node_len, seed=node_len + bw, back_edges=back_edges, self_loops=self_loops, max_span=max_span)
    reads, seeds = synth.walk_reads(g, 8, 900, seed=900 + node_len, mid_seed=True, first_nodes=max(1, len(g.nodes) // 3))
    _, oras, _ = check_batch(g.nodes, g.edges, reads, seeds, bw, ctx="cyclic")
    assert sum(1 for o in oras if o["status"] == 0 and not o["failed"]) >= 4


def case_ramp():
    node_len, bw, ramp, err = pcases.RAMP_CASES[0]
    rng = np.random.default_rng(node_len * 7 + bw)
    g = synth.SynthGraph(synth.random_genome(30000, 900 + node_len), node_len=node_len, snp_every=60, indel_every=400, seed=node_len)
    reads, seeds = synth.simulate_reads(g, 8, 1500, sub=err, ins=err, dele=err, seed=1500 + bw, mid_seed=False)
    reads = pcases.damaged_reads(reads, rng)
    _, oras, _ = check_batch(g.nodes, g.edges, reads, seeds, bw, ramp=ramp, ctx="ramp")
    assert sum(1 for o in oras if o["status"] == 0 and not o["failed"]) >= 4


def case_wide():
    branches, branch_len, shared, tail_len, bw, ramp, cyclic = wc.CASES["300x64"]
    nodes, edges, reads, seeds = wc.fan_batch(branches, branch_len, shared, tail_len, cyclic)
    _, oras, _ = check_batch(nodes, edges, reads, seeds, bw, ramp=ramp, ctx="300 branches")
    assert all(o["status"] == 0 for o in oras)


def case_several_seeds():
    g = synth.bubble_graph(30000, node_len=32, seed=23)
    reads, seeds = synth.simulate_reads(g, 6, 1500, seed=4)
    other, oseeds = synth.simulate_reads(g, 6, 1500, seed=40, mid_seed=True)
    multi = [[s, (o[0], 700, o[2]), s, (s[0], 0, not s[2])] for s, o in zip(seeds, oseeds)]
    reads = list(reads) + [reads[0]]
    multi.append([(10 ** 6, 0, False)])
    devs, oras, _ = check_batch(g.nodes, g.edges, reads, multi, 35, ctx="several seeds")
    assert oras[-1]["status"] != 0 and devs[-1]["path_seq"] == b"" and devs[-1]["path_seq_backward"] == 0


def case_many_jobs_one_wave():
    """257 reads on one wave, run twice: the same bytes both times, and the oracle's"""
    g, reads, seeds = oc.many_jobs_batch()
    assert len(reads) == 257
    gg = binding.Graph(g.nodes, g.edges)
    b = gg.prepare(reads, seeds, 35, 0, F_PATH)
    oras = pc.oracle_results(g.nodes, g.edges, reads, seeds, 35)
    base_at = ColumnBases(gg, g.nodes)
    runs = []
    for again in range(2):
        b.run()
        devs = b.collect()
        assert compare_path(devs, oras, base_at, "257 reads on one wave, run %d" % again) >= 200
        runs.append([(d["path_seq"], d["path_seq_backward"]) for d in devs])
    assert runs[0] == runs[1]
    return b.path_seq_stats()


def case_seeded_batch_equals_two_calls(g, reads, min_aligned):
    gg = binding.Graph(g.nodes, g.edges)
    gg.build_seed_index()
    one = gg.align_reads(reads, flags=F_PATH)
    found = gg.find_seeds(reads)
    two = gg.align(reads, found.seeds, 35, 0, F_PATH)
    oras = pc.oracle_results(g.nodes, g.edges, reads, [list(s) for s in found.seeds], 35)
    assert compare_path(one, oras, ColumnBases(gg, g.nodes), "seeded batch") >= min_aligned
    for a, b in zip(one, two):
        assert a["path_seq"] == b["path_seq"] and a["path_seq_backward"] == b["path_seq_backward"]


def _mid_seed_batch():
    g, batches = oc.random_graph_batches(pcases.RANDOM_GRAPHS[1], mid_only=True)
    reads, seeds, bw, _ = batches[0]
    return g, reads, seeds, bw


def case_all_flags_together():
    """GA_F_OPS | GA_F_PILEUP | GA_F_PATHSEQ: runs and pileup equal those of a batch without the new flag, bases those of one with it alone"""
    g, reads, seeds, bw = _mid_seed_batch()
    gg = binding.Graph(g.nodes, g.edges)
    old = binding.GA_F_OPS | binding.GA_F_PILEUP
    results, piles = {}, {}
    for flags in (old, old | F_PATH, F_PATH):
        devs, b = run_path(gg, reads, seeds, bw, flags=flags)
        results[flags] = devs
        if flags & binding.GA_F_PILEUP:
            piles[flags] = gg.pileup("bases")
            piles[flags].add(b)
    for a, c, p in zip(results[old], results[old | F_PATH], results[F_PATH]):
        assert "path_seq" not in a
        assert om.as_pairs(a["ops"]) == om.as_pairs(c["ops"]) and a["op_counts"] == c["op_counts"]
        assert (c["path_seq"], c["path_seq_backward"]) == (p["path_seq"], p["path_seq_backward"])
    assert (piles[old].counts() == piles[old | F_PATH].counts()).all() and piles[old].counts().sum() > 0
    oras = pc.oracle_results(g.nodes, g.edges, reads, seeds, bw)
    assert compare_path(results[old | F_PATH], oras, ColumnBases(gg, g.nodes), "all flags") >= 6


def case_flag_changes_nothing_else():
    import ctypes as C
    g, reads, seeds, bw = _mid_seed_batch()
    gg = binding.Graph(g.nodes, g.edges)
    plain, b0 = run_path(gg, reads, seeds, bw, flags=0)
    flagged, b1 = run_path(gg, reads, seeds, bw)
    assert b0.stats()["reserved"] == b1.stats()["reserved"] == 0
    for a, f in zip(plain, flagged):
        assert "path_seq" not in a and "ops" not in f
        for key in ("status", "failed", "score", "alignment_start", "alignment_end", "query_position", "mappings", "columns"):
            assert a[key] == f[key], key
        assert f["trace"].shape[0] == 0
    # without the flag: the three fields are NULL / 0 and the statistics are refused
    out = C.POINTER(binding.GaResultsPathSeq)()
    assert b0.L.ga_batch_collect(b0.h, C.byref(out)) == 0
    try:
        assert not out.contents.read_path_seq and not out.contents.path_bases and out.contents.n_path_bases == 0
    finally:
        b0.L.ga_results_free(out)
    assert b0.L.ga_batch_path_seq_stats(b0.h, C.byref(binding.GaBatchPathSeqStats())) == 100


def case_unsplit():
    """a linear GFA of long segments cut into 64-bp pieces: ga_results_unsplit carries the bases over unchanged, and they are the oracle's
    on the same pieces given as an ordinary graph"""
    import test_gfa_split as tgs
    segs, gfa = tgs._long_segment_gfa(3, 5000, 81)
    nodes, edges = tgs._pieces_graph(segs, 64, 3)
    rng = np.random.default_rng(82)
    per_seg, nxt = {}, 4
    for i, s in enumerate(segs):
        per_seg[i] = [i + 1] + list(range(nxt, nxt + (len(s) - 1) // 64))
        nxt += (len(s) - 1) // 64
    reads, seeds = [], []
    for k in range(4):
        seg = int(rng.integers(0, 3))
        start = int(rng.integers(64, 5000 - 1300)) // 64 * 64
        body = np.frombuffer(segs[seg][start:start + 1200].encode(), dtype=np.uint8)
        reads.append(synth.add_errors(body, 0.03, 0.03, 0.03, rng).tobytes().decode())
        # a seed at the first base, and one 640 bases in (both parts)
        seeds.append((per_seg[seg][start // 64], 0, False) if k % 2 == 0 else (per_seg[seg][start // 64 + 10], 640, False))
    split = binding.Graph(gfa=gfa, split=64)
    b = split.prepare(reads, seeds, 35, 0, F_PATH)
    b.run()
    pieces, merged = b.collect(), b.collect(unsplit=True)
    oras = pc.oracle_results(nodes, edges, reads, seeds, 35)
    assert compare_path(pieces, oras, ColumnBases(split, nodes), "split graph") == len(reads)
    for x, m in zip(pieces, merged):
        assert x["path_seq"] and (m["path_seq"], m["path_seq_backward"]) == (x["path_seq"], x["path_seq_backward"])
        assert len(m["mappings"]) < len(x["mappings"])
    assert any(m["path_seq_backward"] > 0 for m in merged)


# ---- without the oracle ----------------------------------------------------------------------------------------------------------
def case_ops_and_path_walked_together():
    """ACGT-only reads with GA_F_OPS | GA_F_PATHSEQ, part by part: the bases number matches + mismatches + deletions + one per part
    (no part of these reads starts on a dummy node); at every MATCH the path base is the read's, at every MISMATCH it is not"""
    g = synth.bubble_graph(30000, node_len=32, seed=23)
    reads, seeds = synth.simulate_reads(g, 6, 1500, seed=4)
    more, mseeds = synth.simulate_reads(g, 6, 1500, seed=40, mid_seed=True)
    reads, seeds = list(reads) + list(more), list(seeds) + list(mseeds)
    assert all(set(r) <= set("ACGT") for r in reads)
    gg = binding.Graph(g.nodes, g.edges)
    devs, b = run_path(gg, reads, seeds, 35, flags=binding.GA_F_OPS | F_PATH)
    checked = 0
    for i, (d, read, seed) in enumerate(zip(devs, reads, seeds)):
        assert d["status"] == 0 and not d["failed"], i
        runs = om.as_pairs(d["ops"])
        cut = [k for k, (t, _) in enumerate(runs) if t == om.SPLIT]
        path, nb = d["path_seq"], d["path_seq_backward"]
        if cut:
            parts = [(runs[:cut[0]], path[:nb], d["alignment_start"]), (runs[cut[0] + 1:], path[nb:], seed[1])]
        else:
            assert seed[1] == 0 and nb == 0, (i, "a read with one part whose seed is not at its first base")
            parts = [(runs, path, 0)]
        m, x, ins, dele = om.counts_of(runs)
        assert len(path) == m + x + dele + len(parts), (i, len(path), m, x, dele, len(parts))
        for part_runs, part_path, row in parts:
            j = 0                                    # (c_0: a base of its own, no item)
            for t, n in part_runs:
                for _ in range(n):
                    if t in (om.MATCH, om.MISMATCH):
                        j += 1
                        row += 1
                        assert (chr(part_path[j]) == read[row]) == (t == om.MATCH), (i, j, row, t)
                    elif t == om.INSERTION:
                        row += 1
                    else:
                        j += 1
            assert j == len(part_path) - 1, (i, j, len(part_path))
        checked += 1
    assert checked == len(reads) and sum(1 for d in devs if d["path_seq_backward"] > 0) >= 5
