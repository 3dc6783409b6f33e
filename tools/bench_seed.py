"""Seeding measured next to the aligner it feeds: the headline workload of bench.py (E. coli-scale linear graph of 64-bp nodes,
50 000 x 10 kb reads at ONT error) or the bubble graph.  One JSON line on stdout.

Reported: index build time and size; the ga_find_seeds kernel time per batch (HIP events inside the library; warm-up calls, then
timed calls: median, min, max); reads without a seed; the aligner's kernel_ms for the SAME batch from the reads' true seeds, and the
ratio of the two, which must stay below 1 (in the overlapped pipeline seeding is a stage in front of the
kernels).  The aligner from the seeds found here is reported beside it: those seeds lie inside the reads, so every read is two
extensions where the benchmark's true seeds (first base of the read) make one -- its rate is not comparable with README.md's figures.

    python tools/bench_seed.py --graph linear
    python tools/bench_seed.py --graph bubbles --reads 50000 --read-len 10000
    python tools/bench_seed.py --graph bubbles --node-len 8 --max-walks 64

--max-walks N (1..256): the walk index (k-mers across edges; graphs of nodes shorter than k need it, --node-len goes down to 8).  The
in-node index of the same graph is built and timed first, in the same call ("in_node": its size, build time and ga_find_seeds kernel
time); everything else in the row is then the walk index's, with its walk statistics.

--loci: one seed per locus (ga_find_seeds_loci) measured beside ga_find_seeds on the same batch and index, the timed calls of the two
alternating: "loci" holds the grouped kernel's time, its seeds, the jobs and the aligner's kernel_ms from them, its ratio to the
aligner's kernel_ms from true seeds, and the two sums seeding kernel + aligner kernels, grouped and ungrouped, with the saving and the
min-max spreads it has to exceed.

--coord topology: the topology coordinate (ga_graph_set_seed_coordinate) measured beside the file-order one on the same batch and
index, the coordinate switched before every timed call so that the two alternate call by call: "coord" holds the coordinate's build
time next to the index build's, its rounds, and under either coordinate the ga_find_seeds_loci kernel time, seeds, jobs and the
aligner's kernel_ms from those seeds.  --shuffle-nodes: the graph's nodes in a random order (random.Random(1).shuffle), edges as they
are: the file that is not in path order.

--seeded: seeded batches (ga_batch_prepare_seeded) measured beside the two-call path on the same reads and index, at the C ABI (no
Python lists in between): wall time of ga_find_seeds_loci + ga_batch_prepare against wall time of ga_batch_prepare_seeded, alternating
call by call (--warmup calls, then --calls timed ones, at least 10), with the seeded call's split (ga_batch_prepare_stats_t); then
the host-to-host rate of sharding.run_overlapped over 12 chunks of the reads, the stage in front of the kernels being the two calls
or the one, alternating run by run.  The row says whether either difference exceeds the larger of the two min-max spreads.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def seeded_row(args, G, reads, gen_s):
    """--seeded: see the module's text"""
    import ctypes as C
    import numpy as np
    from graphaligner_amd import binding, sharding
    L = G.L
    st = G.build_seed_index()
    p = G._seed_params(None, "bench_seed")
    rs = binding.ReadSet(reads, [[]] * len(reads))
    n = rs.n_reads

    def two_call(r=rs):
        """ga_find_seeds_loci, then ga_batch_prepare on the set's own arrays; returns (the batch, wall ms, the set's kernel ms)"""
        t0 = time.perf_counter()
        out = C.POINTER(binding.GaSeedSetLoci)()
        binding._check(L, L.ga_find_seeds_loci(G.h, r.arr, r.n_reads, C.byref(p), C.byref(out)), "ga_find_seeds_loci")
        S = out.contents
        shim = binding.ReadSet.__new__(binding.ReadSet)
        shim._keep, shim._names, shim.arr, shim.sarr, shim.n_reads, shim.total_bp = r._keep, r._names, r.arr, S.seeds, r.n_reads, r.total_bp
        shim.offs = np.ctypeslib.as_array(S.seed_offsets, shape=(r.n_reads + 1,))
        b = binding.Batch(G, shim, None, args.bandwidth, 0, 0)
        ms = (time.perf_counter() - t0) * 1e3
        kernel_ms = S.kernel_ms
        b._rs = r
        L.ga_seed_set_free(out)
        return b, ms, kernel_ms

    def one_call(r=rs):
        t0 = time.perf_counter()
        b = G.prepare_seeded(r, None, True, args.bandwidth)
        return b, (time.perf_counter() - t0) * 1e3

    calls = max(args.calls, 10)
    two_ms, two_kernel, one_ms, split = [], [], [], []
    jobs = [0, 0]
    for i in range(args.warmup + calls):
        b, ms, kms = two_call()
        jobs[0] = b.stats()["n_jobs"]
        b.close()
        b2, ms2 = one_call()
        ps = b2.prepare_stats()
        jobs[1] = ps["n_jobs"]
        b2.close()
        if i >= args.warmup:
            two_ms.append(ms); two_kernel.append(kms); one_ms.append(ms2); split.append(ps)
    two_ms, one_ms = np.array(two_ms), np.array(one_ms)

    def stat(a, warmup=None):
        return {"median": round(float(np.median(a)), 3), "min": round(float(a.min()), 3), "max": round(float(a.max()), 3), "calls": len(a),
                "warmup": args.warmup if warmup is None else warmup}

    def verdict(slow, fast):
        """is `fast` shorter than `slow` by more than the larger of the two min-max spreads (medians)"""
        spread = max(float(slow.max() - slow.min()), float(fast.max() - fast.min()))
        gain = float(np.median(slow) - np.median(fast))
        return {"difference": round(gain, 3), "larger_spread": round(spread, 3), "shorter_by_more_than_the_spread": bool(gain > spread)}

    # the overlapped pipeline over 12 chunks, the stage in front of the kernels being the two calls or the one
    chunk = (n + 11) // 12
    sets = [binding.ReadSet(reads[a:a + chunk], [[]] * len(reads[a:a + chunk])) for a in range(0, n, chunk)]

    class TwoCallGraph:
        def prepare(self, what, seeds, bw, ramp, flags):
            return two_call(what)[0]

    bp = sum(len(r) for r in reads)
    rate = {"two_call": [], "seeded": []}
    aligned = {}
    for i in range(1 + args.overlap_runs):
        for kind in ("two_call", "seeded"):
            t0 = time.perf_counter()
            if kind == "two_call":
                res = sharding.run_overlapped(TwoCallGraph(), list(enumerate(sets)), args.bandwidth, summary=True)
            else:
                res = sharding.run_overlapped(G, list(enumerate(sets)), args.bandwidth, summary=True, find_seeds=dict(params=None, loci=True))
            s = time.perf_counter() - t0
            aligned[kind] = int(sum(int(((r["status"] == 0) & (r["failed"] == 0)).sum()) for _, r in res))
            if i:
                rate[kind].append(s * 1e3)
    wall = {k: np.array(v) for k, v in rate.items()}
    return {
        "tool": "tools/bench_seed.py --seeded", "graph": args.graph, "genome_bp": args.genome, "node_len": args.node_len, "reads": n, "read_len": args.read_len,
        "read_bp": bp, "gen_s": round(gen_s, 1), "index_entries": st["entries"], "jobs": {"two_call": int(jobs[0]), "seeded": int(jobs[1])},
        "prepare_wall_ms": {"two_call": stat(two_ms), "seeded": stat(one_ms), "two_call_seed_kernel_ms": round(float(np.median(two_kernel)), 3), **verdict(two_ms, one_ms)},
        "seeded_split_ms": {k: round(float(np.median([d[k] for d in split])), 3) for k in ("seed_kernel_ms", "plan_kernel_ms", "eq_kernel_ms", "host_ms")},
        "reads_without_seed": int(split[-1]["reads_without_seed"]),
        "overlapped_12_chunks": {"wall_ms": {k: stat(v, 1) for k, v in wall.items()}, "Mbp_s": {k: round(bp / float(np.median(v)) / 1e3, 1) for k, v in wall.items()},
                                 "reads_aligned": aligned, **verdict(wall["two_call"], wall["seeded"])},
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", choices=["linear", "bubbles"], default="linear")
    ap.add_argument("--genome", type=int, default=4641652)
    ap.add_argument("--node-len", type=int, default=64, help="8 or more")
    ap.add_argument("--max-walks", type=int, default=0, help="0: the in-node index; 1..256: the walk index")
    ap.add_argument("--reads", type=int, default=50000)
    ap.add_argument("--read-len", type=int, default=10000)
    ap.add_argument("--bandwidth", type=int, default=35)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--align-runs", type=int, default=5)
    ap.add_argument("--loci", action="store_true", help="also measure ga_find_seeds_loci (one seed per locus)")
    ap.add_argument("--coord", choices=["file", "topology"], default="file", help="topology: also measure the topology coordinate")
    ap.add_argument("--shuffle-nodes", action="store_true", help="node list in a random order")
    ap.add_argument("--seeded", action="store_true", help="measure ga_batch_prepare_seeded beside ga_find_seeds_loci + ga_batch_prepare, and nothing else")
    ap.add_argument("--overlap-runs", type=int, default=3, help="--seeded: timed run_overlapped passes per path (one warm-up pass each before them)")
    args = ap.parse_args()
    if args.node_len < 8 or not 0 <= args.max_walks <= 256:
        raise SystemExit("bench_seed.py: --node-len must be 8 or more and --max-walks 0..256")

    import numpy as np
    # torch before the library: it brings the HIP runtime the library must bind to (tests/conftest.py)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_seed.py needs a GPU: there is no CPU path to time")
    import __graft_entry__ as entry
    entry.build_product()
    from graphaligner_amd import binding, synth

    t0 = time.time()
    if args.graph == "linear":
        g = synth.linear_graph(args.genome, node_len=args.node_len, seed=42)
    else:
        g = synth.bubble_graph(args.genome, node_len=args.node_len, seed=44)
    reads, seeds = synth.simulate_reads(g, args.reads, args.read_len, sub=0.04, ins=0.04, dele=0.04, seed=43)
    gen_s = time.time() - t0
    if args.shuffle_nodes:
        import random
        random.Random(1).shuffle(g.nodes)                       # (after the reads: they do not depend on the order)
    G = binding.Graph(gfa=g.gfa())

    if args.seeded:
        print(json.dumps(seeded_row(args, G, reads, gen_s)))
        return

    grouped = {}

    def timed_find():
        """with --loci the grouped call runs after every ungrouped one, warm-up included (its result and times go to `grouped`)"""
        for _ in range(args.warmup):
            found = G.find_seeds(reads)
            if args.loci:
                G.find_seeds(reads, loci=True)
        ms, ms_loci = [], []
        for _ in range(args.calls):
            found = G.find_seeds(reads)
            ms.append(found.kernel_ms)
            if args.loci:
                grouped["found"] = G.find_seeds(reads, loci=True)
                ms_loci.append(grouped["found"].kernel_ms)
        grouped["ms"] = np.array(ms_loci)
        return found, np.array(ms)

    def index_row(st):
        return {"k": st["k"], "sample_shift": st["sample_shift"], "kmers_seen": st["kmers_seen"], "entries": st["entries"], "distinct_keys": st["distinct_keys"],
                "bytes": st["bytes"], "build_ms": round(st["build_ms"], 2)}

    def ms_row(ms):
        return {"median": round(float(np.median(ms)), 3), "min": round(float(ms.min()), 3), "max": round(float(ms.max()), 3), "calls": len(ms),
                "warmup": args.warmup, "source": "HIP events around the kernel, inside the library"}

    st = G.build_seed_index()
    in_node = None
    if args.max_walks:
        G.build_seed_index()                                    # (built twice: the first build of a process also loads the kernels)
        st = G.seed_index_stats()
        found, ms = timed_find()
        in_node = {"index": index_row(st), "find_seeds_kernel_ms": ms_row(ms), "reads_without_seed": sum(1 for s in found.seeds if not s)}
        G.build_seed_index(max_walks=args.max_walks)
        st = G.build_seed_index(max_walks=args.max_walks)
        walk = G.seed_index_walk_stats()
    found, ms = timed_find()

    def aligner_kernel_ms(rd, sd):
        rs = binding.ReadSet(rd, sd)
        b = G.prepare(rs, None, args.bandwidth, 0)
        out = []
        for i in range(args.align_runs + 1):
            b.run()
            if i:                                       # (the first run warms up)
                out.append(b.stats()["kernel_ms"])
        jobs = b.stats()["n_jobs"]
        res = b.collect(summary=True)
        b.close()
        spreads.append(max(out) - min(out))
        return float(np.median(out)), int(jobs), int(((res["status"] == 0) & (res["failed"] == 0)).sum())

    spreads = []                                        # max - min of every aligner measurement, in call order

    true_ms, true_jobs, true_ok = aligner_kernel_ms(reads, seeds)
    have = [i for i in range(len(reads)) if found.seeds[i]]
    own_ms, own_jobs, own_ok = aligner_kernel_ms([reads[i] for i in have], [found.seeds[i] for i in have])
    bp = sum(len(r) for r in reads)
    sup = [s[0] for s in found.support if s]
    row = {
        "tool": "tools/bench_seed.py", "graph": args.graph, "genome_bp": args.genome, "node_len": args.node_len, "reads": len(reads), "read_len": args.read_len,
        "read_bp": bp, "gen_s": round(gen_s, 1),
        "index": index_row(st),
        "find_seeds_kernel_ms": ms_row(ms),
        "find_seeds_Gbp_s": round(bp / float(np.median(ms)) / 1e6, 2),
        "reads_without_seed": len(reads) - len(have), "truncated_reads": int(sum(found.truncated)),
        "mean_hits": round(float(np.mean(found.n_hits)), 1), "mean_support_of_first_seed": round(float(np.mean(sup)), 1) if sup else 0.0,
        "aligner_true_seeds": {"kernel_ms": round(true_ms, 3), "jobs": true_jobs, "reads_aligned": true_ok},
        "seed_ms_over_aligner_ms": round(float(np.median(ms)) / true_ms, 4),
        "aligner_own_seeds": {"kernel_ms": round(own_ms, 3), "jobs": own_jobs, "reads_aligned": own_ok,
                              "note": "seeds inside the reads: two extensions per read (and up to max_seeds seeds), where the true seeds at the first base make one; "
                                      "not comparable with README.md's rates"},
    }
    if args.loci:
        lf, lms = grouped["found"], grouped["ms"]
        lhave = [i for i in range(len(reads)) if lf.seeds[i]]
        loci_ms, loci_jobs, loci_ok = aligner_kernel_ms([reads[i] for i in lhave], [lf.seeds[i] for i in lhave])
        size = [s[0] for s in lf.locus_hits if s]
        sum_own, sum_loci = float(np.median(ms)) + own_ms, float(np.median(lms)) + loci_ms
        row["loci"] = {
            "find_seeds_loci_kernel_ms": ms_row(lms),
            "loci_kernel_over_find_seeds_kernel": round(float(np.median(lms)) / float(np.median(ms)), 3),
            "seeds": sum(len(s) for s in lf.seeds), "seeds_ungrouped": sum(len(s) for s in found.seeds),
            "reads_with_two_seeds": sum(1 for s in lf.seeds if len(s) > 1), "reads_with_two_seeds_ungrouped": sum(1 for s in found.seeds if len(s) > 1),
            "reads_without_seed": len(reads) - len(lhave), "loci_with_candidate": int(sum(lf.n_loci)),
            "first_seed_equals_ungrouped_first_seed": sum(1 for a, b in zip(lf.seeds, found.seeds) if a[:1] == b[:1]),
            "mean_hits_of_first_locus": round(float(np.mean(size)), 1) if size else 0.0,
            "aligner_grouped_seeds": {"kernel_ms": round(loci_ms, 3), "jobs": loci_jobs, "reads_aligned": loci_ok},
            "seed_ms_over_aligner_ms": round(float(np.median(lms)) / true_ms, 4),
            "seeding_plus_aligner_ms": {"ungrouped": round(sum_own, 3), "grouped": round(sum_loci, 3), "saving": round(sum_own - sum_loci, 3),
                                        "spread_ungrouped": round(float(ms.max() - ms.min()) + spreads[1], 3),
                                        "spread_grouped": round(float(lms.max() - lms.min()) + spreads[2], 3),
                                        "note": "medians; a spread is max - min of the seeding calls plus max - min of the aligner runs"},
        }
    if args.coord == "topology":
        G.set_seed_coordinate("topology")                       # (the first call of a process also loads the kernels)
        cs = G.set_seed_coordinate("topology")
        per = {"file": {"ms": [], "found": None}, "topology": {"ms": [], "found": None}}
        for i in range(args.warmup + args.calls):
            for kind in ("file", "topology"):
                G.set_seed_coordinate(kind)
                f = G.find_seeds(reads, loci=True)
                if i >= args.warmup:
                    per[kind]["ms"].append(f.kernel_ms)
                    per[kind]["found"] = f
        G.set_seed_coordinate("file")
        row["coord"] = {"shuffled_nodes": bool(args.shuffle_nodes), "build_ms": round(cs["build_ms"], 3), "index_build_ms": round(st["build_ms"], 2),
                        "trees": cs["trees"], "cycles_cut": cs["cycles_cut"], "cycle_rounds": cs["cycle_rounds"], "depth_rounds": cs["depth_rounds"],
                        "extent_sum": cs["extent_sum"]}
        for kind in ("file", "topology"):
            f, kms = per[kind]["found"], np.array(per[kind]["ms"])
            khave = [i for i in range(len(reads)) if f.seeds[i]]
            a_ms, a_jobs, a_ok = aligner_kernel_ms([reads[i] for i in khave], [f.seeds[i] for i in khave])
            ksup = [s[0] for s in f.support if s]
            row["coord"][kind] = {"find_seeds_loci_kernel_ms": ms_row(kms), "seeds": sum(len(s) for s in f.seeds),
                                  "reads_with_two_seeds": sum(1 for s in f.seeds if len(s) > 1), "reads_without_seed": len(reads) - len(khave),
                                  "mean_support_of_first_seed": round(float(np.mean(ksup)), 1) if ksup else 0.0,
                                  "aligner": {"kernel_ms": round(a_ms, 3), "jobs": a_jobs, "reads_aligned": a_ok},
                                  "seeding_plus_aligner_ms": round(float(np.median(kms)) + a_ms, 3)}
    if args.max_walks:
        row["walk"] = {key: int(v) for key, v in walk.items()}
        row["in_node"] = in_node
    print(json.dumps(row))


if __name__ == "__main__":
    main()
