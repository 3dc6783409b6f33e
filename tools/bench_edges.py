"""Edge support (pileups of kind "edges") measured on the workload of bench.py (E. coli-scale linear graph of 64-bp nodes, 50 000 x 10 kb
reads at ONT error, one seed at the first base) or on the bubble graph.  One JSON line on stdout.

    python tools/bench_edges.py --graph linear
    python tools/bench_edges.py --graph bubbles

One batch is prepared with GA_F_OPS | GA_F_PILEUP, run and collected once; then --warmup adds and --calls timed adds, the two kinds
alternating (an EDGES pileup and a DEPTH pileup of the same graph), each add the whole batch again.  Reported per kind: the add's
HIP-event kernel time (ga_pileup_stats) as median and min-max, moves read per second and items per second.  The yardstick is the
DEPTH add of the same run -- the same walk over the same moves with one atomic per item, where EDGES has about one per node length --
and next to both the time of ga_ops_count_kernel on the same batch: the walk with no atomics at all.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", choices=["linear", "bubbles"], default="linear")
    ap.add_argument("--genome", type=int, default=4641652)
    ap.add_argument("--node-len", type=int, default=64)
    ap.add_argument("--reads", type=int, default=50000)
    ap.add_argument("--read-len", type=int, default=10000)
    ap.add_argument("--bandwidth", type=int, default=35)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()

    import numpy as np
    # torch before the library: it brings the HIP runtime the library must bind to (tests/conftest.py)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_edges.py needs a GPU: there is no CPU path to time")
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
    G = binding.Graph(gfa=g.gfa())
    L = G.L
    whole = binding.ReadSet(reads, seeds)

    def stat(a):
        a = np.array(a, dtype=np.float64)
        return {"median": round(float(np.median(a)), 3), "min": round(float(a.min()), 3), "max": round(float(a.max()), 3), "calls": len(a), "warmup": args.warmup}

    b = G.prepare(whole, None, args.bandwidth, 0, binding.GA_F_OPS | binding.GA_F_PILEUP)
    b.run()
    out = C.POINTER(binding.GaResultsOps)()
    binding._check(L, L.ga_batch_collect(b.h, C.byref(out)), "ga_batch_collect")
    L.ga_results_free(out)
    ops, bst = b.ops_stats(), b.stats()
    piles = {"edges": G.pileup("edges"), "depth": G.pileup("depth")}
    ms = {"edges": [], "depth": []}
    per_add = {}
    for i in range(args.warmup + args.calls):
        for kind, p in piles.items():
            before = p.stats()
            p.add(b)
            st = p.stats()
            per_add[kind] = {"items": st["items_added"] - before["items_added"], "moves": st["moves_read"] - before["moves_read"],
                             "jobs": st["jobs_walked"] - before["jobs_walked"]}
            if i >= args.warmup:
                ms[kind].append(st["add_kernel_ms"])
    # (every add was the same batch: a slot's count is a multiple of the number of adds, and the grand total is the items added)
    n_adds = args.warmup + args.calls
    edges = piles["edges"].counts().astype(np.int64)
    consistent = bool(int(edges.sum()) == n_adds * per_add["edges"]["items"] and not (edges % n_adds).any())
    folded = piles["edges"].edge_support()
    res = {"tool": "tools/bench_edges.py", "graph": args.graph, "genome_bp": args.genome, "node_len": args.node_len, "reads": len(reads), "read_len": args.read_len,
           "read_bp": whole.total_bp, "gen_s": round(gen_s, 1), "kernel_ms_of_the_run": round(bst["kernel_ms"], 3),
           "ops_count_kernel_ms_same_batch": round(ops["count_kernel_ms"], 3), "ops_write_kernel_ms_same_batch": round(ops["write_kernel_ms"], 3),
           "reads_from_device": piles["edges"].stats()["reads_from_device"] // n_adds, "reads_from_host": piles["edges"].stats()["reads_from_host"] // n_adds,
           "slots": piles["edges"].entries, "columns": piles["depth"].entries, "bigraph_edges": len(folded),
           "bigraph_edges_supported": sum(1 for c in folded.values() if c >= 1), "counts_consistent": consistent}
    for kind in ms:
        med = float(np.median(ms[kind])) / 1e3
        res[kind] = {"add_kernel_ms": stat(ms[kind]), "jobs_walked": per_add[kind]["jobs"], "moves_read": per_add[kind]["moves"], "items_added": per_add[kind]["items"],
                     "moves_per_s": round(per_add[kind]["moves"] / med, 1), "items_per_s": round(per_add[kind]["items"] / med, 1),
                     "add_over_ops_count_kernel": round(med * 1e3 / ops["count_kernel_ms"], 3)}
    res["edges_median_over_depth_median"] = round(res["edges"]["add_kernel_ms"]["median"] / res["depth"]["add_kernel_ms"]["median"], 3)
    res["edges_median_above_depth_max"] = bool(res["edges"]["add_kernel_ms"]["median"] > res["depth"]["add_kernel_ms"]["max"])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
