"""GA_F_OPS measured next to the aligner whose moves it codes: the headline workload of bench.py (E. coli-scale linear graph of 64-bp
nodes, 50 000 x 10 kb reads at ONT error, one seed at the first base) or the bubble graph.  One JSON line on stdout.

    python tools/bench_ops.py --graph linear
    python tools/bench_ops.py --graph bubbles

Whole batch, flags 0 and GA_F_OPS alternating call by call (--warmup calls, then --calls timed ones): the batch's kernel_ms, the two
operations kernels' HIP-event times (ga_batch_ops_stats) and their share of kernel_ms, runs per move, and the wall time of
ga_batch_collect at the C ABI.  With flags 0 such a batch hands back node runs, with GA_F_OPS moves (as with GA_F_TRACE), so the two
kernel_ms are reported side by side.
A subset that fits the result pool (--trace-reads), flags 0, GA_F_OPS and GA_F_TRACE alternating: the wall time of ga_batch_collect,
and whether GA_F_OPS costs less than GA_F_TRACE by more than the larger of the two min-max spreads.
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
    ap.add_argument("--trace-reads", type=int, default=4000, help="reads of the subset that is also collected with GA_F_TRACE (32 bytes per cell)")
    args = ap.parse_args()

    import numpy as np
    # torch before the library: it brings the HIP runtime the library must bind to (tests/conftest.py)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_ops.py needs a GPU: there is no CPU path to time")
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
    n_sub = min(args.trace_reads, len(reads))
    subset = binding.ReadSet(reads[:n_sub], seeds[:n_sub])

    def one(rs, flags):
        """prepare, run, collect at the C ABI -> (batch statistics, operations statistics or None, collect wall ms, reads aligned)"""
        b = G.prepare(rs, None, args.bandwidth, 0, flags)
        b.run()
        out = C.POINTER(binding.GaResultsOps if flags & binding.GA_F_OPS else binding.GaResults)()
        t = time.perf_counter()
        binding._check(L, L.ga_batch_collect(b.h, C.byref(out)), "ga_batch_collect")
        ms = (time.perf_counter() - t) * 1e3
        R = out.contents
        ok = sum(1 for i in range(0, R.n_reads, max(1, R.n_reads // 500)) if R.reads[i].status == 0 and not R.reads[i].failed)
        st, ops = b.stats(), (b.ops_stats() if flags & binding.GA_F_OPS else None)
        L.ga_results_free(out)
        b.close()
        return st, ops, ms, ok

    def stat(a):
        a = np.array(a, dtype=np.float64)
        return {"median": round(float(np.median(a)), 3), "min": round(float(a.min()), 3), "max": round(float(a.max()), 3), "calls": len(a), "warmup": args.warmup}

    def verdict(slow, fast):
        """is `fast` shorter than `slow` by more than the larger of the two min-max spreads (medians)"""
        slow, fast = np.array(slow), np.array(fast)
        spread = max(float(slow.max() - slow.min()), float(fast.max() - fast.min()))
        gain = float(np.median(slow) - np.median(fast))
        return {"difference": round(gain, 3), "larger_spread": round(spread, 3), "shorter_by_more_than_the_spread": bool(gain > spread)}

    F0, FO, FT = 0, binding.GA_F_OPS, binding.GA_F_TRACE
    kernel = {F0: [], FO: []}
    collect = {F0: [], FO: []}
    count_ms, write_ms, share = [], [], []
    last_ops = None
    for i in range(args.warmup + args.calls):
        for flags in (F0, FO):
            st, ops, ms, _ = one(whole, flags)
            if i >= args.warmup:
                kernel[flags].append(st["kernel_ms"])
                collect[flags].append(ms)
                if ops:
                    count_ms.append(ops["count_kernel_ms"]); write_ms.append(ops["write_kernel_ms"])
                    share.append((ops["count_kernel_ms"] + ops["write_kernel_ms"]) / st["kernel_ms"])
                    last_ops = ops
    sub = {F0: [], FO: [], FT: []}
    for i in range(args.warmup + args.calls):
        for flags in (F0, FO, FT):
            _, _, ms, _ = one(subset, flags)
            if i >= args.warmup:
                sub[flags].append(ms)
    print(json.dumps({
        "tool": "tools/bench_ops.py", "graph": args.graph, "genome_bp": args.genome, "node_len": args.node_len, "reads": len(reads), "read_len": args.read_len,
        "read_bp": whole.total_bp, "gen_s": round(gen_s, 1),
        "kernel_ms": {"flags_0_node_runs": stat(kernel[F0]), "GA_F_OPS_moves": stat(kernel[FO])},
        "ops_count_kernel_ms": stat(count_ms), "ops_write_kernel_ms": stat(write_ms),
        "ops_kernels_share_of_kernel_ms": stat(share),
        "jobs_coded": last_ops["jobs_coded"], "moves_read": last_ops["moves_read"], "runs_written": last_ops["runs_written"],
        "runs_per_move": round(last_ops["runs_written"] / max(last_ops["moves_read"], 1), 4),
        "reads_from_device": last_ops["reads_from_device"], "reads_from_host": last_ops["reads_from_host"],
        "collect_wall_ms_whole_batch": {"flags_0": stat(collect[F0]), "GA_F_OPS": stat(collect[FO])},
        "collect_wall_ms_subset": {"reads": n_sub, "flags_0": stat(sub[F0]), "GA_F_OPS": stat(sub[FO]), "GA_F_TRACE": stat(sub[FT]),
                                   "GA_F_OPS_against_GA_F_TRACE": verdict(sub[FT], sub[FO])},
    }))


if __name__ == "__main__":
    main()
