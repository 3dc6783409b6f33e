"""GA_F_PATHSEQ measured next to the operations kernels whose walk it shares: the headline workload of bench.py (E. coli-scale linear
graph of 64-bp nodes, 50 000 x 10 kb reads at ONT error, one seed at the first base) or the bubble graph.  One JSON line on stdout.

    python tools/bench_pathseq.py --graph linear
    python tools/bench_pathseq.py --graph bubbles

Whole batch, flags 0, GA_F_OPS, GA_F_PATHSEQ and GA_F_OPS | GA_F_PATHSEQ alternating call by call (--warmup calls, then --calls timed
ones): the batch's kernel_ms, the two path-sequence kernels' HIP-event times (ga_batch_path_seq_stats) next to the two operations kernels'
of the same batch (the batches with both flags), and whether a path-sequence launch is slower than its operations counterpart by more
than the larger of the two min-max spreads; bases per move; the wall time of ga_batch_collect at the C ABI and the bytes each flag adds
to the download (offsets and runs or bases; the moves themselves come down with either flag, not with flags 0).
A subset that fits the result pool (--trace-reads), flags 0, GA_F_OPS, GA_F_PATHSEQ and GA_F_TRACE alternating: the wall time of
ga_batch_collect.
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
        raise SystemExit("bench_pathseq.py needs a GPU: there is no CPU path to time")
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
    F0, FO, FP, FT = 0, binding.GA_F_OPS, binding.GA_F_PATHSEQ, binding.GA_F_TRACE

    def one(rs, flags):
        """prepare, run, collect at the C ABI -> (batch statistics, operations statistics, path-sequence statistics, collect wall ms, path bases of the reads)"""
        b = G.prepare(rs, None, args.bandwidth, 0, flags)
        b.run()
        out = C.POINTER(binding.GaResultsPathSeq if flags & FP else binding.GaResultsOps if flags & FO else binding.GaResults)()
        t = time.perf_counter()
        binding._check(L, L.ga_batch_collect(b.h, C.byref(out)), "ga_batch_collect")
        ms = (time.perf_counter() - t) * 1e3
        R = out.contents
        read_bases = 0
        if flags & FP:
            recs = np.ctypeslib.as_array(C.cast(R.read_path_seq, C.POINTER(C.c_uint32)), shape=(R.n_reads, 4))
            read_bases = int(recs[:, 2].sum())
        st, ops, path = b.stats(), (b.ops_stats() if flags & FO else None), (b.path_seq_stats() if flags & FP else None)
        L.ga_results_free(out)
        b.close()
        return st, ops, path, ms, read_bases

    def stat(a):
        a = np.array(a, dtype=np.float64)
        return {"median": round(float(np.median(a)), 3), "min": round(float(a.min()), 3), "max": round(float(a.max()), 3), "calls": len(a), "warmup": args.warmup}

    def verdict(ref, new):
        """is `new` longer than `ref` by more than the larger of the two min-max spreads (medians)"""
        ref, new = np.array(ref), np.array(new)
        spread = max(float(ref.max() - ref.min()), float(new.max() - new.min()))
        more = float(np.median(new) - np.median(ref))
        return {"difference": round(more, 3), "larger_spread": round(spread, 3), "longer_by_more_than_the_spread": bool(more > spread)}

    variants = (F0, FO, FP, FO | FP)
    name = {F0: "flags_0", FO: "GA_F_OPS", FP: "GA_F_PATHSEQ", FO | FP: "GA_F_OPS|GA_F_PATHSEQ", FT: "GA_F_TRACE"}
    kernel = {f: [] for f in variants}
    collect = {f: [] for f in variants}
    times = {k: [] for k in ("ops_count", "ops_write", "path_count", "path_write", "path_count_alone", "path_write_alone")}
    last_ops = last_path = None
    read_bases = 0
    for i in range(args.warmup + args.calls):
        for flags in variants:
            st, ops, path, ms, rb = one(whole, flags)
            if i < args.warmup:
                continue
            kernel[flags].append(st["kernel_ms"])
            collect[flags].append(ms)
            if flags == (FO | FP):
                times["ops_count"].append(ops["count_kernel_ms"]); times["ops_write"].append(ops["write_kernel_ms"])
                times["path_count"].append(path["count_kernel_ms"]); times["path_write"].append(path["write_kernel_ms"])
                last_ops, last_path, read_bases = ops, path, rb
            elif flags == FP:
                times["path_count_alone"].append(path["count_kernel_ms"]); times["path_write_alone"].append(path["write_kernel_ms"])
    sub_variants = (F0, FO, FP, FT)
    sub = {f: [] for f in sub_variants}
    for i in range(args.warmup + args.calls):
        for flags in sub_variants:
            _, _, _, ms, _ = one(subset, flags)
            if i >= args.warmup:
                sub[flags].append(ms)
    jobs = last_path["jobs_walked"]
    print(json.dumps({
        "tool": "tools/bench_pathseq.py", "graph": args.graph, "genome_bp": args.genome, "node_len": args.node_len, "reads": len(reads), "read_len": args.read_len,
        "read_bp": whole.total_bp, "gen_s": round(gen_s, 1),
        "kernel_ms": {name[f]: stat(kernel[f]) for f in variants},
        "same_batch_kernel_ms": {k: stat(times[k]) for k in ("ops_count", "ops_write", "path_count", "path_write")},
        "path_kernels_alone_ms": {"count": stat(times["path_count_alone"]), "write": stat(times["path_write_alone"])},
        "path_count_against_ops_count": verdict(times["ops_count"], times["path_count"]),
        "path_write_against_ops_write": verdict(times["ops_write"], times["path_write"]),
        "jobs_walked": jobs, "moves_read": last_path["moves_read"], "bases_written": last_path["bases_written"], "bases_in_results": read_bases,
        "bases_per_move": round(last_path["bases_written"] / max(last_path["moves_read"], 1), 4), "runs_written": last_ops["runs_written"],
        "reads_from_device": last_path["reads_from_device"], "reads_from_host": last_path["reads_from_host"],
        "download_bytes_added": {"moves_with_either_flag": last_path["moves_read"], "GA_F_OPS": 4 * last_ops["runs_written"] + 8 * (jobs + 1),
                                 "GA_F_PATHSEQ": last_path["bases_written"] + 8 * (jobs + 1)},
        "collect_wall_ms_whole_batch": {name[f]: stat(collect[f]) for f in variants},
        "collect_wall_ms_subset": dict({"reads": n_sub}, **{name[f]: stat(sub[f]) for f in sub_variants}),
    }))


if __name__ == "__main__":
    main()
