"""Site queries (ga_pileup_sites) measured.  One JSON line on stdout.

    python tools/bench_sites.py --mode compare --graph linear      # against the only thing there was before: the whole download
    python tools/bench_sites.py --mode compare --graph bubbles
    python tools/bench_sites.py --mode rate --gbp 0.128            # the mark kernel's rate on a large, almost empty pileup

compare: the graph and batch of tools/bench_pileup.py (E. coli-scale graph of 64-bp nodes, 50 000 x 10 kb reads at ONT error), the batch
added once to a BASES pileup.  Then --warmup and --calls timed calls of each of the two, alternating in one run: the whole Pileup.sites()
call, folded, at (min_depth 3, min_alt 2, 1/4) -- both kernels, the scan, the download of the sites and their conversion --, and
Pileup.counts() of the whole pileup.  The numpy selection over the downloaded planes (tests/site_model.py, the same rule) is timed
separately, once per call, and its result must equal the device's.  Reported: medians and min-max of each, and whether the sites call's
median is shorter than the download's by more than the larger of the two min-max spreads.

rate: a graph from the native generator of tools/bench_c5.py (tests/native), a BASES pileup that is zero but for one small batch, and
--calls folded queries over all of it.  bytes_read = 32 per column, once, plus the 1-bit-per-entry mask the kernel stores; the kernel's
own time comes from a profiler run of this mode (rocprofv3 --kernel-trace --stats -- python tools/bench_sites.py --mode rate ...); the
HIP-event time over both launches and the scan is reported here as an upper bound.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

QUERY = dict(min_depth=3, min_alt=2, alt_frac=(1, 4))


def stat(np, a, warmup):
    a = np.array(a, dtype=np.float64)
    return {"median": round(float(np.median(a)), 3), "min": round(float(a.min()), 3), "max": round(float(a.max()), 3), "calls": len(a), "warmup": warmup}


def compare(args, np, binding, synth):
    import site_model as sm
    t0 = time.time()
    g = synth.linear_graph(args.genome, node_len=args.node_len, seed=42) if args.graph == "linear" else synth.bubble_graph(args.genome, node_len=args.node_len, seed=44)
    reads, seeds = synth.simulate_reads(g, args.reads, args.read_len, sub=0.04, ins=0.04, dele=0.04, seed=43)
    gen_s = time.time() - t0
    G = binding.Graph(g.nodes, g.edges)
    b = G.prepare(binding.ReadSet(reads, seeds), None, args.bandwidth, 0, binding.GA_F_PILEUP)
    b.run()
    b.collect(summary=True)
    pile = G.pileup("bases")
    pile.add(b)
    ids = [0] + [i for n, _ in g.nodes for i in (2 * n, 2 * n + 1)] + [0]
    lens = [1] + [len(s) for _, s in g.nodes for _ in (0, 1)] + [1]
    node_start, twin, forward = sm.tables_of_graph(ids, lens)
    assert int(node_start[-1]) == pile.entries
    ms = {"sites_call": [], "download": [], "numpy_selection": [], "sites_kernels": []}
    equal = True
    for i in range(args.warmup + args.calls):
        t0 = time.perf_counter()
        got = pile.sites(fold=True, **QUERY)
        t1 = time.perf_counter()
        planes = pile.counts()
        t2 = time.perf_counter()
        want_e, want_F = sm.sites(planes, "bases", fold=True, node_start=node_start, twin=twin, forward=forward, **QUERY)
        t3 = time.perf_counter()
        equal = equal and np.array_equal(got["entry"].astype(np.int64), want_e) and np.array_equal(got["counts"], want_F)
        if i >= args.warmup:
            ms["sites_call"].append((t1 - t0) * 1e3)
            ms["download"].append((t2 - t1) * 1e3)
            ms["numpy_selection"].append((t3 - t2) * 1e3)
            ms["sites_kernels"].append(got.kernel_ms)
    res = {"tool": "tools/bench_sites.py", "mode": "compare", "graph": args.graph, "genome_bp": args.genome, "node_len": args.node_len, "reads": len(reads),
           "read_len": args.read_len, "gen_s": round(gen_s, 1), "columns": pile.entries, "pileup_bytes": pile.entries * 32, "query": "fold, min_depth 3, min_alt 2, 1/4",
           "sites": int(got.total), "site_bytes": int(got.total) * binding.SITE_DTYPE.itemsize, "equal_to_numpy_model": bool(equal)}
    for k, v in ms.items():
        res[k + "_ms"] = stat(np, v, args.warmup)
    s, d = res["sites_call_ms"], res["download_ms"]
    spread = max(s["max"] - s["min"], d["max"] - d["min"])
    res["larger_spread_ms"] = round(spread, 3)
    res["sites_call_shorter_than_download_by_more_than_the_spread"] = bool(d["median"] - s["median"] > spread)
    return res


def rate(args, np, binding, synth):
    import subprocess
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "native")])
    SG = C.CDLL(os.path.join(ROOT, "tests", "_build", "libga_scalegen.so"))
    SG.ga_scalegen_bubbles.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_int]
    SG.ga_scalegen_bubbles_walk.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_uint64, C.c_char_p]
    SG.ga_scalegen_bubbles_walk.restype = C.c_uint64
    seed, block, node_len = 50, 45, 32
    n_blocks = int(args.gbp * 1e9) // block
    L = binding.load()
    t0 = time.time()
    gg = object.__new__(binding.Graph)
    gg.L = L
    gg.h = L.ga_graph_create()
    binding._check(L, SG.ga_scalegen_bubbles(gg.h, seed, n_blocks, block, node_len), "ga_scalegen_bubbles")
    binding._check(L, L.ga_graph_upload(gg.h, 0), "ga_graph_upload")
    build_s = time.time() - t0
    rng = np.random.default_rng(52)
    read_len, n_reads = 5000, 200
    blocks_per_read = read_len // (block - 2) + 64
    reads, seeds = [], []
    buf = C.create_string_buffer(read_len)
    for i, b0 in enumerate(rng.integers(4, n_blocks - blocks_per_read - 4, size=n_reads)):
        n = SG.ga_scalegen_bubbles_walk(seed, 1000 + i, int(b0), n_blocks, block, node_len, read_len, buf)
        reads.append(synth.add_errors(np.frombuffer(buf.raw[:n], dtype=np.uint8), 0.04, 0.04, 0.04, rng).tobytes().decode())
        seeds.append((int(b0) * 16 + 1, 0, False))
    b = gg.prepare(binding.ReadSet(reads, seeds), None, args.bandwidth, 0, binding.GA_F_PILEUP)
    b.run()
    b.collect(summary=True)
    pile = gg.pileup("bases")
    pile.add(b)
    res = {"tool": "tools/bench_sites.py", "mode": "rate", "gbp_one_strand": args.gbp, "columns": pile.entries, "graph_build_and_upload_s": round(build_s, 1),
           "items_in_the_pileup": int(pile.stats()["items_added"])}
    for fold in (True, False):
        ms, call = [], []
        for i in range(args.warmup + args.calls):
            t0 = time.perf_counter()
            got = pile.sites(fold=fold, min_depth=1, min_alt=1)
            if i >= args.warmup:
                call.append((time.perf_counter() - t0) * 1e3)
                ms.append(got.kernel_ms)
        # every plane word once: with the fold the forward copies' lanes read both strands' words, the reverse copies' lanes read nothing
        bytes_read = pile.entries * 32 + pile.entries // 8
        key = "fold" if fold else "unfolded"
        res[key] = {"sites": int(got.total), "bytes_read": bytes_read, "events_ms_both_launches_and_scan": stat(np, ms, args.warmup), "call_ms": stat(np, call, args.warmup),
                    "TB_per_s_by_events_lower_bound": round(bytes_read / (float(np.median(ms)) * 1e-3) / 1e12, 3)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["compare", "rate"], default="compare")
    ap.add_argument("--graph", choices=["linear", "bubbles"], default="linear")
    ap.add_argument("--genome", type=int, default=4641652)
    ap.add_argument("--node-len", type=int, default=64)
    ap.add_argument("--reads", type=int, default=50000)
    ap.add_argument("--read-len", type=int, default=10000)
    ap.add_argument("--bandwidth", type=int, default=35)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--gbp", type=float, default=0.128, help="rate: bases of one strand, in Gbp (the pileup has twice as many columns)")
    args = ap.parse_args()
    import numpy as np
    # torch before the library: it brings the HIP runtime the library must bind to (tests/conftest.py)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_sites.py needs a GPU: there is no CPU path to time")
    import __graft_entry__ as entry
    entry.build_product()
    from graphaligner_amd import binding, synth
    print(json.dumps((compare if args.mode == "compare" else rate)(args, np, binding, synth)))


if __name__ == "__main__":
    main()
