"""Build time of the topology coordinate (ga_graph_set_seed_coordinate) next to the index build it follows: the bubble graph of
tools/bench_seed.py at 64-bp nodes (in-node index) and at 8-bp nodes (walk index), each in path order and with its node list
shuffled (random.Random(1).shuffle).  One JSON line on stdout: per graph the nodes, the index build's build_ms (the second build of the
process: the first also loads the kernels), the coordinate's build_ms over --calls calls after one warm-up call (median, min, max;
wall time of the call's device work, inside the library), its rounds, trees and cycles cut.

    python tools/bench_seed_coord.py
    python tools/bench_seed_coord.py --node-len 8 --shuffle-nodes --calls 1      # one build, for a kernel trace
"""
import argparse
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=4641652)
    ap.add_argument("--node-len", type=int, default=0, help="64 or 8; 0: both")
    ap.add_argument("--shuffle-nodes", action="store_true", help="only the shuffled node list (default: path order and shuffled)")
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()

    import numpy as np
    # torch before the library: it brings the HIP runtime the library must bind to (tests/conftest.py)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_seed_coord.py needs a GPU: there is no CPU path to time")
    import __graft_entry__ as entry
    entry.build_product()
    from graphaligner_amd import binding, synth

    rows = []
    for node_len in ([args.node_len] if args.node_len else [64, 8]):
        g = synth.bubble_graph(args.genome, node_len=node_len, seed=44)
        path_order = list(g.nodes)
        for shuffle in ([True] if args.shuffle_nodes else [False, True]):
            g.nodes = list(path_order)
            if shuffle:
                random.Random(1).shuffle(g.nodes)
            G = binding.Graph(gfa=g.gfa())
            walks = 64 if node_len < 15 else 0
            G.build_seed_index(max_walks=walks)
            st = G.build_seed_index(max_walks=walks)
            G.set_seed_coordinate("topology")
            ms = []
            for _ in range(args.calls):
                cs = G.set_seed_coordinate("topology")
                ms.append(cs["build_ms"])
            ms = np.array(ms)
            rows.append({"graph": "bubbles", "genome_bp": args.genome, "node_len": node_len, "shuffled_nodes": shuffle, "nodes": int(G.node_count),
                         "index": {"max_walks": walks, "entries": int(st["entries"]), "build_ms": round(st["build_ms"], 2)},
                         "coordinate_build_ms": {"median": round(float(np.median(ms)), 3), "min": round(float(ms.min()), 3), "max": round(float(ms.max()), 3),
                                                 "calls": len(ms), "warmup": 1, "source": "wall time of the call's device work, inside the library"},
                         "cycle_rounds": cs["cycle_rounds"], "depth_rounds": cs["depth_rounds"], "trees": cs["trees"], "cycles_cut": cs["cycles_cut"]})
            del G
    print(json.dumps({"tool": "tools/bench_seed_coord.py", "rows": rows}))


if __name__ == "__main__":
    main()
