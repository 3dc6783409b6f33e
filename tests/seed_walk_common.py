"""shared helpers of the walk-index tests (tests/test_seed_walks.py on the host build, tests/test_seed_walks_gpu.py on the product
library): the graphs, the comparison of a library's walk index with the model of tests/seed_walk_model.py, and the accuracy run of
seed_common.accuracy with a walk index (that function builds its index without arguments, hence the variant here)."""

import numpy as np

from graphaligner_amd import binding, compare, synth
import seed_walk_model


GRAPHS = {
    "short8": lambda: synth.SynthGraph(synth.random_genome(4000, 5), node_len=8, snp_every=40, seed=2),      # test_seed_index.py's
    "bubbles8": lambda: synth.bubble_graph(12000, node_len=8, seed=3),
    "bubbles32": lambda: synth.bubble_graph(12000, node_len=32, seed=3),
    "cyclic16": lambda: synth.cyclic_graph(3000, node_len=16),                                              # back edges and self-loops
    "linear": lambda: synth.linear_graph(12000),
}


def walk_index_cases():
    """(graph, k, sample_shift, max_walks)"""
    for k in (11, 15, 31):
        for s in (0, 2, 5):
            yield "short8", k, s, 64
    for name in ("bubbles8", "bubbles32", "cyclic16", "linear"):
        for max_walks in (1, 4, 64, 256):
            for k, s in ((15, 2), (31, 0)):
                yield name, k, s, max_walks


def check_walk_index(nodes, edges, k, s, max_walks, lib_path):
    """index, index statistics and walk statistics of the library against the model's; returns (graph, model, index stats, walk stats)"""
    g = binding.Graph(nodes, edges, lib_path=lib_path)
    st = g.build_seed_index(k=k, sample_shift=s, max_walks=max_walks)
    ws = g.seed_index_walk_stats()
    keys, idx, offs = g.seed_index_entries()
    model = seed_walk_model.WalkModel(nodes, edges, k, s, max_walks)
    want = model.entries()
    got = list(zip(keys.tolist(), idx.tolist(), offs.tolist()))
    assert len(got) == len(want), ("entries", len(got), len(want))
    assert got == want
    assert ws == model.stats, (ws, model.stats)
    assert st["entries"] == len(want) and st["distinct_keys"] == len(set(e[0] for e in want))
    assert st["kmers_seen"] == model.kmers_seen == 2 * sum(max(0, len(seq) - k + 1) for _, seq in nodes) + ws["walk_kmers"]
    assert st["k"] == k and st["sample_shift"] == s and st["bytes"] >= 16 * len(want)
    return g, model, st, ws


def accuracy_walks(graph, reads, true_seeds, truth, align_lib, seed_lib, max_walks, bw=35, **params):
    """seed_common.accuracy with a walk index: every read counts in both runs (a read without a seed, failed, or with any other status
    is absent from the predictions, which compare.compare counts as a bad match).  The in-node index of the same graph is built first
    and the reads it gives a seed are counted."""
    names = ["read%d" % i for i in range(len(reads))]
    sizes = {nid: len(seq) for nid, seq in graph.nodes}
    truth_by_name = {n: t for n, t in zip(names, truth)}
    ga = binding.Graph(graph.nodes, graph.edges, lib_path=align_lib)
    gs = ga if seed_lib == align_lib else binding.Graph(graph.nodes, graph.edges, lib_path=seed_lib)
    st0 = gs.build_seed_index()
    in_node = gs.find_seeds(reads, **params)
    st = gs.build_seed_index(max_walks=max_walks)
    ws = gs.seed_index_walk_stats()
    found = gs.find_seeds(reads, **params)

    def good(seeds):
        have = [i for i in range(len(reads)) if seeds[i]]
        predicted = {}
        if have:
            out = ga.align([reads[i] for i in have], [list(seeds[i]) if isinstance(seeds[i], list) else [seeds[i]] for i in have], bw, flags=0)
            for i, r in zip(have, out):
                if r["status"] == 0 and not r["failed"]:
                    predicted[names[i]] = compare.predicted_nodes(r)
        return compare.compare(truth_by_name, predicted, sizes)["good"]

    good_true = good([[s] for s in true_seeds])
    good_own = good(found.seeds)
    sup = [s[0] for s in found.support if s]
    return dict(reads=len(reads), good_true_seeds=good_true, good_own_seeds=good_own, allowance=max(1, len(reads) // 100),
                reads_with_seed_in_node_index=sum(1 for s in in_node.seeds if s), in_node_index_entries=int(st0["entries"]),
                reads_without_seed=sum(1 for s in found.seeds if not s), mean_support=round(float(np.mean(sup)), 2) if sup else 0.0,
                truncated_reads=sum(1 for t in found.truncated if t), index_entries=int(st["entries"]), index_bytes=int(st["bytes"]),
                max_walks=int(ws["max_walks"]), tail_starts=int(ws["tail_starts"]), tail_starts_skipped=int(ws["tail_starts_skipped"]),
                walk_kmers=int(ws["walk_kmers"]), duplicates_dropped=int(ws["duplicates_dropped"]), seed_kernel_ms=round(found.kernel_ms, 3))
