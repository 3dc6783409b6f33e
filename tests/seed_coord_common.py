"""shared helpers of the topology-coordinate tests (tests/test_seed_coord.py on the host build, tests/test_seed_coord_gpu.py on the
product library): the host build, graphs with their node list permuted, the hand-made chains, cycles and self-loops, the comparison of
ga_graph_set_seed_coordinate with the model of tests/seed_coord_model.py, and the accuracy run of seed_common.accuracy with the
coordinate set."""
import ctypes as C
import random

import numpy as np

from graphaligner_amd import binding, compare, synth
import seed_coord_model as scm

STAT_KEYS = ("kind", "trees", "cycles_cut", "cycle_rounds", "depth_rounds", "extent_sum")


def shuffled(nodes, seed=1):
    """the node list in a random order; the edges stay as they are"""
    out = list(nodes)
    random.Random(seed).shuffle(out)
    return out


def closed(g):
    """the edges of a SynthGraph plus one from its last node to its first (its ids run along the path, whatever the order of the node
    list): a circular contig"""
    ids = [nid for nid, _ in g.nodes]
    return list(g.edges) + [(max(ids), False, min(ids), False)]


def dna(n, seed):
    return synth.random_genome(n, seed).tobytes().decode()


def chain(n, seed=0):
    """n nodes of 1 to 40 bp, 1 -> 2 -> ... -> n"""
    rng = random.Random(100 + seed)
    nodes = [(i + 1, dna(rng.randint(1, 40), 1000 * seed + i)) for i in range(n)]
    return nodes, [(i, False, i + 1, False) for i in range(1, n)]


def cycle(n, tail=0, first_id=1, seed=0):
    """a cycle of n nodes (ids first_id ..) and a chain of `tail` nodes (the ids behind them) that leads into its first node"""
    rng = random.Random(200 + seed)
    ids = list(range(first_id, first_id + n + tail))
    nodes = [(i, dna(rng.randint(1, 40), 1000 * seed + i)) for i in ids]
    cyc, tl = ids[:n], ids[n:]
    edges = [(cyc[i], False, cyc[(i + 1) % n], False) for i in range(n)]
    edges += [(tl[i], False, tl[i + 1], False) for i in range(len(tl) - 1)]
    if tl:
        edges.append((tl[-1], False, cyc[0], False))
    return nodes, edges


def graph_with_lists(lib_path, nodes, edges, given_in, given_out):
    """a binding.Graph whose digraph nodes named in `given_in` / `given_out` ({digraph id: [digraph ids]}) get their finished neighbour
    lists through ga_graph_set_neighbors, the rest through the bigraph calls"""
    L = binding.load(lib_path)
    G = binding.Graph.__new__(binding.Graph)
    G.L, G.h = L, L.ga_graph_create()
    for nid, seq in nodes:
        assert L.ga_graph_add_bigraph_node(G.h, int(nid), seq.encode(), len(seq)) == 0
    for f, fs, t, te in edges:
        assert L.ga_graph_add_bigraph_edge(G.h, int(f), int(fs), int(t), int(te)) == 0
    for d in set(given_in) | set(given_out):
        i = np.array(given_in.get(d, []), dtype=np.int64)
        o = np.array(given_out.get(d, []), dtype=np.int64)
        assert L.ga_graph_set_neighbors(G.h, d, i.ctypes.data_as(C.c_void_p), len(i), o.ctypes.data_as(C.c_void_p), len(o)) == 0
    assert L.ga_graph_finalize(G.h, 0) == 0 and L.ga_graph_upload(G.h, 0) == 0
    return G


def check_coordinate(G, nodes, edges, given=None, **index):
    """index build (k 11 by default: the small cases have short nodes), topology coordinate, and every node's lin and the statistics
    against the model; the edge rule on the library's own array.  Returns (lin of the library, the model's statistics)."""
    G.build_seed_index(**(index or dict(k=11)))
    st = G.set_seed_coordinate("topology")
    want, stats, parent, lens = scm.of_graph(nodes, edges, given)
    got = G.seed_coordinate()
    assert len(got) == len(want) == 2 * len(nodes) + 2
    bad = np.nonzero(got != np.array(want, dtype=np.int64))[0]
    assert len(bad) == 0, ("lin differs at node index", int(bad[0]), int(got[bad[0]]), want[bad[0]], len(bad))
    assert {k: st[k] for k in STAT_KEYS} == stats, (st, stats)
    assert st == G.seed_coord_stats() and st["build_ms"] >= 0
    assert got[0] == 0 and got[-1] == 0                                        # the dummy nodes
    for v, p in enumerate(parent):
        if p is not None:
            assert got[v] == got[p] + lens[p], ("edge rule", v, p)
    return got, stats


def root_of(parent, v):
    while parent[v] is not None:
        v = parent[v]
    return v


def first_seeds(res):
    return [(s[0] if s else None, sup[0] if sup else None) for s, sup in zip(res.seeds, res.support)]


def mean_first_support(res):
    sup = [s[0] for s in res.support if s]
    return float(np.mean(sup)) if sup else 0.0


def accuracy(nodes, edges, reads, true_seeds, truth, align_lib, seed_lib, coordinate, loci=False, good_true=None, bw=35, **params):
    """the harness of seed_common.accuracy with the coordinate set before the seeds are found (that function builds the index in file
    order, hence the variant here): every read counts in both runs; a read without a seed, failed, or with any other status is absent
    from the predictions, which compare.compare counts as a bad match.  good_true: the figure of an earlier call with
    the same reads, which does not depend on the coordinate"""
    names = ["read%d" % i for i in range(len(reads))]
    sizes = {nid: len(seq) for nid, seq in nodes}
    truth_by_name = {n: t for n, t in zip(names, truth)}
    ga = binding.Graph(nodes, edges, lib_path=align_lib)
    gs = ga if seed_lib == align_lib else binding.Graph(nodes, edges, lib_path=seed_lib)
    st = gs.build_seed_index(coordinate=coordinate)
    cs = gs.seed_coord_stats()
    found = gs.find_seeds(reads, loci=loci, **params)

    def good(seeds):
        have = [i for i in range(len(reads)) if seeds[i]]
        predicted = {}
        if have:
            out = ga.align([reads[i] for i in have], [list(seeds[i]) if isinstance(seeds[i], list) else [seeds[i]] for i in have], bw, flags=0)
            for i, r in zip(have, out):
                if r["status"] == 0 and not r["failed"]:
                    predicted[names[i]] = compare.predicted_nodes(r)
        return compare.compare(truth_by_name, predicted, sizes)["good"]

    good_true = good([[s] for s in true_seeds]) if good_true is None else good_true
    good_own = good(found.seeds)
    sup = [s[0] for s in found.support if s]
    return dict(reads=len(reads), coordinate=coordinate, loci=bool(loci), good_true_seeds=good_true, good_own_seeds=good_own, allowance=max(1, len(reads) // 100),
                reads_without_seed=sum(1 for s in found.seeds if not s), seeds=sum(len(s) for s in found.seeds),
                reads_with_two_seeds=sum(1 for s in found.seeds if len(s) > 1), mean_support=round(float(np.mean(sup)), 2) if sup else 0.0,
                truncated_reads=sum(1 for t in found.truncated if t), index_entries=int(st["entries"]), trees=cs["trees"], cycles_cut=cs["cycles_cut"],
                coord_build_ms=round(cs["build_ms"], 3), seed_kernel_ms=round(found.kernel_ms, 3))
