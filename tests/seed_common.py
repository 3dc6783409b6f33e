"""shared helpers of the seeding tests: the host build of the seeding program, the comparison of a library's index and seeds with the
model of tests/seed_model.py, and the accuracy run (reads aligned from their true seeds against the same reads aligned from the seeds
the library finds, both judged against the simulation's truth by the reference's 0.7 rule)."""
import json
import os

import numpy as np

from graphaligner_amd import binding, compare, synth
import seed_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def big_node_graph(n=100000, seed=9):
    """one node of n bp"""
    return [(1, synth.random_genome(n, seed).tobytes().decode())], []


def check_index(nodes, edges, k, s, lib_path):
    g = binding.Graph(nodes, edges, lib_path=lib_path)
    st = g.build_seed_index(k=k, sample_shift=s)
    keys, idx, offs = g.seed_index_entries()
    want = seed_model.Model(nodes, k, s).entries()
    got = list(zip(keys.tolist(), idx.tolist(), offs.tolist()))
    assert len(got) == len(want), ("entries", len(got), len(want))
    assert got == want
    assert st["entries"] == len(want) and st["distinct_keys"] == len(set(e[0] for e in want))
    assert st["kmers_seen"] == 2 * sum(max(0, len(seq) - k + 1) for _, seq in nodes)
    assert st["k"] == k and st["sample_shift"] == s and st["bytes"] >= 16 * len(want)
    return g, st


def check_reads(g, model, reads, which=None, **params):
    """the library's result for every read (or those in `which`) against the model's"""
    res = g.find_seeds(reads, **params)
    assert len(res.seeds) == len(reads)
    for i in (range(len(reads)) if which is None else which):
        want = model.find(reads[i], **params)
        got = dict(seeds=[(int(n), int(p), bool(r)) for n, p, r in res.seeds[i]], support=res.support[i], n_hits=res.n_hits[i], truncated=res.truncated[i])
        assert got == want, ("read", i, len(reads[i]), got, want)
    return res


def spiked_reads(g, seed=3):
    """reads of the kinds the rule names: both strands, 400 bp to 5 kb; characters outside ACGT; lengths around the 193-bp rule"""
    reads = []
    for n, length, sd in ((6, 400, seed), (6, 1200, seed + 1), (5, 3000, seed + 2), (3, 5000, seed + 3)):
        reads += synth.simulate_reads(g, n, length, seed=sd)[0]
    long = synth.simulate_reads(g, 3, 2500, seed=seed + 4)[0]
    r = long[0]
    reads.append(r[:700] + "N" + r[701:1400] + r[1400:1700].lower() + r[1700:2000] + "NNNN" + r[2004:])
    clean = synth.simulate_reads(g, 1, 2000, sub=0.0, ins=0.0, dele=0.0, seed=seed + 5)[0][0]
    reads += [clean[:150], clean[:385], clean[:386], clean[:10], ""]
    return reads


def accuracy(graph, reads, true_seeds, truth, align_lib, seed_lib, bw=35, **params):
    """every read counts in both runs: a read without a seed, failed, or with any other status is simply absent from the predictions,
    which compare.compare counts as a bad match"""
    names = ["read%d" % i for i in range(len(reads))]
    sizes = {nid: len(seq) for nid, seq in graph.nodes}
    truth_by_name = {n: t for n, t in zip(names, truth)}
    ga = binding.Graph(graph.nodes, graph.edges, lib_path=align_lib)
    gs = ga if seed_lib == align_lib else binding.Graph(graph.nodes, graph.edges, lib_path=seed_lib)
    st = gs.build_seed_index()
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
                reads_without_seed=sum(1 for s in found.seeds if not s), mean_support=round(float(np.mean(sup)), 2) if sup else 0.0,
                truncated_reads=sum(1 for t in found.truncated if t), index_entries=int(st["entries"]), index_bytes=int(st["bytes"]),
                seed_kernel_ms=round(found.kernel_ms, 3))


def record(path, key, row):
    """profiles/<file>.json: one row per case"""
    full = os.path.join(ROOT, "profiles", path)
    data = json.load(open(full)) if os.path.exists(full) else {}
    data[key] = row
    with open(full, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")
