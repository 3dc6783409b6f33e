"""shared helpers of the seeds-per-locus tests (tests/test_seed_loci.py on the host build, tests/test_seed_loci_gpu.py on the product
library): the host build, the comparison of Graph.find_seeds(loci=True) with the model of tests/seed_loci_model.py, the hand-made
cases of the rule (zigzag, gap, repeat) and the accuracy run of seed_common.accuracy with grouped seeds."""

import numpy as np

from graphaligner_amd import binding, compare, synth
import seed_loci_model

PARAM_SETS = (dict(), dict(max_seeds=1), dict(max_seeds=3), dict(max_hits=16), dict(min_support=1, window=100, diag_tol=5), dict(max_occ=1))


def as_dict(res, i):
    return dict(seeds=[(int(n), int(p), bool(r)) for n, p, r in res.seeds[i]], support=res.support[i], locus_hits=res.locus_hits[i],
                locus_span=res.locus_span[i], n_loci=res.n_loci[i], n_hits=res.n_hits[i], truncated=res.truncated[i])


def check_reads(g, model, reads, which=None, **params):
    """the library's grouped result for every read (or those in `which`) against the model's: seeds, support, the three locus fields,
    n_loci, n_hits, truncated"""
    res = g.find_seeds(reads, loci=True, **params)
    assert len(res.seeds) == len(reads) == len(res.n_loci)
    for i in (range(len(reads)) if which is None else which):
        want, _ = seed_loci_model.find_loci(model, reads[i], **params)
        got = as_dict(res, i)
        assert got == want, ("read", i, len(reads[i]), got, want)
        assert len(got["seeds"]) <= got["n_loci"]
    return res


def plain(res):
    """everything a result carries but the kernel's time"""
    return (res.seeds, res.support, res.n_hits, res.truncated, res.locus_hits, res.locus_span, res.n_loci)


def text(a):
    return a.tobytes().decode()


# ---- hand-made cases ----------------------------------------------------------------------------------------------------------------
ZIGZAG_T = 20
ZIGZAG_PARAMS = dict(k=11, sample_shift=0, min_support=1, diag_tol=ZIGZAG_T)


def zigzag_case():
    """One node of random sequence G and error-free reads made of pieces of it; a piece at read position r on diagonal d is
    G[x + r + d : ...], so all its k-mers hit that diagonal.  Read 0: piece A on diagonal 0, then B on 2T, then C on T, with diag_tol = T
    and the whole read inside one window: A and B are not linked, A-C and C-B are.  Read 1: six pieces on 0, 2T, ..., 10T and then
    the connectors on 9T, 7T, ..., T, the lowest last: the smallest label reaches the pieces one per hook, through hits that come
    later in the read.  Returns (nodes, reads, params, per read the number of k-mers inside its pieces)."""
    T = ZIGZAG_T
    G = text(synth.random_genome(20000, 17))

    def build(x, diags, piece):
        out, r = [], 0
        for d in diags:
            out.append(G[x + r + d:x + r + d + piece])
            r += piece
        return "".join(out), len(diags) * (piece - 11 + 1)

    a, na = build(5000, [0, 2 * T, T], 250)
    b, nb = build(9000, [0, 2 * T, 4 * T, 6 * T, 8 * T, 10 * T, 9 * T, 7 * T, 5 * T, 3 * T, T], 60)
    return [(1, G)], [a, b], ZIGZAG_PARAMS, [na, nb]


def check_zigzag(res, reads, inside):
    for i, r in enumerate(reads):
        # the read's own pieces are one locus, from its first k-mer to its last; chance hits elsewhere are loci of their own
        assert res.seeds[i] and res.locus_hits[i][0] >= inside[i], (i, res.locus_hits[i], inside[i])
        assert res.locus_hits[i][0] <= res.n_hits[i] and res.locus_span[i][0] == (0, len(r) - 11), (i, res.locus_span[i])
        assert all(n < inside[i] // 10 for n in res.locus_hits[i][1:]), (i, res.locus_hits[i])


def gap_case():
    """an error-free read with 1 500 random bases in its middle: two loci on one diagonal, more than `window` apart"""
    gen = synth.random_genome(30000, 5)
    G = text(gen)
    g = synth.SynthGraph(gen, node_len=64)
    a = 3000
    read = G[a:a + 700] + text(synth.random_genome(1500, 99)) + G[a + 2200:a + 2900]
    return g, [read]


def check_gap(res):
    assert res.n_loci[0] == 2 and len(res.seeds[0]) == 1, (res.n_loci, res.seeds)
    assert res.locus_span[0][0][1] - res.locus_span[0][0][0] < 700


def repeat_case():
    """a genome with a 2.5 kb segment inserted a second time; reads through the first copy, through the second, and inside the repeat"""
    gen = synth.random_genome(30000, 5)
    gen = np.concatenate([gen[:14000], gen[8000:10500], gen[14000:]])
    g = synth.SynthGraph(gen, node_len=64)
    reads = []
    for n, (lo, hi) in enumerate(((7000, 12000), (12500, 17500), (8200, 10200))):
        reads.append(text(synth.add_errors(gen[lo:hi], 0.04, 0.04, 0.04, np.random.default_rng(50 + n))))
    return g, reads


def check_repeat(res):
    for i in range(3):
        assert len(res.seeds[i]) == 2 and min(res.locus_hits[i]) >= 100 and res.locus_hits[i][0] >= res.locus_hits[i][1], (i, res.locus_hits[i])


# ---- usability ------------------------------------------------------------------------------------------------------------------------
def accuracy(graph, reads, true_seeds, truth, align_lib, seed_lib, bw=35, **params):
    """the harness of seed_common.accuracy with grouped seeds (that function calls find_seeds without `loci`, hence the variant here):
    every read counts in both runs; a read without a seed, failed, or with any other status is absent from the predictions, which
    compare.compare counts as a bad match.  The ungrouped call on the same index is made too, for the number of seeds it gives."""
    names = ["read%d" % i for i in range(len(reads))]
    sizes = {nid: len(seq) for nid, seq in graph.nodes}
    truth_by_name = {n: t for n, t in zip(names, truth)}
    ga = binding.Graph(graph.nodes, graph.edges, lib_path=align_lib)
    gs = ga if seed_lib == align_lib else binding.Graph(graph.nodes, graph.edges, lib_path=seed_lib)
    st = gs.build_seed_index()
    ungrouped = gs.find_seeds(reads, **params)
    found = gs.find_seeds(reads, loci=True, **params)

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
    size = [s[0] for s in found.locus_hits if s]
    return dict(reads=len(reads), good_true_seeds=good_true, good_own_seeds=good_own, allowance=max(1, len(reads) // 100),
                reads_without_seed=sum(1 for s in found.seeds if not s), seeds=sum(len(s) for s in found.seeds),
                seeds_ungrouped=sum(len(s) for s in ungrouped.seeds), reads_with_two_seeds=sum(1 for s in found.seeds if len(s) > 1),
                reads_with_two_seeds_ungrouped=sum(1 for s in ungrouped.seeds if len(s) > 1), loci_with_candidate=sum(found.n_loci),
                mean_hits_of_first_locus=round(float(np.mean(size)), 2) if size else 0.0, truncated_reads=sum(1 for t in found.truncated if t),
                index_entries=int(st["entries"]), seed_kernel_ms=round(found.kernel_ms, 3), seed_kernel_ms_ungrouped=round(ungrouped.kernel_ms, 3))
