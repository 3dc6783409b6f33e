"""shared helpers of the seeded-batch tests (tests/test_seed_plan.py on the host build of tests/emul, tests/test_seed_plan_gpu.py
on the product library): the host build, graphs made of digraph nodes, the three-way comparison of a seeded batch's plan with the
two-call path's and the model's, and the hand-made inputs for the clauses of the rule."""
import ctypes as C

import numpy as np

from graphaligner_amd import binding, synth
import seed_plan_model as spm

COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def revcomp(s):
    return "".join(COMP[c] for c in reversed(s))


def text(a):
    return a.tobytes().decode()


class DigraphGraph(binding.Graph):
    """a graph of digraph nodes given one by one (ga_graph_add_node): [(digraph id, sequence)], edges [(from id, to id)]"""

    def __init__(self, dnodes, dedges=(), overlap=0, lib_path=None, device=0):
        self.L = binding.load(lib_path)
        self.h = self.L.ga_graph_create()
        for did, seq in dnodes:
            binding._check(self.L, self.L.ga_graph_add_node(self.h, int(did), seq.encode(), len(seq), int(did) & 1), "ga_graph_add_node")
        for f, t in dedges:
            binding._check(self.L, self.L.ga_graph_add_edge(self.h, int(f), int(t)), "ga_graph_add_edge")
        binding._check(self.L, self.L.ga_graph_finalize(self.h, overlap), "ga_graph_finalize")
        binding._check(self.L, self.L.ga_graph_upload(self.h, device), "ga_graph_upload")


def rows(a):
    return [tuple(int(v) for v in r) for r in a.tolist()]


def plain_seeds(res):
    return (res.seeds, res.support, res.n_hits, res.truncated, res.locus_hits, res.locus_span, res.n_loci)


def check_plan(G, dnodes, overlap, reads, loci=False, bw=35, **params):
    """the plan of a seeded batch against the two-call path's and the model's, field by field, and its seeds against find_seeds';
    returns (plan of the seeded batch, the seeds)"""
    found = G.find_seeds(reads, loci=loci, **params)
    seeded = G.prepare_seeded(reads, params, loci, bw)
    two = G.prepare(reads, found.seeds, bw)
    try:
        assert plain_seeds(seeded.seeds()) == plain_seeds(found)
        a, b = seeded.plan(), two.plan()
        want = spm.plan(dnodes, overlap, reads, found.seeds)
        for kind in ("jobs", "seeds", "fills"):
            assert a[kind].dtype == b[kind].dtype
            assert rows(a[kind]) == rows(b[kind]), (kind, "seeded batch against the two-call path")
            assert rows(a[kind]) == want[kind], (kind, "against the model")
        st = seeded.prepare_stats()
        assert st["n_seeds"] == len(want["seeds"]) and st["n_jobs"] == len(want["jobs"])
        assert st["reads_without_seed"] == sum(1 for s in found.seeds if not s)
        return a, found
    finally:
        seeded.close()
        two.close()


def same_results(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        for key in ("status", "failed", "score", "mappings", "alignment_start", "alignment_end", "query_position"):
            assert x[key] == y[key], (i, key, x[key], y[key])
        assert np.array_equal(x["trace"], y["trace"]), i


def check_results(G, reads, loci=False, bw=35, flags=0, **params):
    """align_reads against align over find_seeds, read for read; returns the results"""
    found = G.find_seeds(reads, loci=loci, **params)
    got = G.align_reads(reads, params, loci, bw, flags=flags)
    want = G.align(reads, found.seeds, bw, flags=flags)
    same_results(got, want)
    return got, found


def mixed_reads(g, n, length=3000, seed=5):
    """n reads of the graph with reads that get no seed at the first, the middle and the last place: one of 300 bp and one of random
    sequence"""
    reads = synth.simulate_reads(g, n, length, seed=seed)[0]
    short = reads[0][:300]
    alien = text(synth.random_genome(length, 991))
    return [short] + reads[:n // 2] + [alien, short] + reads[n // 2:] + [alien]


# ---- hand-made graphs ------------------------------------------------------------------------------------------------------------------
def strand_graph():
    """three pieces of random sequence, 2 kb each, as digraph nodes: a proper pair (ids 2, 3), a node with one strand only (id 4) and a
    pair whose reverse strand is 100 bp short (ids 6, 7).  Returns (digraph nodes, the three forward sequences)."""
    a, b, c = (text(synth.random_genome(2000, s)) for s in (41, 42, 43))
    return [(2, a), (3, revcomp(a)), (4, b), (6, c), (7, revcomp(c)[:1900])], (a, b, c)


def star_read(G, read, where, overlap=0, **params):
    """`read` with a character that has no complement at where(p), p being the read's seed position AFTER the change (the change moves
    the k-mers, so the place is searched for); returns (the read, p)"""
    p = G.find_seeds([read], **params).seeds[0][0][1]
    for _ in range(12):
        at = where(p)
        changed = read[:at] + "*" + read[at + 1:]
        got = G.find_seeds([changed], **params).seeds[0]
        if got and where(got[0][1]) == at:
            return changed, got[0][1]
        assert got, "the changed read lost its seed"
        p = got[0][1]
    raise AssertionError("no place for the character")


def overlap_graph(ovl):
    """6 kb of random sequence as three bigraph nodes whose ends overlap by ovl"""
    a = text(synth.random_genome(6000, 51))
    return [(1, a[:2000 + ovl]), (2, a[2000:4000 + ovl]), (3, a[4000:])], [(1, 0, 2, 0), (2, 0, 3, 0)], a


# name -> (place of the character given the seed position p, the graph's overlap, whether the seed still gets its jobs)
STAR_CASES = {"star-at-0": (lambda p: 0, 0, False), "star-before-seed": (lambda p: p // 2, 0, False), "star-at-p+ovl-1": (lambda p: p - 1, 0, False),
              "star-at-p+ovl-1-overlap16": (lambda p: p + 15, 16, False), "star-at-p+ovl-overlap16": (lambda p: p + 16, 16, True),
              "star-behind-seed": (lambda p: p + 300, 0, True)}


def check_star_case(G, dnodes, ovl, clean, where, jobs_made):
    """clean[0] with the character, followed by clean[1]: plan three ways, the clause's own outcome, and the results"""
    read, p = star_read(G, clean[0], where, max_seeds=1)
    plan, found = check_plan(G, dnodes, ovl, [read, clean[1]], max_seeds=1)
    alone, _ = check_plan(G, dnodes, ovl, [clean[1]], max_seeds=1)
    first = rows(plan["seeds"])[0]
    assert first[0] == p and read[where(p)] == "*"
    if jobs_made:
        assert first[2:] == (spm.OK, 1, 0, 1) and len(plan["jobs"]) == 4
        assert rows(plan["jobs"])[2][0] == rows(plan["jobs"])[0][1] + rows(plan["jobs"])[1][1]
    else:
        # GA_S_ASSERTION, no jobs for that seed, and the next read's jobs lie where they lie without it
        assert first[2:] == (spm.ASSERTION, 0, -1, -1)
        assert rows(plan["jobs"]) == rows(alone["jobs"]) and [f[1:] for f in rows(plan["fills"])] == [f[1:] for f in rows(alone["fills"])]
    got, _ = check_results(G, [read, clean[1]], max_seeds=1)
    if not jobs_made:
        assert got[0]["status"] == spm.ASSERTION
    assert got[1]["status"] == 0 and not got[1]["failed"]
