"""One seed per locus in plain Python (include/graphaligner_amd.h, "one seed per locus"): the read's hits as
tests/seed_model.py defines them, an ordinary union-find over the link relation, dicts and sorts for the rest.  Written from the text
of the rule over a seed_model.Model or a seed_walk_model.WalkModel (their .index, .lin, .digraph_id and kept_kmers); it shares no code
with graphaligner_amd/csrc/ga_seed.h and is what the tests compare ga_find_seeds_loci with, field for field."""
import bisect

from seed_model import DEFAULTS, MIN_ARM, kept_kmers


def hits_of(model, read, P):
    """[(p, node index, offset)] in (p, index order) order, cut at max_hits; whether it was cut"""
    hits = []
    for p, key in kept_kmers(read, model.k, model.s):
        ent = model.index.get(key, ())
        if 1 <= len(ent) <= P["max_occ"]:
            hits.extend((p, n, o) for n, o in ent)
    return hits[:P["max_hits"]], len(hits) > P["max_hits"]


def find_loci(model, read, **params):
    """what Graph.find_seeds(read, loci=True, **params) must return for this read, and `loci`: every locus as (hits, first p, last p,
    seed hit or None), for the tests that look at loci that gave no seed"""
    P = dict(DEFAULTS, k=model.k, sample_shift=model.s)
    P.update(params)
    assert P["k"] == model.k and P["sample_shift"] == model.s
    L = len(read)
    hits, truncated = hits_of(model, read, P)
    H = len(hits)
    ps = [h[0] for h in hits]
    strand = [model.digraph_id[n] & 1 for _, n, _ in hits]
    diag = [model.lin[n] + o - p for p, n, o in hits]

    def linked(i, j):
        return strand[i] == strand[j] and abs(ps[i] - ps[j]) <= P["window"] and abs(diag[i] - diag[j]) <= P["diag_tol"]

    parent = list(range(H))

    def root(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    support = [0] * H
    for i in range(H):
        lo, hi = bisect.bisect_left(ps, ps[i] - P["window"]), bisect.bisect_right(ps, ps[i] + P["window"])
        for j in range(lo, hi):
            if j == i or linked(i, j):
                support[i] += 1                                        # (the hit itself counts)
                if j != i:
                    parent[root(i)] = root(j)
    members = {}
    for i in range(H):
        members.setdefault(root(i), []).append(i)
    order = lambda i: (-support[i], hits[i][0], hits[i][1], hits[i][2])
    loci = []
    for m in members.values():
        cand = [i for i in m if hits[i][0] >= MIN_ARM and L - hits[i][0] >= MIN_ARM and support[i] >= P["min_support"]]
        loci.append(dict(hits=len(m), first_p=min(ps[i] for i in m), last_p=max(ps[i] for i in m), seed=min(cand, key=order) if cand else None))
    with_seed = [c for c in loci if c["seed"] is not None]
    with_seed.sort(key=lambda c: (-c["hits"],) + order(c["seed"]))
    taken = []
    for c in with_seed:
        if len(taken) >= P["max_seeds"]:
            break
        i = c["seed"]
        if any(strand[t["seed"]] == strand[i] and abs(diag[t["seed"]] - diag[i]) <= P["diag_tol"] for t in taken):
            continue
        taken.append(c)
    ids = [model.digraph_id[hits[c["seed"]][1]] for c in taken]
    return dict(seeds=[(d >> 1, hits[c["seed"]][0], bool(d & 1)) for d, c in zip(ids, taken)],
                support=[support[c["seed"]] for c in taken], locus_hits=[c["hits"] for c in taken],
                locus_span=[(c["first_p"], c["last_p"]) for c in taken], n_loci=len(with_seed), n_hits=H, truncated=truncated), loci
