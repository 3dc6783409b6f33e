"""The seeding rule in plain Python (include/graphaligner_amd.h, "seeds found on the device"): a dict from key
to the list of its entries, Python integers throughout.  Written from the text of the rule; it shares no code with
graphaligner_amd/csrc/ga_seed.h and is what the tests compare the library with, entry for entry and seed for seed."""
import bisect

MASK64 = (1 << 64) - 1
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
DEFAULTS = dict(k=15, sample_shift=2, max_occ=8, max_hits=4096, window=1024, diag_tol=64, min_support=2, max_seeds=2)
MIN_ARM = 193


def mix(x):
    x ^= x >> 29
    x = (x * 0x9E3779B97F4A7C15) & MASK64
    x ^= x >> 32
    return x & 0xFFFFFFFF


def kept_kmers(seq, k, s):
    """(position, key) of every kept k-mer of a string; a character outside ACGT breaks the k-mers that contain it"""
    out = []
    mask = (1 << (2 * k)) - 1
    low = (1 << s) - 1
    key = 0
    run = 0                       # valid characters in a row up to here
    for i, ch in enumerate(seq):
        c = CODE.get(ch)
        if c is None:
            run = 0
            key = 0
            continue
        key = ((key << 2) | c) & mask
        run += 1
        if run >= k and (mix(key) & low) == 0:
            out.append((i + 1 - k, key))
    return out


class Model:
    def __init__(self, nodes, k=15, sample_shift=2):
        """nodes: [(bigraph id, sequence)] in the order they were added (distinct ids).  Node indices are the library's: 0 is the dummy
        start node, bigraph node number i is 1 + 2i (forward, digraph id 2 id) and 2 + 2i (reverse complement, digraph id 2 id + 1)."""
        self.k, self.s = k, sample_shift
        self.digraph_id = {}
        self.lin = {}
        self.index = {}
        cum = 0
        for i, (nid, seq) in enumerate(nodes):
            rc = "".join(COMP[c] for c in reversed(seq))
            for index, did, text in ((1 + 2 * i, 2 * nid, seq), (2 + 2 * i, 2 * nid + 1, rc)):
                self.digraph_id[index] = did
                self.lin[index] = cum if did % 2 == 0 else -(cum + len(seq) - 1)
                for o, key in kept_kmers(text, k, sample_shift):
                    self.index.setdefault(key, []).append((index, o))       # (node index, offset) ascending by construction
            cum += len(seq)

    def entries(self):
        """[(key, node index, offset)] ordered by (key, node index, offset)"""
        return [(key, n, o) for key in sorted(self.index) for n, o in self.index[key]]

    def find(self, read, **params):
        P = dict(DEFAULTS, k=self.k, sample_shift=self.s)
        P.update(params)
        assert P["k"] == self.k and P["sample_shift"] == self.s
        L = len(read)
        hits = []                                                           # (p, node index, o), in (p, index order) order
        for p, key in kept_kmers(read, self.k, self.s):
            ent = self.index.get(key, ())
            if 1 <= len(ent) <= P["max_occ"]:
                hits.extend((p, n, o) for n, o in ent)
        truncated = len(hits) > P["max_hits"]
        hits = hits[:P["max_hits"]]
        ps = [h[0] for h in hits]
        strand = [self.digraph_id[n] & 1 for _, n, _ in hits]
        diag = [self.lin[n] + o - p for p, n, o in hits]
        support = []
        for i, (p, n, o) in enumerate(hits):
            lo, hi = bisect.bisect_left(ps, p - P["window"]), bisect.bisect_right(ps, p + P["window"])
            support.append(sum(1 for j in range(lo, hi) if strand[j] == strand[i] and abs(diag[j] - diag[i]) <= P["diag_tol"]))
        cand = [i for i, (p, n, o) in enumerate(hits) if p >= MIN_ARM and L - p >= MIN_ARM and support[i] >= P["min_support"]]
        cand.sort(key=lambda i: (-support[i], hits[i][0], hits[i][1], hits[i][2]))
        taken = []
        for i in cand:
            if len(taken) >= P["max_seeds"]:
                break
            if any(strand[t] == strand[i] and abs(diag[t] - diag[i]) <= P["diag_tol"] for t in taken):
                continue
            taken.append(i)
        return dict(seeds=[(self.digraph_id[hits[i][1]] >> 1, hits[i][0], bool(self.digraph_id[hits[i][1]] & 1)) for i in taken],
                    support=[support[i] for i in taken], n_hits=len(hits), truncated=truncated)
