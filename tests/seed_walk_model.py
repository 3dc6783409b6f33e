"""The walk index in plain Python (include/graphaligner_amd.h, "seeds found on the device": ga_graph_build_seed_index_walks; DESIGN.md
section 10): strings and Python integers throughout, the walks of a tail start by recursion over out-neighbours.  Written from the text
of the rule; it takes `mix`, `kept_kmers` and `Model.find` from tests/seed_model.py (the lookup and the ranking do not change) and
shares no code with graphaligner_amd/csrc/ga_seed.h."""
import seed_model
from seed_model import CODE, COMP, mix


def key_of(text):
    key = 0
    for ch in text:
        key = (key << 2) | CODE[ch]
    return key


class WalkModel(seed_model.Model):
    def __init__(self, nodes, edges, k=15, sample_shift=2, max_walks=64):
        """nodes: [(bigraph id, sequence)] in the order they were added; edges: [(from, from is reversed, to, to is reversed)].
        Node indices as in seed_model.Model: bigraph node number i is 1 + 2i forward and 2 + 2i reverse (the dummy nodes, index 0 and
        the last one, have no edges and do not appear here)."""
        super().__init__([], k, sample_shift)
        self.max_walks = max_walks
        text, index_of = {}, {}
        cum = 0
        for i, (nid, seq) in enumerate(nodes):
            rc = "".join(COMP[c] for c in reversed(seq))
            for index, did, t in ((1 + 2 * i, 2 * nid, seq), (2 + 2 * i, 2 * nid + 1, rc)):
                text[index] = t
                index_of[did] = index
                self.digraph_id[index] = did
                self.lin[index] = cum if did % 2 == 0 else -(cum + len(seq) - 1)
            cum += len(seq)
        # a bigraph edge is two digraph edges: right end of `from` -> right end of `to`, and the mirrored one
        out = {index: [] for index in text}
        for f, f_rev, t, t_rev in edges:
            for a, b in ((2 * f + int(bool(f_rev)), 2 * t + int(bool(t_rev))), (2 * t + 1 - int(bool(t_rev)), 2 * f + 1 - int(bool(f_rev)))):
                a, b = index_of[a], index_of[b]
                if b not in out[a]:
                    out[a].append(b)
        self.text, self.out = text, out
        low = (1 << sample_shift) - 1
        triples = set()
        self.stats = dict(max_walks=max_walks, tail_starts=0, tail_starts_skipped=0, walk_kmers=0, duplicates_dropped=0)
        self.in_node_kmers = 0
        kept_before_dedup = 0
        for index in sorted(text):
            t = text[index]
            for o in range(len(t)):
                if o + k <= len(t):
                    self.in_node_kmers += 1
                    kmers = [t[o:o + k]]
                else:
                    self.stats["tail_starts"] += 1
                    kmers = []
                    self._walks(t[o:], index, kmers)
                    if len(kmers) > max_walks:
                        self.stats["tail_starts_skipped"] += 1
                        continue
                    self.stats["walk_kmers"] += len(kmers)
                for kmer in kmers:
                    key = key_of(kmer)
                    if (mix(key) & low) == 0:
                        kept_before_dedup += 1
                        triples.add((key, index, o))
        self.stats["duplicates_dropped"] = kept_before_dedup - len(triples)
        self.kmers_seen = self.in_node_kmers + self.stats["walk_kmers"]
        for key, index, o in sorted(triples):
            self.index.setdefault(key, []).append((index, o))

    def _walks(self, prefix, node, found):
        """the k-base texts of the walks that begin with `prefix` and go on behind `node`; gives up beyond max_walks + 1 (the start is
        skipped then, whatever the exact number)"""
        for m in self.out[node]:
            if len(found) > self.max_walks:
                return
            t = self.text[m]
            if len(t) == 0:
                continue
            need = self.k - len(prefix)
            if len(t) >= need:
                found.append(prefix + t[:need])
            else:
                self._walks(prefix + t, m, found)
