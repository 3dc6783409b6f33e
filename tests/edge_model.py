"""Edge support: which graph edges the alignments cross.  THE RULE, over the TraceItem lists alone (the lists GA_F_TRACE returns): take the
list of a read with status 0 that did not fail and cut it at the SPLIT item into parts.  For every two consecutive items a, b of one part
let da = 2 * a.node_id + a.reverse and db = 2 * b.node_id + b.reverse, and count one for the directed edge da -> db when b's column is
not a's column, b is not the next offset of the same digraph node, neither item lies on a dummy node, and the edge exists in the graph.
Edges are per strand, like the columns of a pileup: a backward part counts on the other strand's edge, and binding.fold_edge_support sums
an edge with its mirror, which is the quantity the reference's SupportedSubgraph thresholds at >= 1.  What follows from the rule: the
first cell of each part has no item, so a crossing out of that cell, or across the SPLIT, is not counted (up to three per read); a turn
through a self-loop on a one-base node stays in its column and is not counted.
This module holds the rule over the oracle's lists, a graph's slot table (its in-neighbour lists laid end to end) built from `nodes` /
`edges` alone, and the fold; tests/test_edge_support.py holds them against the mappings of the same oracle results.  A pileup kind
that sums these counts on the device is not in the tree: this is the model such a kind is to be checked against."""
import numpy as np

import ops_model as om
import pileup_model as pm


# ---- the slot table ---------------------------------------------------------------------------------------------------------------
def slot_table(node_ids, edges):
    """[(from digraph id, to digraph id)] per slot: the in-neighbour lists of the finalized graph laid end to end, in node-index order
    (a bigraph node is its forward copy, then its reverse copy; a repeated id is ignored) and then in the order the edges were added, a
    repeated edge kept once.  A bigraph edge (from, from_start, to, to_end) is the two digraph edges of BigraphToDigraph.cpp:32-56"""
    order, in_lists = [], {}
    for nid in node_ids:
        for d in (2 * int(nid), 2 * int(nid) + 1):
            if d not in in_lists:
                in_lists[d] = []
                order.append(d)

    def add(f, t):
        if f not in in_lists[t]:
            in_lists[t].append(f)

    for f, fs, t, te in edges:
        f, t = int(f), int(t)
        from_left, from_right = (2 * f, 2 * f + 1) if fs else (2 * f + 1, 2 * f)
        to_left, to_right = (2 * t, 2 * t + 1) if te else (2 * t + 1, 2 * t)
        add(from_right, to_right)
        add(to_left, from_left)
    return [(f, d) for d in order for f in in_lists[d]]


# ---- the rule over the oracle's lists ---------------------------------------------------------------------------------------------
def crossings_of(ora, graph_bp, edge_set):
    """the directed edges (da, db) one read counts, one entry per count, in list order"""
    if ora["status"] != 0 or ora["failed"]:
        return []
    t = ora["trace"]
    dummy = pm.dummy_items(ora, graph_bp)
    out = []
    for i in range(1, len(t)):
        a, b = t[i - 1], t[i]
        if int(a[4]) == om.SPLIT or int(b[4]) == om.SPLIT:
            continue                                        # (the parts are cut at the SPLIT item: nothing is counted across it)
        da, db = 2 * int(a[0]) + int(bool(a[2])), 2 * int(b[0]) + int(bool(b[2]))
        if da == db and int(a[1]) == int(b[1]):
            continue                                        # the same column
        if da == db and int(b[1]) == int(a[1]) + 1:
            continue                                        # the next offset of the same node
        if dummy[i - 1] or dummy[i]:
            continue
        if edge_set is not None and (da, db) not in edge_set:
            continue                                        # (edge_set None: every pair the other conditions select)
        out.append((da, db))
    return out


class Model:
    """counts per directed edge (from digraph id, to digraph id); `items` = everything counted; per read its count"""

    def __init__(self, slots):
        self.slots = list(slots)
        self.edge_set = set(self.slots)
        self.counts = {}
        self.items = 0
        self.reads = 0
        self.per_read = []

    def add(self, ora, graph_bp, times=1):
        if ora["status"] != 0 or ora["failed"]:
            self.per_read.append(None)
            return
        self.reads += 1
        got = crossings_of(ora, graph_bp, self.edge_set)
        for e in got:
            self.counts[e] = self.counts.get(e, 0) + times
        self.items += times * len(got)
        self.per_read.append(len(got))

    def plane(self):
        """the counts per slot"""
        return np.array([self.counts.get(e, 0) for e in self.slots], dtype=np.int64)


def of(oras, graph_bp, slots, times=1):
    m = Model(slots)
    for o in oras:
        m.add(o, graph_bp, times)
    return m


def fold(slots, counts):
    """per bidirected edge -- a directed edge a -> b and its mirror b ^ 1 -> a ^ 1 under one key, the smaller of the two pairs -- the
    summed counts: what fold_edge_support of the binding must return"""
    out = {}
    for (a, b), c in zip(slots, counts):
        key = min((int(a), int(b)), (int(b) ^ 1, int(a) ^ 1))
        out[key] = out.get(key, 0) + int(c)
    return out
