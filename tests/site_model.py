"""The rule of site queries (include/graphaligner_amd.h: "pileup sites") in numpy, independent of the device source: whole-array
arithmetic over the planes, no tiles, rounds or scans.

sites(planes, kind, params, ...) -> (entries, F) with entries ascending (all of them: `total` is len(entries); the caller cuts at
max_sites) and F the folded counts as an (n, 8) uint32 array.

  planes      (K, entries) uint32, K = 8 for "bases", 1 for "depth" and "edges"
  node_start  (n_nodes + 1,) first column of every node (the two dummy nodes included) and the column count    [columns kinds, fold]
  twin        (n_nodes,) the node index of the other strand, < 0 or >= n_nodes for none                          [columns kinds, fold]
  forward     (n_nodes,) bool: the node's digraph id is even and it is no dummy node                             [columns kinds, fold]
  mirror      (entries,) the mirror slot of every slot, >= entries (0xffffffff) for none                         [edges, fold]
"""
import numpy as np


def tables_of_graph(ids, node_lens):
    """node_start, twin, forward of a finalized graph from its nodes' digraph ids in index order (dummy nodes first and last, id 0)"""
    ids = [int(i) for i in ids]
    n = len(ids)
    node_start = np.concatenate([[0], np.cumsum(np.asarray(node_lens, dtype=np.int64))]).astype(np.int64)
    index = {ids[k]: k for k in range(1, n - 1)}
    twin = np.full(n, -1, dtype=np.int64)
    forward = np.zeros(n, dtype=bool)
    for k in range(1, n - 1):
        twin[k] = index.get(ids[k] ^ 1, -1)
        forward[k] = ids[k] % 2 == 0
    return node_start, twin, forward


def folded(planes, kind, fold, first, n, node_start=None, twin=None, forward=None, mirror=None):
    """(candidate entries, F) over the range"""
    planes = np.asarray(planes, dtype=np.uint32)
    K, entries = planes.shape
    assert K == (8 if kind == "bases" else 1)
    e = np.arange(first, first + n, dtype=np.int64)
    F = np.zeros((len(e), 8), dtype=np.uint32)
    if not fold:
        F[:, :K] = planes[:, e].T
        return e, F
    if kind == "edges":
        m = np.asarray(mirror, dtype=np.int64)[e]
        none = (m < 0) | (m >= entries)
        keep = none | (e <= m)
        e, m, none = e[keep], m[keep], none[keep]
        F = np.zeros((len(e), 8), dtype=np.uint32)
        add = ~none & (m != e)
        partner = np.where(add, planes[0, np.where(add, m, 0)], 0).astype(np.uint32)
        F[:, 0] = planes[0, e] + partner                       # (uint32: wraps)
        return e, F
    node_start = np.asarray(node_start, dtype=np.int64)
    node = np.searchsorted(node_start, e, side="right") - 1
    tw = np.asarray(twin, dtype=np.int64)[node]
    keep = np.asarray(forward, dtype=bool)[node] & (tw >= 0) & (tw < len(node_start) - 1)
    e, node, tw = e[keep], node[keep], tw[keep]
    length = node_start[node + 1] - node_start[node]
    c2 = node_start[tw] + length - 1 - (e - node_start[node])
    F = np.zeros((len(e), 8), dtype=np.uint32)
    if kind == "depth":
        F[:, 0] = planes[0, e] + planes[0, c2]
        return e, F
    partner_plane = [0, 4, 3, 2, 1, 5, 6, 7]
    for p in range(8):
        F[:, p] = planes[p, e] + planes[partner_plane[p], c2]
    return e, F


def select(F, kind, min_depth, min_alt, alt_num, alt_den):
    """the flag of every candidate, in Python integers where 64 bits could be left"""
    F64 = F.astype(np.uint64)
    if kind == "bases":
        D = F64[:, :7].sum(axis=1)
        X = np.maximum(D - F64[:, 0], F64[:, 7])
    else:
        D = F64[:, 0]
        X = np.zeros_like(D)
    # (X * alt_den < 2^35 * 2^16 and alt_num * D likewise: inside uint64)
    return (D >= np.uint64(min_depth)) & (X >= np.uint64(min_alt)) & (X * np.uint64(alt_den) >= np.uint64(alt_num) * D)


def sites(planes, kind, fold=True, min_depth=1, min_alt=0, alt_frac=(0, 1), first=0, n=None, node_start=None, twin=None, forward=None, mirror=None):
    planes = np.asarray(planes, dtype=np.uint32)
    n = planes.shape[1] - first if n is None else n
    e, F = folded(planes, kind, fold, first, n, node_start, twin, forward, mirror)
    ok = select(F, kind, min_depth, min_alt, alt_frac[0], alt_frac[1])
    return e[ok], F[ok]


def both_strands(planes, kind, entries, node_start=None, twin=None, mirror=None):
    """of the given fold sites: does each have a non-zero count from both strands (columns: the column and its partner; edges: the slot
    and its mirror)"""
    planes = np.asarray(planes, dtype=np.uint32)
    e = np.asarray(entries, dtype=np.int64)
    if kind == "edges":
        m = np.asarray(mirror, dtype=np.int64)[e]
        has = (m >= 0) & (m < planes.shape[1]) & (m != e)
        return has & (planes[0, e] > 0) & (planes[0, np.where(has, m, 0)] > 0)
    node_start = np.asarray(node_start, dtype=np.int64)
    node = np.searchsorted(node_start, e, side="right") - 1
    tw = np.asarray(twin, dtype=np.int64)[node]
    c2 = node_start[tw] + (node_start[node + 1] - node_start[node]) - 1 - (e - node_start[node])
    return (planes[:, e].sum(axis=0) > 0) & (planes[:, c2].sum(axis=0) > 0)
