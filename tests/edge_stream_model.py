"""An independent replay of a move stream over a small graph given as in-lists, for the fabricated streams of tests/test_edge_pileup.py:
what a pileup of kind "edges" must count for one job.  Nothing here is the kernel's walk: the cells are stepped one move at a time the
way the host steps a traceback (one move takes a cell to its predecessor), laid out as the final trace of the part -- a forward job's
back to front, a backward job's in stream order on the mirror cells --, the first cell dropped because it has no item, and then the rule
of edge_model.py is applied to consecutive items: two columns, not the next offset of the same node, no dummy node, an edge of the graph.

A graph is (node_len, in_lists, twin): node 0 and the last node are the two dummy nodes (one column, no edges); in_lists[k] are node k's
in-neighbours in order; twin[k] is the node of the other strand or NONE.  The slot of the edge f -> t is sum(len(in_lists[:t])) + place."""
import numpy as np

import ops_model as om

NONE = 0xFFFFFFFF


def one_strand(node_lens, edges):
    """a graph whose other strand was never added (the digraph-level calls with one id of each pair): node i is index 1 + i, every twin
    is NONE, so a backward job has no mirror cell anywhere and counts nothing"""
    n = len(node_lens) + 2
    in_lists = [[] for _ in range(n)]
    for i, j in edges:
        if 1 + i not in in_lists[1 + j]:
            in_lists[1 + j].append(1 + i)
    return [1] + [int(x) for x in node_lens] + [1], in_lists, [NONE] * n


def doubled(node_lens, edges, drop_mirror_of=(), no_twin_of=()):
    """the two strands of a graph of `node_lens` (node i's length) and `edges` (i, j): node i's forward copy is index 1 + 2 * i, its
    reverse copy 2 + 2 * i, and an edge i -> j is also the edge j' -> i' between the reverse copies -- but for the edges listed in
    drop_mirror_of, whose mirror edge is left out (a crossing of such an edge by a backward job then counts nowhere).  The nodes listed
    in no_twin_of keep both copies but neither knows the other (twin NONE on interior nodes, as for a node whose id's partner names
    another sequence): every edge that touches one has no mirror slot"""
    n = 2 * len(node_lens) + 2
    node_len = [1] + [int(x) for x in node_lens for _ in (0, 1)] + [1]
    in_lists = [[] for _ in range(n)]
    for i, j in edges:
        f, t = 1 + 2 * i, 1 + 2 * j
        if f not in in_lists[t]:
            in_lists[t].append(f)
        if (i, j) not in drop_mirror_of and t + 1 not in in_lists[f + 1]:
            in_lists[f + 1].append(t + 1)
    twin = [NONE] + [k + 1 if k % 2 else k - 1 for k in range(1, n - 1)] + [NONE]
    for i in no_twin_of:
        twin[1 + 2 * i] = twin[2 + 2 * i] = NONE
    return node_len, in_lists, twin


def csr(in_lists):
    off = np.zeros(len(in_lists) + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(x) for x in in_lists])
    nbr = np.array([m for lst in in_lists for m in lst] + [0], dtype=np.uint32)       # (never empty: ctypes wants an address)
    return off, nbr


def route(codes, graph, start, choose):
    """the move bytes of a stream of move codes walked back from the cell `start` = (node, offset): a column step out of a node's offset 0
    names the in-neighbour choose(node, in-degree) picks.  The stream is cut where a column step would leave a node without in-neighbours"""
    node_len, in_lists, _ = graph
    node, offset = start
    moves = []
    for code in codes:
        via = 0
        if code != om.MOVE_UP:
            if offset > 0:
                offset -= 1
            else:
                if not in_lists[node]:
                    break
                via = int(choose(node, len(in_lists[node])))
                node = in_lists[node][via]
                offset = node_len[node] - 1
        moves.append(code | (via << 2))
    return moves


def replay(moves, graph, start, start_row, trace_rows, backward):
    """(counts per slot, crossings counted) of one job whose traceback is `moves` from the cell `start` at row start_row"""
    node_len, in_lists, twin = graph
    last = len(node_len) - 1
    first_slot = np.concatenate([[0], np.cumsum([len(x) for x in in_lists])])
    counts = np.zeros(int(first_slot[-1]), dtype=np.int64)
    node, offset = start
    row = start_row
    cells = [(node, offset, row)]
    for m in moves:
        code, via = m & 3, m >> 2
        if code != om.MOVE_LEFT:
            row -= 1
        if code != om.MOVE_UP:
            if offset > 0:
                offset -= 1
            else:
                node = in_lists[node][via]
                offset = node_len[node] - 1
        cells.append((node, offset, row))
    assert row >= 0, "a fabricated stream stays inside its rows"
    # the host's trace: the stream's last cell first; cells at rows >= trace_rows are dropped from its end (the stream's first cells)
    trace = cells[::-1]
    while trace and trace[-1][2] >= trace_rows:
        trace.pop()
    if backward:
        trace = trace[::-1]
        mirrored = []
        for nd, off, r in trace:
            if twin[nd] == NONE:
                mirrored.append(None)                        # (no mirror cell: nothing that touches it can be counted)
            else:
                mirrored.append((twin[nd], node_len[nd] - 1 - off, r))
        trace = mirrored
    items = trace[1:]                                        # the first cell of the part has no item
    n = 0
    for a, b in zip(items, items[1:]):
        if a is None or b is None:
            continue
        if a[0] == b[0] and (b[1] == a[1] or b[1] == a[1] + 1):
            continue
        if a[0] in (0, last) or b[0] in (0, last):
            continue
        if a[0] not in in_lists[b[0]]:
            continue
        counts[int(first_slot[b[0]]) + in_lists[b[0]].index(a[0])] += 1
        n += 1
    return counts, n


def mirror_slots(graph):
    """per slot of f -> t the slot of twin(t) -> twin(f), or NONE: what the library's table must hold"""
    node_len, in_lists, twin = graph
    last = len(node_len) - 1
    first_slot = np.concatenate([[0], np.cumsum([len(x) for x in in_lists])])
    out = []
    for t, lst in enumerate(in_lists):
        for f in lst:
            mf, mt = twin[t], twin[f]
            ok = t not in (0, last) and f not in (0, last) and mf != NONE and mt != NONE and mf not in (0, last) and mt not in (0, last) and mf in in_lists[mt]
            out.append(int(first_slot[mt]) + in_lists[mt].index(mf) if ok else NONE)
    return np.array(out, dtype=np.uint32)
