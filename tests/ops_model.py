"""What GA_F_OPS must return (include/graphaligner_amd.h): the types of the oracle's TraceItem list cut into maximal runs, and an
independent replay of a move stream over a chain of nodes for the fabricated streams of tests/test_ops.py."""
import numpy as np

MATCH, MISMATCH, INSERTION, DELETION, SPLIT = 1, 2, 3, 4, 5
MOVE_LEFT, MOVE_DIAG, MOVE_UP = 0, 1, 2


def rle(types):
    out = []
    for t in types:
        if out and out[-1][0] == t:
            out[-1] = (t, out[-1][1] + 1)
        else:
            out.append((t, 1))
    return out


def oracle_ops(ora):
    """the runs of a read from its oracle result (a dict of oracle_binding); a read that failed or asserted has none"""
    if ora["status"] != 0 or ora["failed"]:
        return []
    return rle([int(t) for t in ora["trace"][:, 4]])


def counts_of(runs):
    """(match, mismatch, insertion, deletion): summed run lengths"""
    return tuple(sum(n for t, n in runs if t == k) for k in (MATCH, MISMATCH, INSERTION, DELETION))


def as_pairs(ops):
    """the (n, 2) array of the binding as a list of (type, length)"""
    return [(int(t), int(n)) for t, n in np.asarray(ops).reshape(-1, 2)]


def chain_base(x):
    """base x of the chain the emulation library's stream hook builds"""
    return "ACGT"[x % 4]


_COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A"}


def replay(moves, n_nodes, node_len, start_row, trace_rows, backward, read):
    """the runs of one job whose traceback is `moves` (GA_MOVE_* codes) over a chain of n_nodes nodes of node_len bases, from the chain's
    last base at row start_row: positions are one coordinate along the chain (below 0: the dummy start node, which matches nothing).
    The chain has no self-loop, so a move up is always an insertion."""
    x, row = n_nodes * node_len - 1, start_row
    types = []
    for m in moves:
        code = m & 3
        ax, arow = x, row
        if code != MOVE_LEFT:
            row -= 1
        if code != MOVE_UP:
            x -= 1
        if arow >= trace_rows:
            continue
        if code == MOVE_LEFT:
            types.append(DELETION)
        elif code == MOVE_UP:
            types.append(INSERTION)
        else:
            cx, crow = (x, row) if backward else (ax, arow)
            ch = read[trace_rows - 1 - crow] if backward else read[crow]
            base = chain_base(cx) if cx >= 0 else None
            if backward and base:
                base = _COMPLEMENT[base]
            types.append(MATCH if base and (ch == base or ch == "N") else MISMATCH)
    if not backward:
        types.reverse()
    return rle(types)
