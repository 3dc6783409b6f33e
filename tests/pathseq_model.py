"""What GA_F_PATHSEQ must return (include/graphaligner_amd.h): per part of the alignment the base of its first cell, then the graph_char
of every TraceItem of type MATCH, MISMATCH or DELETION, from the oracle's raw cells and TraceItem list alone; and an independent replay
of a move stream over a chain of nodes for the fabricated streams of tests/test_pathseq.py (the chain of ops_model.replay)."""
import ops_model as om
import pileup_model as pm

_EMITS = (om.MATCH, om.MISMATCH, om.DELETION)
_COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A"}


def oracle_path_seq(ora, base_at):
    """(bytes, n_backward) of a read from its oracle result (a dict of oracle_binding): bw_trace / fw_trace hold the parts' cells as
    (column, read position) in final order, `trace` the 7-column TraceItem list.  base_at(column) -> the graph's base there, needed for
    the first cell of each part alone; every item's graph_char is checked against it on the way; base_at.graph_bp = the graph's columns,
    the two dummy nodes' included.  A read that failed or asserted has no sequence."""
    if ora["status"] != 0 or ora["failed"]:
        return b"", 0
    graph_bp = base_at.graph_bp
    t = ora["trace"]
    bw, fw = ora["bw_trace"], ora["fw_trace"]
    dummy = pm.dummy_items(ora, graph_bp)               # (asserts that the list and the raw cells line up: backward - 1, SPLIT, forward - 1)
    is_dummy = lambda column: column == 0 or column == graph_bp - 1
    out, n_backward, at = [], 0, 0
    for part in (bw, fw):
        if len(part):
            first = int(part[0, 0])
            if not is_dummy(first):
                out.append(base_at(first))
            for k in range(1, len(part)):
                item, on_dummy = t[at], dummy[at]
                at += 1
                if on_dummy:
                    continue
                assert chr(int(item[5])) == base_at(int(part[k, 0])), "the column table and the oracle's graph_char disagree"
                if int(item[4]) in _EMITS:
                    out.append(chr(int(item[5])))
        if part is bw:
            n_backward = len(out)
            if len(bw) and len(fw):
                # the model's own cross-check: the SPLIT item carries the forward part's first cell
                assert int(t[at, 4]) == om.SPLIT
                assert is_dummy(int(fw[0, 0])) or chr(int(t[at, 5])) == base_at(int(fw[0, 0])), "SPLIT item and the forward part's first cell disagree"
                at += 1
    assert at == len(t)
    return "".join(out).encode(), n_backward


def replay(moves, n_nodes, node_len, start_row, trace_rows, backward):
    """the bases of one job whose traceback is `moves` (GA_MOVE_* codes) over the chain of the emulation library's stream hooks, from
    the chain's last base at row start_row.  Written over the job's cell list, not over the stream's places: the cells are listed, those
    at rows >= trace_rows dropped, the rest put in read order, and then c_0 gives its base and every later cell gives one when the move
    between it and its predecessor in read order took a column step.  The chain has no self-loop, so a move up gives nothing; positions
    below 0 are the start dummy and give nothing; the hook has no twin table, so a backward job's bases are the cells' own, complemented."""
    x, row = n_nodes * node_len - 1, start_row
    cells = [(x, row, None)]                            # (position, row, the move that led here)
    for m in moves:
        code = m & 3
        if code != om.MOVE_LEFT:
            row -= 1
        if code != om.MOVE_UP:
            x -= 1
        cells.append((x, row, code))
    # stream order: cells[i + 1] is reached from cells[i] by move i
    kept = [i for i, c in enumerate(cells) if c[1] < trace_rows]
    if not kept:
        return b""
    assert kept == list(range(kept[0], len(cells))), "rows only fall along a stream"

    def base(pos):
        if pos < 0:
            return ""
        b = om.chain_base(pos)
        return _COMPLEMENT[b] if backward else b

    out = []
    if backward:
        # read order is stream order; a cell is described by the move that leads to it
        out.append(base(cells[kept[0]][0]))
        for i in kept[1:]:
            if cells[i][2] != om.MOVE_UP:
                out.append(base(cells[i][0]))
    else:
        # read order is the stream reversed; a cell is described by the move that starts in it
        out.append(base(cells[-1][0]))
        for i in reversed(kept[:-1]):
            if cells[i + 1][2] != om.MOVE_UP:
                out.append(base(cells[i][0]))
    return "".join(out).encode()
