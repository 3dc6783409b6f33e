"""GA_F_PATHSEQ on the host build: the path-sequence program of graphaligner_amd/csrc/ga_pathseq.h (tests/emul/pathseq.mk ->
tests/_build/libga_pathseq_emul.so) over fabricated move streams, against pathseq_model.replay, with guard bytes around the job's
place; and what needs no device of the interface: the host emulation of the back end writes no path sequences and refuses the flag.
The product's kernels run the cases of pathseq_cases.py in test_pathseq_gpu.py.  Without the feature nothing here passes: there is no
such program to build."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from graphaligner_amd import binding
import ops_cases as oc
import ops_model as om
import parity_common as pc
import pathseq_model as psm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L_, D_, U_ = om.MOVE_LEFT, om.MOVE_DIAG, om.MOVE_UP
STREAM_LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 4096, 4097)
NODE_LENGTHS = (1, 3, 64)
KINDS = ("diag", "left", "up", "alternating", "random", "lanes-0-and-63", "off-the-front")
# start_row = trace_rows - 1 + DROP: nothing dropped; the drop ends inside round 0; inside round 1 (where the stream has that many row steps)
DROPS = (0, 2, 71)
GUARD, FILL = 0x5A, 0xA5


@pytest.fixture(scope="module")
def hook():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emul"), "-f", "pathseq.mk"])
    L = C.CDLL(os.path.join(ROOT, "tests", "_build", "libga_pathseq_emul.so"))
    L.ga_emul_pathseq_stream.restype = C.c_long
    L.ga_emul_pathseq_stream.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_size_t]
    return L


def codes(kind, n, rng):
    if kind == "diag":
        return [D_] * n
    if kind == "left":
        return [L_] * n
    if kind == "up":
        return [U_] * n                   # only c_0 has a base
    if kind == "alternating":
        return [(D_, L_, U_)[i % 3] for i in range(n)]
    if kind == "lanes-0-and-63":
        # a base from the first and the last lane of every round and from nowhere else (a diagonal at lane 0, a move left at lane 63)
        return [D_ if i % 64 == 0 else L_ if i % 64 == 63 else U_ for i in range(n)]
    return [int(x) for x in rng.choice([D_, D_, D_, L_, U_], size=n)]


def streams():
    """every fabricated stream as (kind, moves, n_nodes, node_len, start_row, trace_rows, backward)"""
    for kind in KINDS:
        for node_len in NODE_LENGTHS:
            for backward in (False, True):
                rng = np.random.default_rng(len(kind) * 31 + node_len + int(backward))
                for n in STREAM_LENGTHS:
                    if kind == "off-the-front":
                        # the chain's columns used up by one step: the stream's last column step enters the start dummy, where moves up follow
                        n_nodes = max(1, n // (2 * node_len))
                        moves = [D_] * (n_nodes * node_len) + [U_] * 3
                    else:
                        moves = codes(kind, n, rng)
                        cols = sum(1 for m in moves if m != U_)
                        n_nodes = (cols + 2) // node_len + 2
                    rows = sum(1 for m in moves if m != L_)
                    for drop in DROPS:
                        yield kind, moves, n_nodes, node_len, rows, max(rows + 1 - drop, 0), backward


def run_stream(hook, moves, n_nodes, node_len, start_row, trace_rows, backward):
    """the hook's bytes; the place is as long as the longest possible sequence, pre-filled, with one guard byte on each side"""
    mv = np.array(moves, dtype=np.uint8)
    cap = len(moves) + 1
    buf = np.full(cap + 2, FILL, dtype=np.uint8)
    buf[0] = buf[-1] = GUARD
    n = hook.ga_emul_pathseq_stream(mv.ctypes.data_as(C.c_void_p), len(moves), n_nodes, node_len, start_row, trace_rows, int(backward),
                                    C.c_void_p(buf.ctypes.data + 1), cap)
    assert 0 <= n <= cap
    assert buf[0] == GUARD and buf[-1] == GUARD, "a guard byte was written"
    assert (buf[1 + n:-1] == FILL).all(), "bytes behind the job's count were written"
    return buf[1:1 + n].tobytes()


@pytest.mark.parametrize("kind", KINDS)
def test_fabricated_streams(hook, kind):
    seen = 0
    for k, moves, n_nodes, node_len, start_row, trace_rows, backward in streams():
        if k != kind:
            continue
        got = run_stream(hook, moves, n_nodes, node_len, start_row, trace_rows, backward)
        want = psm.replay(moves, n_nodes, node_len, start_row, trace_rows, backward)
        assert got == want, (kind, len(moves), n_nodes, node_len, start_row, trace_rows, backward, got[:80], want[:80])
        seen += 1
    assert seen >= len(STREAM_LENGTHS) * len(NODE_LENGTHS) * 2 * len(DROPS)


def test_what_the_streams_cover():
    """the properties the list of streams is there for, checked on the model's side"""
    some = [s[1:] for s in streams()]
    assert any(len(m) == 0 and psm.replay(m, nn, nl, sr, tr, b) != b"" for m, nn, nl, sr, tr, b in some), "a job without moves has its one cell"
    assert any(m and all(x == U_ for x in m) and len(psm.replay(m, nn, nl, sr, tr, b)) == 1 for m, nn, nl, sr, tr, b in some), "all-UP: c_0 alone"
    assert any(m and all(x == L_ for x in m) and tr > 0 and len(psm.replay(m, nn, nl, sr, tr, b)) == len(m) + 1 for m, nn, nl, sr, tr, b in some)
    assert any(psm.replay(m, nn, nl, sr, tr, b) == b"" and tr == 0 for m, nn, nl, sr, tr, b in some), "no kept cell: nothing"
    off = [(m, nn, nl, sr, tr, b) for m, nn, nl, sr, tr, b in some if m[-3:] == [U_] * 3 and sum(1 for x in m if x != U_) == nn * nl]
    assert off and all(len(psm.replay(m, nn, nl, sr, sr + 1, b)) == nn * nl for m, nn, nl, sr, tr, b in off), "the dummy's cells give nothing"


def test_replay_agrees_with_the_operations_model():
    """ACGT reads copied from the chain: at every MATCH of ops_model.replay the path base is the read's, and the bases number matches +
    mismatches + deletions + 1"""
    rng = np.random.default_rng(5)
    for backward in (False, True):
        moves = codes("random", 300, rng)
        rows = sum(1 for m in moves if m != L_)
        n_nodes, node_len = 400, 1
        runs = om.replay(moves, n_nodes, node_len, rows, rows + 1, backward, "A" * (rows + 1))
        m, x, i, d = om.counts_of(runs)
        assert len(psm.replay(moves, n_nodes, node_len, rows, rows + 1, backward)) == m + x + d + 1


def test_the_emulated_back_end_refuses_the_flag():
    """tests/emul's back end writes no path sequences: the prepare is refused with GA_E_INVALID, and works without the flag"""
    g, reads, seeds = oc.round_edge_batch(64)
    gg = binding.Graph(g.nodes, g.edges, lib_path=pc.emul_lib_path())
    with pytest.raises(RuntimeError, match=r"\(100\)"):
        gg.prepare(reads, seeds, 35, 0, binding.GA_F_PATHSEQ)
    devs = gg.align(reads, seeds, 35)
    assert len(devs) == len(reads) and all("path_seq" not in d for d in devs)
    b = gg.prepare(reads, seeds, 35, 0, 0)
    st = binding.GaBatchPathSeqStats()
    assert b.L.ga_batch_path_seq_stats(b.h, C.byref(st)) == 100
