"""GA_F_OPS on the host build (tests/emul: behind the emulated ladder graphaligner_amd/csrc/ga_ops.h run
launch by launch): every read's runs against ops_model.rle(oracle trace types).  Cases: ops_cases.py; the same cases on the GPU are in
test_ops_gpu.py.  On a library without the flag every test here fails: a result has no `ops`."""
import ctypes as C

import numpy as np
import pytest

from graphaligner_amd import binding, synth
import alphabet_cases as ac
import ops_cases as oc
import ops_model as om
import parity_common as pc


@pytest.fixture(scope="module")
def lib():
    return pc.emul_lib_path()


@pytest.fixture(autouse=True, params=["lanes-first", "wave-per-read-first"])
def _first_pass(request, monkeypatch):
    """both first passes of the emulated ladder: the lanes = reads program, or the wave-per-read program over everything"""
    monkeypatch.delenv("GA_TEST_WAVE_SLOTS", raising=False)
    monkeypatch.setenv("GA_LANES", "1" if request.param == "lanes-first" else "0")


@pytest.mark.parametrize("node_len", [64, 1], ids=["64-bp-nodes", "1-bp-nodes"])
def test_round_edges_and_crossings(lib, node_len):
    oc.case_round_edges(node_len, lib)


@pytest.mark.parametrize("row", [(5, 40, 0, 0), (8, 15, 60, 0)], ids=str)
def test_crossings_on_short_nodes(lib, row):
    oc.case_crossing_graphs(row, lib)


def test_in_degree_above_four(lib):
    oc.case_fan_in_degree(lib)


@pytest.mark.parametrize("row", [(64, 100, 1000, 0), (8, 15, 60, 0)], ids=str)
def test_both_parts(lib, row):
    oc.case_both_parts(row, lib)


def test_one_part_and_reverse_strand(lib):
    oc.case_one_part_and_strands(lib)


def test_gfa_overlap(lib):
    oc.case_gfa_overlap(lib)


def test_one_base_self_loop(lib):
    oc.case_self_loop(lib)


@pytest.mark.parametrize("name,probes", [("64bp-nodes", "all"), ("8bp-nodes", "lengths")])
def test_alphabet(lib, name, probes):
    oc.case_alphabet(name, ac.all_probes() if probes == "all" else ac.length_probes(), lib)


def test_cyclic_band(lib):
    oc.case_cyclic(lib)


def test_ramp_redo(lib):
    oc.case_ramp(lib)


def test_300_branches(lib):
    oc.case_wide(lib)


def test_several_seeds(lib):
    oc.case_several_seeds(lib)


def test_many_jobs_on_one_wave(lib, monkeypatch):
    monkeypatch.setenv("GA_TEST_WAVE_SLOTS", "1")
    st = oc.case_many_jobs_one_wave(lib)
    assert st["jobs_coded"] >= 257 and st["runs_written"] > 0


def test_flag_changes_nothing_else(lib):
    oc.case_flag_changes_nothing_else(lib)


def test_older_back_ends_refuse_the_flag():
    """a back end that does not code operations: the prepare is refused with GA_E_INVALID, and works without the flag"""
    g, reads, seeds = oc.round_edge_batch(64)
    with pc.emul_profile("emul"):
        gg = binding.Graph(g.nodes, g.edges, lib_path=pc.emul_lib_path())
    with pytest.raises(RuntimeError, match=r"\(100\)"):
        gg.prepare(reads, seeds, 35, 0, binding.GA_F_OPS)
    assert len(gg.align(reads, seeds, 35)) == len(reads)


def test_seeded_batch_equals_two_calls(lib):
    """the twin of test_ops_gpu.py's: the driver's graph and reads (test_seed_plan.py::test_driver_output_is_byte_identical)"""
    g = synth.bubble_graph(30000, node_len=32, seed=21)
    reads, _ = synth.simulate_reads(g, 6, 1200, seed=77, mid_seed=True)
    oc.case_seeded_batch_equals_two_calls(g, reads, 5, lib)


def test_ops_string():
    assert binding.ops_string([(1, 254), (2, 1), (3, 3), (4, 2)]) == "254=1X3I2D"
    assert binding.ops_string(np.array([[1, 5], [5, 1], [1, 7]], dtype=np.uint32)) == "5=|7="
    assert binding.ops_string([]) == ""


# ---- fabricated streams: the walk alone, through the emulation library's test entry point, against ops_model.replay ----------------
L_, D_, U_ = om.MOVE_LEFT, om.MOVE_DIAG, om.MOVE_UP
STREAM_LENGTHS = (0, 1, 63, 64, 65, 4096, 4097)


def _stream(kind, n, rng):
    if kind == "diag":
        return [D_] * n
    if kind == "left":
        return [L_] * n
    if kind == "up":
        return [U_] * n
    if kind == "alternating":
        return [(D_, L_, U_)[i % 3] for i in range(n)]
    return [int(x) for x in rng.choice([D_, D_, D_, L_, U_], size=n)]


def _run_stream(lib, moves, n_nodes, node_len, start_row, trace_rows, backward, read):
    L = binding.load(lib)
    L.ga_emul_ops_stream.restype = C.c_long
    L.ga_emul_ops_stream.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_char_p, C.c_uint32, C.c_void_p, C.c_size_t]
    mv = np.array(moves, dtype=np.uint8)
    out = np.zeros(len(moves) + 2, dtype=np.uint32)
    n = L.ga_emul_ops_stream(mv.ctypes.data_as(C.c_void_p), len(moves), n_nodes, node_len, start_row, trace_rows, int(backward), read.encode(), len(read),
                             out.ctypes.data_as(C.c_void_p), len(out))
    assert n >= 0
    return [(int(w & 7), int(w >> 3)) for w in out[:n]]


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
@pytest.mark.parametrize("chain", [(5000, 1), (1, 5000)], ids=["1-bp-nodes", "one-5000-bp-node"])
@pytest.mark.parametrize("kind", ["diag", "left", "up", "alternating", "random"])
def test_fabricated_streams(lib, kind, chain, backward):
    n_nodes, node_len = chain
    rng = np.random.default_rng(len(kind) * 31 + n_nodes + int(backward))
    for n in STREAM_LENGTHS:
        moves = _stream(kind, n, rng)
        rows = sum(1 for m in moves if m != L_)
        cols = sum(1 for m in moves if m != U_)
        if cols >= n_nodes * node_len:
            continue                      # (the stream would leave the chain and the start dummy: nothing a traceback writes)
        read = "".join(rng.choice(list("ACGTN"), size=rows + 70))
        for cut in (0, 1, 37, 64):        # trace_rows cutting inside a round: the first `cut` rows of the stream are dropped
            start_row = rows
            trace_rows = max(start_row + 1 - cut, 0)
            got = _run_stream(lib, moves, n_nodes, node_len, start_row, trace_rows, backward, read)
            want = om.replay(moves, n_nodes, node_len, start_row, trace_rows, backward, read)
            assert got == want, (kind, chain, backward, n, cut, binding.ops_string(got)[:200], binding.ops_string(want)[:200])


def test_sharding_passes_the_flag_and_the_fields_through(lib):
    """run_overlapped and align_queued with GA_F_OPS: the runs of a direct call, as dicts and with summary=True"""
    from graphaligner_amd import sharding
    g, reads, seeds = oc.round_edge_batch(64)
    gg = binding.Graph(g.nodes, g.edges, lib_path=lib)
    direct = gg.align(reads, seeds, 35, 0, binding.GA_F_OPS)
    halves = [(0, (reads[:5], seeds[:5])), (1, (reads[5:], seeds[5:]))]
    parts = dict(sharding.run_overlapped(gg, halves, 35, flags=binding.GA_F_OPS))
    assert [binding.ops_string(r["ops"]) for r in parts[0] + parts[1]] == oc.ROUND_EXPECTED
    queued = sharding.align_queued(gg, reads, seeds, 35, flags=binding.GA_F_OPS, chunk_reads=4)
    assert [binding.ops_string(r["ops"]) for r in queued] == oc.ROUND_EXPECTED
    assert [r["op_counts"] for r in queued] == [r["op_counts"] for r in direct]
    recs, counts, runs = sharding.align_queued(gg, reads, seeds, 35, flags=binding.GA_F_OPS, chunk_reads=4, summary=True)
    assert [binding.ops_string(r) for r in runs] == oc.ROUND_EXPECTED and len(recs) == len(reads)
    assert [tuple(int(x) for x in c) for c in counts] == [om.counts_of(om.as_pairs(r)) for r in runs]
    sharded = sharding.align_sharded(gg, reads, seeds, 35, flags=binding.GA_F_OPS)
    assert [binding.ops_string(r["ops"]) for r in sharded] == oc.ROUND_EXPECTED
