"""GA_F_OPS on the GPU: ga_ops_count_kernel and ga_ops_write_kernel through the product library, every read's runs against
ops_model.rle(oracle trace types).  Cases: ops_cases.py; the host build of the same program runs them in test_ops.py.  On a library
without the flag every test here fails: a result has no `ops`."""
import pytest

from graphaligner_amd import synth
import alphabet_cases as ac
import ops_cases as oc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need a real MI355X"


@pytest.fixture(autouse=True, params=["GA_LANES=1", "GA_LANES=0"])
def _first_pass(request, monkeypatch):
    """both first passes: the lanes = reads kernel (its own traceback writes the moves), and the wave-per-read kernels over everything"""
    monkeypatch.delenv("GA_TEST_WAVE_SLOTS", raising=False)
    monkeypatch.setenv("GA_LANES", request.param[-1])


@pytest.mark.parametrize("node_len", [64, 1], ids=["64-bp-nodes", "1-bp-nodes"])
def test_round_edges_and_crossings(node_len):
    st = oc.case_round_edges(node_len)
    assert st["jobs_coded"] == 10 and st["count_kernel_ms"] > 0 and st["write_kernel_ms"] > 0


@pytest.mark.parametrize("row", [(5, 40, 0, 0), (8, 15, 60, 0)], ids=str)
def test_crossings_on_short_nodes(row):
    oc.case_crossing_graphs(row)


def test_in_degree_above_four():
    oc.case_fan_in_degree()


@pytest.mark.parametrize("row", [(64, 100, 1000, 0), (8, 15, 60, 0)], ids=str)
def test_both_parts(row):
    oc.case_both_parts(row)


def test_one_part_and_reverse_strand():
    oc.case_one_part_and_strands()


def test_gfa_overlap():
    oc.case_gfa_overlap()


def test_one_base_self_loop():
    oc.case_self_loop()


@pytest.mark.parametrize("name,probes", [("64bp-nodes", "all"), ("8bp-nodes", "lengths")])
def test_alphabet(name, probes):
    oc.case_alphabet(name, ac.all_probes() if probes == "all" else ac.length_probes())


def test_cyclic_band():
    oc.case_cyclic()


def test_ramp_redo():
    oc.case_ramp()


def test_300_branches():
    oc.case_wide()


def test_several_seeds():
    oc.case_several_seeds()


def test_many_jobs_on_one_wave(monkeypatch):
    monkeypatch.setenv("GA_TEST_WAVE_SLOTS", "1")
    st = oc.case_many_jobs_one_wave()
    assert st["jobs_coded"] >= 257 and st["runs_written"] > 0


def test_flag_changes_nothing_else():
    oc.case_flag_changes_nothing_else()


def test_seeded_batch_equals_two_calls():
    """align_reads(..., flags=GA_F_OPS) equals prepare(reads, find_seeds(reads)) with the flag, run for run, and both the oracle"""
    g = synth.bubble_graph(60000, node_len=64, seed=71)
    reads, _ = synth.simulate_reads(g, 24, 1500, seed=17, mid_seed=True)
    oc.case_seeded_batch_equals_two_calls(g, reads, 12)
