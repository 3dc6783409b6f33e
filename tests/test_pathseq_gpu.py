"""GA_F_PATHSEQ on the GPU: ga_pathseq_count_kernel and ga_pathseq_write_kernel through the product library, every read's path sequence
and the length of its backward part against pathseq_model.oracle_path_seq.  Cases: pathseq_cases.py; the walk alone runs on the host in
test_pathseq.py.  On a library without the flag every test here fails: the prepare is refused."""
import pytest

from graphaligner_amd import synth
import pathseq_cases as psc

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
def test_round_edges(node_len):
    psc.case_round_edges(node_len)


@pytest.mark.parametrize("row", [(5, 40, 0, 0), (8, 15, 60, 0)], ids=str)
def test_crossings_on_short_nodes(row):
    psc.case_crossing_graphs(row)


def test_in_degree_above_four():
    psc.case_fan_in_degree()


@pytest.mark.parametrize("row", [(64, 100, 1000, 0), (8, 15, 60, 0)], ids=str)
def test_both_parts_and_the_seam(row):
    psc.case_both_parts(row)


def test_one_part_and_reverse_strand():
    psc.case_one_part_and_strands()


def test_gfa_overlap():
    psc.case_gfa_overlap()


def test_one_base_self_loop():
    psc.case_self_loop()


def test_cyclic_band():
    psc.case_cyclic()


def test_ramp_redo():
    psc.case_ramp()


def test_300_branches():
    psc.case_wide()


def test_several_seeds():
    psc.case_several_seeds()


def test_many_jobs_on_one_wave_twice(monkeypatch):
    monkeypatch.setenv("GA_TEST_WAVE_SLOTS", "1")
    st = psc.case_many_jobs_one_wave()
    assert st["jobs_walked"] >= 257 and st["bases_written"] > 0


def test_seeded_batch_equals_two_calls():
    g = synth.bubble_graph(60000, node_len=64, seed=71)
    reads, _ = synth.simulate_reads(g, 24, 1500, seed=17, mid_seed=True)
    psc.case_seeded_batch_equals_two_calls(g, reads, 12)


def test_all_three_flags_together():
    psc.case_all_flags_together()


def test_flag_changes_nothing_else():
    psc.case_flag_changes_nothing_else()


def test_unsplit_carries_the_bases_over():
    psc.case_unsplit()


def test_ops_and_path_walked_together():
    psc.case_ops_and_path_walked_together()


def test_sharding_passes_the_flag_and_the_fields_through():
    """run_overlapped, align_queued and align_sharded with GA_F_PATHSEQ: the bases of a direct call, as dicts and with summary=True"""
    from graphaligner_amd import binding, sharding
    g, reads, seeds, bw = psc._mid_seed_batch()
    gg = binding.Graph(g.nodes, g.edges)
    direct = [(r["path_seq"], r["path_seq_backward"]) for r in gg.align(reads, seeds, bw, 0, binding.GA_F_PATHSEQ)]
    assert sum(1 for s, n in direct if s and 0 < n < len(s)) >= 6
    half = len(reads) // 2
    parts = dict(sharding.run_overlapped(gg, [(0, (reads[:half], seeds[:half])), (1, (reads[half:], seeds[half:]))], bw, flags=binding.GA_F_PATHSEQ))
    assert [(r["path_seq"], r["path_seq_backward"]) for r in parts[0] + parts[1]] == direct
    queued = sharding.align_queued(gg, reads, seeds, bw, flags=binding.GA_F_PATHSEQ, chunk_reads=5)
    assert [(r["path_seq"], r["path_seq_backward"]) for r in queued] == direct
    recs, seqs, n_backward = sharding.align_queued(gg, reads, seeds, bw, flags=binding.GA_F_PATHSEQ, chunk_reads=5, summary=True)
    assert len(recs) == len(reads) and list(zip(seqs, (int(n) for n in n_backward))) == direct
    both = sharding.align_queued(gg, reads, seeds, bw, flags=binding.GA_F_OPS | binding.GA_F_PATHSEQ, chunk_reads=5, summary=True)
    assert len(both) == 5 and list(zip(both[3], (int(n) for n in both[4]))) == direct
    sharded = sharding.align_sharded(gg, reads, seeds, bw, flags=binding.GA_F_PATHSEQ)
    assert [(r["path_seq"], r["path_seq_backward"]) for r in sharded] == direct
