"""The read alphabet on the MI355X: ga_eq_words_kernel is the one statement of the rule that has no twin on the host (every
emulation back end ignores GaEqSource), so the probe sets of alphabet_cases.py run through the product library here -- every byte
value in both directions, the edge bytes on the slice-edge rows and on the last real row before the padding, every result against
alphabet_model.py and, field by field, against the oracle.

Both first-pass choices (as test_gpu_parity.py: the lanes = reads kernel takes the match words, the wave-per-read ladder the row
codes the same kernel writes), with and without TraceItem lists.  Further: a batch that qualifies for node runs and one that an
invalid read disqualifies, a batch with more fills than the kernel has blocks (its grid-stride loop), and reads with ambiguity
codes through the sparse variant, which reads the row codes by itself (ga_sparse.h).
"""
import pytest

import alphabet_cases as ac
import parity_cases as cases

pytestmark = pytest.mark.gpu

SPARSE = "<256,1,sparse>"
TRACE = pytest.mark.parametrize("trace", [True, False], ids=["trace-items", "flags-0"])
MODE = pytest.mark.parametrize("mode", ["lanes-first", "ladder-only"])


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need a real MI355X"


@pytest.fixture(autouse=True)
def _environment(monkeypatch):
    monkeypatch.setenv("GA_DEBUG_PASSES", "1")
    for name in ("GA_LANES", "GA_LANES_SPREAD", "GA_TEST_WAVE_SLOTS", "GA_RUNS"):
        monkeypatch.delenv(name, raising=False)


def first_pass(monkeypatch, mode):
    monkeypatch.setenv("GA_LANES", "1" if mode == "lanes-first" else "0")


@TRACE
@MODE
@pytest.mark.parametrize("name", sorted(ac.GRAPHS))
def test_probes_on_the_device(name, mode, trace, monkeypatch, capfd):
    first_pass(monkeypatch, mode)
    capfd.readouterr()
    devs = ac.case_probes(name, ac.all_probes(), trace)
    passes = cases.debug_passes(capfd.readouterr().err)
    # the kernel that was asked for took the jobs: a lanes = reads line first, or no such line at all
    assert passes, "no debug lines"
    lanes_lines = [p for p in passes if p[3] > 1]
    if mode == "lanes-first":
        assert passes[0][3] > 1 and passes[0][1] >= len(devs) // 2, passes
    else:
        assert not lanes_lines, passes


def test_node_runs_see_the_alphabet():
    ac.case_node_runs_see_the_alphabet()


def test_more_fills_than_blocks():
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    stats = ac.case_more_fills_than_blocks(cus)
    print("%d jobs on %d CUs, kernels %.1f ms" % (stats["n_jobs"], cus, stats["kernel_ms"]))


@TRACE
def test_sparse_variant_sees_the_alphabet(trace, capfd):
    """ambiguity codes, lower case and one invalid byte inside the branches of case_sparse_method_and_override's first fan: against the
    oracle alone (no model of a fan), and the sparse variant must have taken the parts whose oracle run shows a sparse slice"""
    ac.fan_batch()              # (its oracle runs print nothing into the capture below)
    capfd.readouterr()
    need = ac.case_sparse_variant_sees_the_alphabet(trace)[2]
    err = capfd.readouterr().err
    print(err, end="")
    lines = cases.passes_of(cases.debug_passes(err), SPARSE)
    assert max(p[1] for p in lines) >= need, (lines, need)
