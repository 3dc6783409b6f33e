"""-B ramp redos that land on a sparse-method slice or meet a backtrace-override window, on the MI355X: the batches of
redo_sparse_cases.py (what each read shows on the oracle: redo_events.py; the host emulation of the same: test_redo_sparse.py)
through the real library, every field of every read against the oracle.

Each batch runs in both first-pass modes (as test_gpu_parity.py), with and without TraceItem lists, and three reads of each of three
batches once more on ONE wave slot (GA_TEST_WAVE_SLOTS=1, wave-per-read kernels only), so that one wave takes job after job on its
predecessors' leavings in LDS and in its generation-stamped sparse tables: a read that fails or ends in an assertion first, then L1
reads.  Every test reads the library's GA_DEBUG_PASSES lines: the sparse variant must have run and taken at least as many jobs as
there are parts whose oracle run shows a sparse slice, and no such read may have been answered by the
first pass."""
import pytest

import parity_cases as cases
import parity_common as pc
import redo_sparse_cases as rc
from graphaligner_amd import binding

pytestmark = pytest.mark.gpu

SPARSE = "<256,1,sparse>"
TRACE = pytest.mark.parametrize("trace", [True, False], ids=["trace-items", "flags-0"])
FAN = pytest.mark.parametrize("fan_index", range(len(rc.FANS)))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need a real MI355X"


@pytest.fixture(scope="module", autouse=True)
def _conditions(_need_gpu):
    """the list shows its events on the oracle alone, before anything is compared"""
    return rc.check_conditions()


@pytest.fixture(autouse=True)
def _debug_lines(monkeypatch):
    monkeypatch.setenv("GA_DEBUG_PASSES", "1")
    for name in ("GA_LANES", "GA_LANES_SPREAD", "GA_TEST_WAVE_SLOTS"):
        monkeypatch.delenv(name, raising=False)


def first_pass(monkeypatch, mode):
    if mode == "lanes-first":
        monkeypatch.setenv("GA_LANES", "1")
    elif mode == "ladder-only":
        monkeypatch.setenv("GA_LANES", "0")


def run_batch(capfd, graph, reads, seeds, bw, ramp, trace):
    """-> (results, debug lines) of one batch through prepare / run / collect"""
    capfd.readouterr()
    gg = binding.Graph(graph.nodes, graph.edges)
    b = gg.prepare(reads, [[s] for s in seeds], bw, ramp, binding.GA_F_TRACE if trace else 0)
    b.run()
    devs = b.collect()
    err = capfd.readouterr().err
    print(err, end="")          # (shown with a failure, and with -s)
    assert len(devs) == len(reads)
    return devs, cases.debug_passes(err)


def batch_of(fan_index):
    found = [b for b in rc.batches() if b[0] == rc.FANS[fan_index]]
    assert found, ("no reads on fan", fan_index)
    return found[0]


def sparse_variant_took(passes, oras, devs, slots=None):
    """the sparse variant ran, with at least as many jobs as the oracle saw parts with a sparse slice; none of those was finished by
    the first pass"""
    lines = cases.passes_of(passes, SPARSE)
    need = rc.sparse_parts(oras)
    assert need >= 1
    assert max(p[1] for p in lines) >= need, (lines, need)
    rc.check_sparse_reads_climbed(devs, oras)
    if slots is not None:
        assert all(p[2] <= slots for p in passes), passes
        assert any(p[2] == slots and p[1] > slots and p[1] >= need for p in lines), ("no wave took job after job", lines)


@TRACE
@FAN
@pytest.mark.parametrize("mode", ["lanes-first", "by-graph-shape"])
def test_redo_cases_equal_the_oracle(fan_index, mode, trace, monkeypatch, capfd):
    fan, g, reads, seeds, descs, oras, classes = batch_of(fan_index)
    first_pass(monkeypatch, mode)
    devs, passes = run_batch(capfd, g, reads, seeds, fan[4], fan[5], trace)
    for d, o, desc, c in zip(devs, oras, descs, classes):
        pc.compare_read(d, pc.expected(o, trace), "fan %s draw %d %s" % (fan, desc[2], sorted(c["events"])))
    sparse_variant_took(passes, oras, devs)


@TRACE
@pytest.mark.parametrize("fan_index", sorted(rc.ONE_WAVE))
def test_redo_cases_on_one_wave(fan_index, trace, monkeypatch, capfd):
    """the wave-per-read kernels only, one wave per launch: job after job through one LDS image and one set of sparse tables.  Three
    reads per fan (redo_sparse_cases.ONE_WAVE): one that asserts or fails, then L1 reads"""
    fan, g, reads, seeds, descs, oras, classes = rc.one_wave_batch(fan_index)
    first_pass(monkeypatch, "ladder-only")
    monkeypatch.setenv("GA_TEST_WAVE_SLOTS", "1")
    devs, passes = run_batch(capfd, g, reads, seeds, fan[4], fan[5], trace)
    for d, o, desc, c in zip(devs, oras, descs, classes):
        pc.compare_read(d, pc.expected(o, trace), "one wave, fan %s draw %d %s" % (fan, desc[2], sorted(c["events"])))
    sparse_variant_took(passes, oras, devs, slots=1)


@TRACE
@pytest.mark.parametrize("mode", ["lanes-first", "by-graph-shape"])
def test_capacity_miss_is_loud_and_named(mode, trace, monkeypatch, capfd):
    """40 branches at bandwidth 35 / 70: status 10 (GA_S_CAPACITY) for the reads named in redo_sparse_cases.CAPACITY_MISSES and for
    no other; every other read of the batch equals the oracle"""
    g, reads, seeds, draws, oras = rc.capacity_batch()
    fan = rc.CAPACITY_FAN
    first_pass(monkeypatch, mode)
    devs, passes = run_batch(capfd, g, reads, seeds, fan[4], fan[5], trace)
    missed = sorted(draw for d, draw in zip(devs, draws) if d["status"] == 10)
    assert missed == sorted(rc.CAPACITY_MISSES), missed
    assert all(d["failed"] for d, draw in zip(devs, draws) if draw in rc.CAPACITY_MISSES)
    for d, o, draw in zip(devs, oras, draws):
        if draw not in rc.CAPACITY_MISSES:
            pc.compare_read(d, pc.expected(o, trace), "40 branches, draw %d" % draw)
    sparse_variant_took(passes, oras, devs)
