"""-B ramp redos that land on a sparse-method slice or meet a backtrace-override window, on the host: the emulated device program
(tests/emul) against the oracle, every field of every read (parity_common.compare_read).

The reads are fixed (redo_sparse_cases.py; found by tools/find_redo_events.py) and named by what the oracle's slice records show
(redo_events.py): before anything is compared, the list must show on the oracle alone that the redos landed where this module
says they do.  The classifier itself is tested first, on hand-made record lists, so that a read cannot be called L1 by a bug in it.

Each batch runs with fresh buffers, with GA_EMUL_POISON, with GA_EMUL_REUSE and with both (as test_emulated_wave_reuse.py), with and
without TraceItem lists.  A batch is listed longest read first, the order in which one wave takes its jobs: reads that fail or end in
an assertion come before L1 reads that align."""
import pytest

import parity_common as pc
import redo_events as ev
import redo_sparse_cases as rc
from graphaligner_amd import binding

BIG = ev.CUTOFF


# ---- the classifier on hand-made records -----------------------------------------------------------------------------------------
def rec(j, bw=20, cells=500, sparse=False, partial=(), min_score=0, nodes=2, direction=0):
    """a slice record with `cells` columns, all written and confirmed at score min_score + 5, except `partial`: {column: end score}
    of columns that were written and whose last row is not confirmed"""
    end = [min_score + 5] * cells
    exists = [1] * cells
    for c, e in dict(partial).items():
        end[c] = e
        exists[c] = 0
    return dict(direction=direction, j=j, bandwidth=bw, sparse=sparse, end=end, end_exists=exists, written=[1] * cells, min_score=min_score, nodes=[0] * nodes)


def events_of(recs, ramp=45, n_slices=None):
    return ev.classify_direction(recs, ramp, n_slices)["events"]


def test_classifier_no_redo_and_plain_redo():
    recs = [rec(64 * k) for k in range(6)]
    out = ev.classify_direction(recs, 45)
    assert out["redos"] == [] and out["events"] == set()
    # a redo that lands on a bit-vector slice, and one that returns to the seed: redos, no event
    recs = [rec(0), rec(64), rec(128), rec(192), rec(128, bw=45), rec(192, bw=45), rec(256)]
    out = ev.classify_direction(recs, 45)
    assert [(d["at"], d["landing"]) for d in out["redos"]] == [(4, 1)] and out["events"] == set()
    recs = [rec(0), rec(64, sparse=True, partial={3: 9}), rec(128), rec(0, bw=45), rec(64, bw=45), rec(128, bw=45)]
    out = ev.classify_direction(recs, 45)
    assert [(d["at"], d["landing"]) for d in out["redos"]] == [(3, None)] and out["events"] == set()


def test_classifier_l1():
    # lands on slice j = 128, sparse with two written columns whose last row is not confirmed; the next slice is a bit-vector slice
    recs = [rec(0), rec(64), rec(128, sparse=True, partial={7: 99, 8: 99}), rec(192), rec(256), rec(192, bw=45, min_score=10), rec(256, bw=45)]
    out = ev.classify_direction(recs, 45)
    assert out["redos"] == [dict(at=5, landing=2, events={"L1"})]
    # the latest record at j - 64 is the landing slice: an earlier sparse version of it does not count
    recs = [rec(0), rec(64, sparse=True, partial={7: 99}), rec(128), rec(64, bw=45), rec(128, bw=45), rec(192), rec(128, bw=45), rec(192, bw=45)]
    assert [d["landing"] for d in ev.classify_direction(recs, 45)["redos"]] == [0, 3] and events_of(recs) == set()
    # a sparse landing slice whose columns all exist, or whose only unconfirmed columns were never written: no L1
    full = rec(128, sparse=True)
    untouched = rec(128, sparse=True, partial={7: 99})
    untouched["written"][7] = 0
    for landing in (full, untouched):
        assert events_of([rec(0), rec(64), landing, rec(192), rec(256), rec(192, bw=45), rec(256, bw=45)]) == set()
    # ... and a bit-vector landing slice with the same columns
    assert events_of([rec(0), rec(64), rec(128, partial={7: 99}), rec(192), rec(192 - 0, bw=45)]) == set()


def test_classifier_l1b():
    # the next slice has minimum 10 and bandwidth 45: an unconfirmed column at 55 can enter its band, one at 56 cannot
    mk = lambda e: [rec(0), rec(64), rec(128, sparse=True, partial={7: e, 9: 300}), rec(192), rec(192, bw=45, min_score=10), rec(256, bw=45)]
    assert events_of(mk(55)) == {"L1", "L1b"}
    assert events_of(mk(56)) == {"L1"}
    # the bound is the NEXT slice's, not the landing slice's
    recs = mk(40)
    recs[4] = rec(192, bw=20, min_score=10)
    assert events_of(recs) == {"L1"}


def test_classifier_l2():
    recs = [rec(0), rec(64), rec(128, sparse=True, partial={7: 9}), rec(192), rec(192, bw=45, sparse=True), rec(256, bw=45)]
    assert events_of(recs) == {"L2"}
    # sparse again although the landing slice has no unconfirmed column
    recs[2] = rec(128, sparse=True)
    assert events_of(recs) == {"L2"}
    # the landing slice is a bit-vector slice: no L2 whatever comes next
    recs[2] = rec(128)
    assert events_of(recs) == set()


def _window(closed, back_to):
    """slices 0, 1 small; 2, 3 of >= 200 000 cells (a window opens at 2, its pre-slice is 1); closed: slice 4 small closes it, 5 small;
    then the last slice turns wrong and the pass goes back: the first slice computed again is `back_to`"""
    recs = [rec(0), rec(64), rec(128, cells=BIG, sparse=True), rec(192, cells=BIG, sparse=True)]
    recs += [rec(256), rec(320), rec(384)] if closed else [rec(256, cells=BIG, sparse=True)]
    return recs + [rec(64 * back_to, bw=45), rec(64 * back_to + 64, bw=45)]


def test_classifier_w1():
    assert events_of(_window(False, 1)) == {"W1"}             # lands on slice 0, before the pre-slice (1): the window is dropped
    # back to the seed: the seed's j is the largest there is, so the window is neither dropped nor cut
    assert events_of(_window(False, 0)) == set()
    # a window whose pre-slice is the seed is dropped by every redo that lands on a slice
    recs = [rec(0, cells=BIG, sparse=True), rec(64, cells=BIG, sparse=True), rec(128, cells=BIG, sparse=True), rec(64, bw=45), rec(128, bw=45)]
    assert "W1" in events_of(recs)
    # no window open (it was closed two slices ago): no W1
    assert "W1" not in events_of(_window(True, 1))


def test_classifier_w2():
    assert events_of(_window(True, 3)) == {"W2"}              # lands on slice 2, the closed window ends at 3: popped
    assert events_of(_window(True, 1)) == {"W2"}              # lands before the whole window
    assert events_of(_window(True, 4)) == set()               # lands on the window's last slice: it stays
    assert events_of(_window(True, 5)) == set()


def test_classifier_w3():
    assert events_of(_window(False, 2)) == {"W3"}             # lands on the pre-slice: the window's two slices lie behind it
    assert events_of(_window(False, 3)) == {"W3"}             # lands on the window's first slice
    # lands on the open window's last slice: nothing to cut
    recs = [rec(0), rec(64), rec(128, cells=BIG, sparse=True), rec(192, cells=BIG, sparse=True), rec(256, cells=BIG, sparse=True), rec(256, bw=45, cells=BIG, sparse=True)]
    assert events_of(recs) == {"L2"}
    # the classifier stops at a W3, as the run does
    out = ev.classify_direction(_window(False, 2) + [rec(256), rec(192, bw=45)], 45)
    assert len(out["redos"]) == 1


def test_classifier_u1():
    # slice 3 turns wrong: rampUntil = 3.  Back to slice 2; slice 3 at the ramp width has 200 000 cells -> rampUntil = 4, slice 4 still ramp
    recs = [rec(0, bw=45), rec(64), rec(128), rec(192), rec(128, bw=45), rec(192, bw=45, cells=BIG, sparse=True), rec(256, bw=45), rec(320)]
    out = ev.classify_direction(recs, 45)
    assert out["events"] == {"U1"} and out["u1"] == [5]
    # the big slice is 2, before rampUntil: nothing moves
    recs = [rec(0, bw=45), rec(64), rec(128), rec(192), rec(128, bw=45, cells=BIG, sparse=True), rec(192, bw=45), rec(256)]
    assert events_of(recs) == set()
    # one cell short of the cutoff
    recs = [rec(0, bw=45), rec(64), rec(128), rec(192), rec(128, bw=45), rec(192, bw=45, cells=BIG - 1, sparse=True), rec(256), rec(320)]
    assert events_of(recs) == set()
    # slice 0 always runs at the ramp width with rampUntil = 0
    assert events_of([rec(0, bw=45, cells=BIG, sparse=True), rec(64, bw=45), rec(128)]) == {"U1"}
    # no ramp width, no U1
    assert events_of([rec(0, bw=20, cells=BIG, sparse=True), rec(64, bw=20), rec(128)], ramp=0) == set()


def test_classifier_ck():
    # 16 slices: a checkpoint every 4.  Slice 1 is the cheapest so far (one node) and sparse; slice 2 turns wrong and the pass returns to
    # the seed, computes slices 0 .. 4 again -- and at slice 4 stores the OLD slice 1 as a checkpoint
    mk = lambda sparse: [rec(0), rec(64, sparse=sparse, nodes=1), rec(128)] + [rec(64 * k, bw=45) for k in range(6)]
    out = ev.classify_direction(mk(True), 45, 16)
    assert out["events"] == {"CK"} and out["ck"] == [1]
    assert events_of(mk(False), n_slices=16) == set()
    assert events_of(mk(True)) == set()                       # (without the slice count the checkpoints are not replayed)
    # without the redo the same checkpoint is the kept slice itself
    assert events_of([rec(0), rec(64, sparse=True, nodes=1)] + [rec(64 * k) for k in range(2, 6)], n_slices=16) == set()


def test_classifier_keeps_directions_apart():
    fw = [rec(0), rec(64), rec(128, sparse=True, partial={7: 9}), rec(192), rec(192, bw=45), rec(256, bw=45)]
    bwd = [rec(64 * k, direction=1) for k in range(4)]
    mixed = bwd[:2] + fw + bwd[2:]           # (the oracle records the backward part first, but nothing here relies on that)
    out = ev.classify(mixed, 45)
    assert out["events"] == {"L1", "L1b"} and out["n_redos"] == 1 and out["n_sparse_landings"] == 1 and out["n_partial"] == [1]
    assert out["directions"][1]["redos"] == []


# ---- the fixed reads: the oracle alone ------------------------------------------------------------------------------------------
def test_case_list_shows_its_events_on_the_oracle():
    counts = rc.check_conditions()
    print(counts)
    assert counts["W3"] == 0          # not found by the search; a read that shows it belongs in the list


# ---- the emulated device program against the oracle ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    return pc.emul_lib_path()


@pytest.fixture(params=[(0, 0), (1, 0), (0, 1), (1, 1)], ids=["fresh", "poison", "reuse", "poison+reuse"])
def switches(request, monkeypatch):
    poison, reuse = request.param
    monkeypatch.setenv("GA_EMUL_POISON", str(poison))
    monkeypatch.setenv("GA_EMUL_REUSE", str(reuse))
    return request.param


TRACE = pytest.mark.parametrize("trace", [True, False], ids=["trace-items", "flags-0"])


def run_batch(graph, reads, seeds, bw, ramp, trace, lib_path):
    gg = binding.Graph(graph.nodes, graph.edges, lib_path=lib_path)
    b = gg.prepare(reads, [[s] for s in seeds], bw, ramp, binding.GA_F_TRACE if trace else 0)
    b.run()
    return b.collect()


@TRACE
def test_redo_cases_equal_the_oracle(lib, switches, trace):
    rc.check_conditions()
    for fan, g, reads, seeds, descs, oras, classes in rc.batches():
        devs = run_batch(g, reads, seeds, fan[4], fan[5], trace, lib)
        assert len(devs) == len(reads)
        for d, o, desc, c in zip(devs, oras, descs, classes):
            pc.compare_read(d, pc.expected(o, trace), "fan %s draw %d %s" % (fan, desc[2], sorted(c["events"])))
        rc.check_sparse_reads_climbed(devs, oras)


@TRACE
def test_capacity_miss_is_loud_and_named(lib, switches, trace):
    """status 10 (GA_S_CAPACITY) for the reads named in redo_sparse_cases.CAPACITY_MISSES and for no other; every other read of the
    batch equals the oracle"""
    g, reads, seeds, draws, oras = rc.capacity_batch()
    fan = rc.CAPACITY_FAN
    devs = run_batch(g, reads, seeds, fan[4], fan[5], trace, lib)
    missed = sorted(draw for d, draw in zip(devs, draws) if d["status"] == 10)
    assert missed == sorted(rc.CAPACITY_MISSES), missed
    assert all(d["failed"] for d, draw in zip(devs, draws) if draw in rc.CAPACITY_MISSES)
    for d, o, draw in zip(devs, oras, draws):
        if draw not in rc.CAPACITY_MISSES:
            pc.compare_read(d, pc.expected(o, trace), "40 branches, draw %d" % draw)
    assert sum(1 for o, draw in zip(oras, draws) if rc.aligned(o) and draw not in rc.CAPACITY_MISSES) >= 2
