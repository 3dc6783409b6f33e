"""Edge support (pileups of kind "edges") on the GPU: ga_pileup_edges_kernel and ga_pileup_slots_kernel through the product library, the
count of every slot against edge_model, which applies the rule to the oracle's TraceItem lists.  Cases: edge_cases.py; the host build of
the same program runs fabricated move streams in test_edge_pileup.py.  Counts are integers: there is no tolerance.  On a library without
the kind every test here fails at binding.GA_PILEUP_EDGES."""
import ctypes as C

import numpy as np
import pytest

from graphaligner_amd import binding, sharding
import edge_cases as ec
import edge_model as em
import pileup_cases as plc
import pileup_model as pm

pytestmark = pytest.mark.gpu

assert binding.GA_PILEUP_EDGES not in (binding.GA_PILEUP_BASES, binding.GA_PILEUP_DEPTH)
GUARD = 0xDEADBEEF


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need a real MI355X"


@pytest.fixture(autouse=True, params=["GA_LANES=1", "GA_LANES=0"])
def _first_pass(request, monkeypatch):
    """both first passes: the lanes = reads kernel (its own traceback writes the moves), and the wave-per-read kernels over everything"""
    monkeypatch.delenv("GA_TEST_WAVE_SLOTS", raising=False)
    monkeypatch.setenv("GA_LANES", request.param[-1])


@pytest.mark.parametrize("name", ec.BATCH_NAMES)
def test_counts_per_slot(name):
    """the batches of the CPU model: counts per slot = the model's plane, items_added = the model's items, edge_support() = the fold"""
    case = ec.batch_case(name)
    gg, pile, model, st, _ = ec.check_case(case)
    assert st["add_kernel_ms"] > 0
    if name == "alphabet":
        assert 0 < st["reads_from_host"] < st["reads_from_device"], st           # (the host's list contributes slot indices)
    if name == "several seeds":
        assert model.reads == len(case.reads) - 1 and st["jobs_walked"] <= 2 * model.reads
    if name == "one part and strands":
        assert any(model.counts.get((b ^ 1, a ^ 1), 0) > 0 for (a, b), c in model.counts.items() if c > 0)      # an edge and its mirror
    if name == "fan":
        t = gg.edge_slots()[1]                                                   # (a node's slots are consecutive: its place in each run)
        starts = np.flatnonzero(np.r_[True, t[1:] != t[:-1]])
        ordinal = np.arange(len(t)) - np.repeat(starts, np.diff(np.r_[starts, len(t)]))
        assert ordinal.max() == 9                                                 # (in-degree 10: the walk enters through in_nbr, past the node record's four)
    if name == "self-loop on a 40-bp node":
        assert model.counts == {(2, 4): 2, (4, 4): 1 + 2, (4, 6): 2}
    if name == "one-base self-loop":
        assert (4, 4) in model.edge_set and model.counts == {(2, 4): 2, (4, 6): 2}


def test_seeded_batch():
    ec.case_seeded_batch()


def test_cases_together_are_not_vacuous():
    """every case has at least two aligned reads and one counted crossing (check_case asserts it per case); together they have more than
    2 000 crossings.  From the oracle alone"""
    total = 0
    for name in ec.BATCH_NAMES:
        case = ec.batch_case(name)
        model = em.of(case.oracle(), case.graph().bp, case.slots)
        assert model.reads >= 2 and model.items >= 1, name
        total += model.items
    assert total > 2000, total


@pytest.mark.parametrize("slots", ["1", None], ids=["one-wave", "all-waves"])
def test_add_twice_reset_and_the_other_kinds(monkeypatch, slots):
    """adding twice doubles the counts and reset zeroes them; the same batch added to a BASES and a DEPTH pileup as well leaves those equal
    to pileup_model; a download into a buffer with guard words behind its end leaves them untouched; a sub-range is the slice of the whole and
    a range past the slots is refused.  (The dummy nodes' slots would have to be zero; graphs built through the loaders give the two dummy
    nodes no edges, so no slot of this graph -- or of any case here -- names id 0, which is asserted instead)"""
    if slots:
        monkeypatch.setenv("GA_TEST_WAVE_SLOTS", slots)
    case = ec.batch_case("one part and strands")
    gg = case.graph()
    oras = case.oracle()
    model = em.of(oras, gg.bp, case.slots)
    edges, bases, depth = gg.pileup("edges"), gg.pileup("bases"), gg.pileup("depth")
    devs, b = ec.run_add(gg, case.reads, case.seeds, case.bw, [bases, edges, depth])
    ec.compare(gg, edges, case.slots, model, ctx="once")
    pmodel = pm.of(oras, gg.bp)
    plc.compare(gg, bases, pmodel, ctx="bases next to edges")
    plc.compare(gg, depth, pmodel, ctx="depth next to edges")
    assert bases.stats()["items_added"] == pmodel.items and bases.stats()["columns"] == gg.bp and bases.counts().shape == (8, gg.bp)
    edges.add(b)
    ec.compare(gg, edges, case.slots, model, times=2, ctx="twice")
    st = edges.stats()
    assert st["items_added"] == 2 * model.items and st["batches_added"] == 2
    plc.compare(gg, bases, pmodel, ctx="bases after the second add to edges")
    # downloads: guard words, sub-ranges, refusals
    whole = edges.counts()
    n = len(case.slots)
    assert whole.shape == (1, n) and whole.any()
    L = gg.L
    for first, count in ((0, n), (0, 1), (1, 64), (63, 130), (n - 1, 1), (n, 0), (5, 0)):
        buf = np.full(count + 16, GUARD, dtype=np.uint32)
        assert L.ga_pileup_download(edges.h, first, count, buf.ctypes.data_as(C.c_void_p)) == 0, (first, count)
        assert (buf[:count] == whole[0, first:first + count]).all() and (buf[count:] == GUARD).all(), (first, count)
        assert (edges.counts(first, count) == whole[:, first:first + count]).all()
    buf = np.full(16, GUARD, dtype=np.uint32)
    for first, count in ((n - 2, 4), (n + 1, 0), (0, n + 1), (gg.bp - 2, 2) if gg.bp > n else (n, 1)):
        assert L.ga_pileup_download(edges.h, first, count, buf.ctypes.data_as(C.c_void_p)) == 100, (first, count)
    assert (buf == GUARD).all()
    with pytest.raises(RuntimeError, match=r"\(100\)"):
        edges.counts(n - 1, 2)
    f, t = gg.edge_slots()
    assert not ((f == 0) | (t == 0)).any() and gg.node_count == 2 * len(case.nodes) + 2
    with pytest.raises(ValueError):
        edges.node(1)
    with pytest.raises(ValueError):
        bases.edge_support()
    edges.reset()
    assert not edges.counts().any()
    st = edges.stats()
    assert st["items_added"] == 0 and st["batches_added"] == 0 and st["columns"] == n and st["kind"] == binding.GA_PILEUP_EDGES
    edges.add(b)
    ec.compare(gg, edges, case.slots, model, ctx="after reset")
    # a batch of another graph, and a kind that is none
    other = case.graph()
    foreign = other.pileup("edges")
    assert L.ga_batch_pileup_add(b.h, foreign.h) == 100 and not foreign.counts().any()
    h = C.c_void_p()
    assert L.ga_pileup_create(gg.h, 3, C.byref(h)) == 100 and L.ga_pileup_create(gg.h, 33, C.byref(h)) == 100


def test_sharding_takes_a_sequence_of_pileups():
    case = ec.batch_case("round edges 8")
    gg = case.graph()
    model = em.of(case.oracle(), gg.bp, case.slots)
    pmodel = pm.of(case.oracle(), gg.bp)
    reads, seeds = case.reads, case.seeds
    edges, bases = gg.pileup("edges"), gg.pileup("bases")
    halves = [(0, (reads[:5], seeds[:5])), (1, (reads[5:], seeds[5:]))]
    parts = dict(sharding.run_overlapped(gg, halves, case.bw, flags=ec.F_PILEUP, pileup=[edges, bases]))
    assert len(parts[0]) + len(parts[1]) == len(reads)
    ec.compare(gg, edges, case.slots, model, ctx="run_overlapped")
    plc.compare(gg, bases, pmodel, ctx="run_overlapped, bases")
    assert edges.stats()["batches_added"] == 2 and bases.stats()["batches_added"] == 2
    queued = gg.pileup("edges")
    alone = gg.pileup("depth")
    res = sharding.align_queued(gg, reads, seeds, case.bw, flags=ec.F_PILEUP, chunk_reads=4, pileup=(queued, alone))
    assert len(res) == len(reads)
    ec.compare(gg, queued, case.slots, model, ctx="align_queued")
    plc.compare(gg, alone, pmodel, ctx="align_queued, depth")
    one = gg.pileup("edges")
    sharding.align_queued(gg, reads, seeds, case.bw, flags=ec.F_PILEUP, chunk_reads=4, pileup=one)       # one pileup, as before
    assert (one.counts() == queued.counts()).all()


def test_graph_of_one_strand():
    """a graph whose other strand was never added (digraph-level calls, every interior twin none; reads cannot be seeded on it, as in the
    reference, which looks both strands of a seed's node up): a pileup of kind "edges" is made all the same -- its mirror-slot table,
    built from those twins, holds no slot --, is zero, has the graph's slots, and downloads and resets like any other"""
    case = ec.batch_case("round edges 8")
    one = binding.Graph.__new__(binding.Graph)
    one.L = binding.load(None)
    one.h = one.L.ga_graph_create()
    for nid, seq in case.nodes:
        assert one.L.ga_graph_add_node(one.h, 2 * nid, seq.encode(), len(seq), 0) == 0
        if nid % 5 == 0:                                       # (some nodes with both strands, most without)
            assert one.L.ga_graph_add_node(one.h, 2 * nid + 1, seq.encode(), len(seq), 1) == 0
    for f, fs, t, te in case.edges:
        assert not fs and not te
        assert one.L.ga_graph_add_edge(one.h, 2 * f, 2 * t) == 0
    assert one.L.ga_graph_finalize(one.h, 0) == 0 and one.L.ga_graph_upload(one.h, 0) == 0
    f, t = one.edge_slots()
    slots = list(zip(f.tolist(), t.tolist()))
    assert slots == [e for e in case.slots if e[0] % 2 == 0 and e[1] % 2 == 0] and len(slots) == len(case.edges)
    pile = one.pileup("edges")
    st = pile.stats()
    assert st["columns"] == len(slots) and st["kind"] == binding.GA_PILEUP_EDGES and pile.counts().shape == (1, len(slots))
    assert not pile.counts().any()
    pile.reset()
    assert not pile.counts(3, 7).any()
    devs = one.align(case.reads[:2], case.seeds[:2], case.bw)
    assert [d["status"] for d in devs] == [3] * 2                # (GA_S_BAD_SEED)
