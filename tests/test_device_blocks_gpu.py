"""The device batches' blocks on the GPU: every stage of a batch borrows its device memory from the graph's block list and hands it
back, some of it before the batch ends (the seeded prepare's work arrays, the operations' counts, a pileup add's and a site query's
lists).  A block that went back early, or twice, would be handed to the next stage while the one before still uses it.  So on ONE
loaded graph the stages run in a row -- a plain batch, a GA_F_OPS batch, a GA_F_PILEUP batch added to a BASES and an EDGES pileup with
a folded site query on each, a seeded batch, the plain batch again, and the same reads as two halves through sharding.run_overlapped --
and every result must equal, bit for bit, what the same call gives on a graph loaded for that call alone; the plain batch must also be
the oracle's, field by field (parity_common).  Integers and bytes throughout: there is no tolerance."""
import numpy as np
import pytest

from graphaligner_amd import binding, sharding, synth
import parity_common as pc

pytestmark = pytest.mark.gpu
BW = 35


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need a real MI355X"


@pytest.fixture(autouse=True)
def _plain_settings(monkeypatch):
    for name in ("GA_LANES", "GA_LANES_SPREAD", "GA_TEST_WAVE_SLOTS", "GA_TEST_TRACE_POOL_BYTES"):
        monkeypatch.delenv(name, raising=False)


def _frozen(x):
    """a result as something that compares with ==: arrays as (dtype, shape, bytes), containers element by element"""
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, x.tobytes())
    if isinstance(x, dict):
        return tuple((k, _frozen(v)) for k, v in sorted(x.items()))
    if isinstance(x, (list, tuple)):
        return tuple(_frozen(v) for v in x)
    return x


def _plain(G, reads, seeds):
    return G.align(reads, seeds, BW, flags=binding.GA_F_TRACE)


def _ops(G, reads, seeds):
    return G.align(reads, seeds, BW, flags=binding.GA_F_OPS)


def _pileups(G, reads, seeds):
    b = G.prepare(reads, seeds, BW, flags=binding.GA_F_PILEUP)
    b.run()
    out = dict(reads=b.collect())
    for kind in ("bases", "edges"):
        pile = G.pileup(kind)
        pile.add(b)
        sites = pile.sites(fold=True)
        assert sites.total == len(sites) > 0, kind
        out[kind] = dict(counts=pile.counts(), sites=np.asarray(sites), total=sites.total)
        pile.close()
    b.close()
    return out


def _seeded(G, reads, seeds):
    return G.align_reads(reads, None, False, BW, 0, binding.GA_F_TRACE)


def _halves(G, reads, seeds):
    h = len(reads) // 2
    inputs = [(0, (reads[:h], seeds[:h])), (1, (reads[h:], seeds[h:]))]
    return sharding.run_overlapped(G, inputs, BW, flags=binding.GA_F_TRACE)


STEPS = [("plain", _plain), ("ops", _ops), ("pileups", _pileups), ("seeded", _seeded), ("plain again", _plain), ("two halves", _halves)]


def test_stages_in_a_row_on_one_graph_equal_each_on_a_fresh_graph():
    g = synth.bubble_graph(40000, node_len=32, seed=11)
    reads, seeds = synth.simulate_reads(g, 16, 1500, seed=5)
    reads2, seeds2 = synth.simulate_reads(g, 8, 1500, seed=6, mid_seed=True)
    reads, seeds = reads + reads2, seeds + seeds2

    def load():
        G = binding.Graph(g.nodes, g.edges)
        G.build_seed_index()
        return G

    # each call on a graph of its own ("plain again" is the plain call: one reference for both)
    want = {}
    for name, step in STEPS:
        if name != "plain again":
            want[name] = _frozen(step(load(), reads, seeds))
    want["plain again"] = want["plain"]

    worn = load()
    got = {}
    for name, step in STEPS:
        res = step(worn, reads, seeds)
        if name == "plain":
            oras = pc.oracle_results(g.nodes, g.edges, reads, seeds, BW)
            for i, (d, o) in enumerate(zip(res, oras)):
                pc.compare_read(d, o, "plain batch on the one graph, read %d" % i)
            assert sum(1 for d in res if not d["failed"]) >= 20
        got[name] = _frozen(res)
    for name, _ in STEPS:
        assert got[name] == want[name], "%s differs from the same call on a freshly loaded graph" % name
    # not vacuous: the halves are the plain batch's reads, so their results are the plain results
    assert tuple(r for _, part in got["two halves"] for r in part) == got["plain"]
    # the plain batch on a fresh graph through parity_common.check_parity: the reference above is the oracle's too
    devs, _ = pc.check_parity(g.nodes, g.edges, reads, seeds, BW, ctx="plain batch on a fresh graph")
    assert _frozen(devs) == want["plain"]
