"""Bands of 200 000 cells and more with more than 256 nodes on the GPU: the ladder's last pass (ga_wide_sparse_kernel: the sparse
method and the backtrace override with 4 096 band nodes, the wave's state and tables in its scratch slot in HBM) through the
product library, against the oracle, every field.  Cases: wide_sparse_cases.py; the host emulation of the same cases is in
test_wide_sparse.py.  Without the pass every fan read here ends as GA_S_CAPACITY (status 10)."""
import functools
import re

import numpy as np
import pytest

from graphaligner_amd import binding, synth
import parity_cases as cases
import parity_common as pc
import wide_cases as wc
import wide_sparse_cases as wsc

pytestmark = pytest.mark.gpu

SPARSE_256 = "<256,1,sparse>"
SPARSE_4096 = "<4096,1,sparse>"
_LEFT = re.compile(r"wave-per-read pass <(\d+),(\d+)(,sparse)?>: \d+ jobs on \d+ slots, [0-9.]+ ms, (\d+) left with GA_CAP_NODES")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need a real MI355X"


@pytest.fixture(autouse=True, params=["lanes-first", "by-graph-shape"])
def _first_pass(request, monkeypatch):
    """every test runs twice, as in test_gpu_parity.py: the lanes = reads kernel forced as the first pass, and the library's own choice"""
    monkeypatch.setenv("GA_DEBUG_PASSES", "1")
    monkeypatch.delenv("GA_TEST_WAVE_SLOTS", raising=False)
    if request.param == "lanes-first":
        monkeypatch.setenv("GA_LANES", "1")
    else:
        monkeypatch.delenv("GA_LANES", raising=False)


def _passes(capfd):
    """(the debug lines as parity_cases reads them, {variant: jobs that pass left with GA_CAP_NODES})"""
    err = capfd.readouterr().err
    print(err, end="")          # (shown with a failure, and with -s: the pass times are read off these lines)
    left = {"<%s,%s%s>" % (m.group(1), m.group(2), m.group(3) or ""): int(m.group(4)) for m in _LEFT.finditer(err)}
    return cases.debug_passes(err), left


def _took_what_was_left(passes, left):
    """the new pass took exactly the jobs <256,true,true> left with GA_CAP_NODES -> how many"""
    line = cases.passes_of(passes, SPARSE_4096)
    assert len(line) == 1, passes
    assert line[0][1] == left[SPARSE_256] and line[0][1] > 0, (line, left)
    return line[0][1]


@pytest.mark.parametrize("trace", [True, False], ids=["trace-items", "flags-0"])
@pytest.mark.parametrize("name", list(wsc.CASES))
def test_parity(name, trace, capfd):
    capfd.readouterr()
    devs, oras = wsc.check_case(name, trace=trace, ctx=name)
    passes, left = _passes(capfd)
    assert _took_what_was_left(passes, left) >= 3


def test_the_limit(capfd):
    capfd.readouterr()
    wsc.check_limit()
    passes, left = _passes(capfd)
    assert _took_what_was_left(passes, left) >= 1


def test_one_slot_serves_job_after_job(capfd, monkeypatch):
    """GA_TEST_WAVE_SLOTS=1: one wave, so one state and one set of sparse tables in HBM, takes the jobs of a case one after the other
    and finds the leavings of the job before"""
    monkeypatch.setenv("GA_TEST_WAVE_SLOTS", "1")
    capfd.readouterr()
    wsc.check_case("300x700-ramp", ctx="one slot")
    passes, left = _passes(capfd)
    line = cases.passes_of(passes, SPARSE_4096)[0]
    assert line[2] == 1 and line[1] >= 3, line
    _took_what_was_left(passes, left)


@functools.lru_cache(maxsize=None)
def mixed_batch():
    """(nodes, edges, reads, seeds, which reads are fan reads), built once per process and left unchanged, in the manner of
    wide_cases.mixed_batch: the 300 x 700 fan and a chain of 64-bp nodes as two components of one graph; 60 ordinary reads on the chain
    and the fan's three reads, shuffled"""
    case = wsc.CASES["300x700"][0]
    branches = case[0]
    nodes, edges, fan_reads, fan_seeds = wsc.batch(case)
    chain = synth.SynthGraph(synth.random_genome(60000, 91), node_len=64, first_id=2 * branches + 3)
    nodes, edges = list(nodes) + list(chain.nodes), list(edges) + list(chain.edges)
    reads, seeds = synth.simulate_reads(chain, 60, 1000, seed=92)
    is_fan = [False] * len(reads) + [True] * len(fan_reads)
    reads, seeds = list(reads) + list(fan_reads), list(seeds) + list(fan_seeds)
    order = np.random.default_rng(94).permutation(len(reads))
    return nodes, edges, [reads[i] for i in order], [seeds[i] for i in order], [is_fan[i] for i in order]


def test_mixed_batch(capfd):
    """fan reads next to ordinary reads in one batch: every read equals the oracle; only the fan reads reach the new pass, the
    ordinary reads report the pass they report when run alone; a second run of the batch gives the same"""
    case = wsc.CASES["300x700"][0]
    nodes, edges, reads, seeds, is_fan = mixed_batch()
    oras = pc.oracle_results(nodes, edges, reads, seeds, case[4])
    g = binding.Graph(nodes, edges)
    b = g.prepare(reads, [[s] for s in seeds], case[4], 0, binding.GA_F_TRACE)
    capfd.readouterr()
    b.run()
    first = b.collect()
    passes, left = _passes(capfd)
    for i, (d, o) in enumerate(zip(first, oras)):
        pc.compare_read(d, o, "mixed batch, read %d" % i)
    assert all(o["status"] == 0 for o in oras)
    assert all(o["sparse_slices"] >= 1 for o, f in zip(oras, is_fan) if f) and all(o["sparse_slices"] == 0 for o, f in zip(oras, is_fan) if not f)
    assert _took_what_was_left(passes, left) == sum(is_fan), passes
    fan_pass = {d["kernel_pass"] for d, f in zip(first, is_fan) if f}
    chain_pass = {d["kernel_pass"] for d, f in zip(first, is_fan) if not f}
    assert len(fan_pass) == 1 and max(chain_pass) < min(fan_pass), (fan_pass, chain_pass)
    alone = binding.Graph(nodes, edges).align([r for r, f in zip(reads, is_fan) if not f], [s for s, f in zip(seeds, is_fan) if not f], case[4], 0, flags=binding.GA_F_TRACE)
    assert [d["kernel_pass"] for d, f in zip(first, is_fan) if not f] == [d["kernel_pass"] for d in alone]
    b.run()
    cases.same_results(first, b.collect(), "mixed batch, second run")


def test_no_new_pass_without_such_jobs(capfd):
    """a batch of ordinary reads sees no launch of the new pass"""
    chain = synth.SynthGraph(synth.random_genome(20000, 95), node_len=64)
    reads, seeds = synth.simulate_reads(chain, 8, 800, seed=96)
    capfd.readouterr()
    pc.check_parity(chain.nodes, chain.edges, reads, seeds, 35, ctx="chain")
    passes, _ = _passes(capfd)
    assert not [p for p in passes if p[0] == SPARSE_4096], passes
