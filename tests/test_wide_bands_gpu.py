"""Bit-vector bands of more than 256 nodes on the GPU: the ladder's pass with 4 096 band nodes (ga_wide_kernel: the wave's band
tables in its scratch slot in HBM) through the product library, against the oracle, every field.  Cases: wide_cases.py; the host
emulation of the same cases is in test_wide_bands.py.  Without the pass every fan read here ends as GA_S_CAPACITY (status 10)."""

import pytest

from graphaligner_amd import binding
import parity_cases as cases
import parity_common as pc
import wide_cases as wc

pytestmark = pytest.mark.gpu

WIDE = "<4096,1>"


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
    err = capfd.readouterr().err
    print(err, end="")          # (shown with a failure, and with -s)
    return cases.debug_passes(err)


@pytest.mark.parametrize("name", ["300x64", "600x16", "2000x12", "cyclic-700x16-ramp"])
def test_parity(name, capfd):
    capfd.readouterr()
    devs, oras = wc.check_case(wc.CASES[name], ctx=name)
    # the three reads through the fan were finished by the pass this is about (and by a later pass than the first: check_case)
    line = cases.passes_of(_passes(capfd), WIDE)[0]
    assert line[1] >= 3, line


def test_the_limit(capfd):
    capfd.readouterr()
    wc.check_limit()
    assert cases.passes_of(_passes(capfd), WIDE)[0][1] >= 3


def test_mixed_batch(capfd):
    """fan reads next to ordinary reads in one batch: every read equals the oracle; the pass number the fan reads report is that of
    the wide pass, the ordinary reads report what they report when run alone; a second run of the batch gives the same"""
    nodes, edges, reads, seeds, is_fan = wc.mixed_batch()
    oras = pc.oracle_results(nodes, edges, reads, seeds, 35)
    g = binding.Graph(nodes, edges)
    b = g.prepare(reads, [[s] for s in seeds], 35, 0, binding.GA_F_TRACE)
    capfd.readouterr()
    b.run()
    first = b.collect()
    passes = _passes(capfd)
    for i, (d, o) in enumerate(zip(first, oras)):
        pc.compare_read(d, o, "mixed batch, read %d" % i)
    assert all(o["status"] == 0 and o["sparse_slices"] == 0 for o in oras)
    assert cases.passes_of(passes, WIDE)[0][1] == 4, passes
    fan_pass = {d["kernel_pass"] for d, f in zip(first, is_fan) if f}
    assert len(fan_pass) == 1 and 0 not in fan_pass, fan_pass
    alone = binding.Graph(nodes, edges).align([r for r, f in zip(reads, is_fan) if not f], [s for s, f in zip(seeds, is_fan) if not f], 35, 0, flags=binding.GA_F_TRACE)
    assert [d["kernel_pass"] for d, f in zip(first, is_fan) if not f] == [d["kernel_pass"] for d in alone]
    b.run()
    cases.same_results(first, b.collect(), "mixed batch, second run")


def test_one_slot_serves_job_after_job(capfd, monkeypatch):
    """GA_TEST_WAVE_SLOTS=1: one wave, so one state in HBM, takes the fan jobs one after the other and finds the leavings of the job before"""
    monkeypatch.setenv("GA_TEST_WAVE_SLOTS", "1")
    capfd.readouterr()
    wc.check_case(wc.CASES["300x64"], ctx="one slot")
    line = cases.passes_of(_passes(capfd), WIDE)[0]
    assert line[2] == 1 and line[1] >= 3, line
