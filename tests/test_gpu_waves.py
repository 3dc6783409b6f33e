"""GPU parity for what the product does on every real run and no small batch reaches by itself:

  * FULL waves of the lanes = reads kernel (64 / 32 / 16 job lanes, not the 8 a small batch is spread to): the block flush over
    all lanes, the wave's shared arena, the spare block of lanes without a node in a round, the LDS strides of 64 / 32 / 16;
  * a wave that takes a SECOND group (lanes kernel) or job (wave-per-read ladder) and so starts on the leavings of the one before
    in its LDS and its scratch slot: GA_TEST_WAVE_SLOTS caps the waves a launch starts;
  * the lanes ladder's hop to a wider variant as a later pass (512 jobs and more left over).

Every read of every batch is compared with the CPU oracle, bit for bit (a capacity status is a failure), with TraceItem lists and
with flags = 0, and every test reads the library's GA_DEBUG_PASSES lines to assert that the kernel variant, the job count and the
wave count it was written for are what ran: a test that cannot find its line fails.  Cases: parity_cases.py."""
import types

import pytest

import parity_cases as cases

pytestmark = pytest.mark.gpu

TRACE = pytest.mark.parametrize("trace", [True, False], ids=["trace-items", "flags-0"])
LANES_VARIANTS = {"<10,64>": (10, 64), "<24,32>": (24, 32), "<56,16>": (56, 16)}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need a real MI355X"


@pytest.fixture(autouse=True)
def _debug_lines(monkeypatch):
    monkeypatch.setenv("GA_DEBUG_PASSES", "1")
    for name in ("GA_LANES", "GA_LANES_SPREAD", "GA_TEST_WAVE_SLOTS"):
        monkeypatch.delenv(name, raising=False)


def run_batch(capfd, graph, reads, seeds, oras, trace, ctx):
    """-> (results, statistics, debug lines) of one batch, every read compared with the oracle"""
    capfd.readouterr()
    devs, stats = cases.run_compared(graph, reads, seeds, oras, 35, trace=trace, ctx=ctx)
    err = capfd.readouterr().err
    print(err, end="")          # (shown with a failure, and with -s)
    return devs, stats, cases.debug_passes(err)


# ---- C1: full waves, each lanes variant --------------------------------------------------------------------------------
_FULL = {}


def full_wave_results(monkeypatch, capfd, variant, trace, mid_seed=False):
    """the batches of `variant` in full waves, no cap on the waves: [(results, statistics, debug lines)], run once per process"""
    key = (variant, trace, mid_seed)
    if key not in _FULL:
        monkeypatch.setenv("GA_LANES", "1")
        monkeypatch.setenv("GA_LANES_SPREAD", "0")
        monkeypatch.delenv("GA_TEST_WAVE_SLOTS", raising=False)
        _FULL[key] = [run_batch(capfd, g, reads, seeds, oras, trace, "%s %s" % (variant, name)) for name, g, reads, seeds, oras in cases.wave_batches(variant, mid_seed)]
    return _FULL[key]


@TRACE
@pytest.mark.parametrize("variant,mid_seed", [("<10,64>", False), ("<24,32>", False), ("<56,16>", False), ("<10,64>", True)])
def test_full_waves(variant, mid_seed, trace, monkeypatch, capfd):
    """101 / 51 / 25 reads of mixed lengths with GA_LANES_SPREAD=0: one full wave of 64 / 32 / 16 lanes and a ragged one; with
    mid-read seeds 128 reads = 256 jobs (backward and forward parts) = four full waves"""
    n, lw = LANES_VARIANTS[variant]
    for (name, g, reads, seeds, oras), (devs, stats, passes) in zip(cases.wave_batches(variant, mid_seed), full_wave_results(monkeypatch, capfd, variant, trace, mid_seed)):
        n_jobs = 2 * len(reads) if mid_seed else len(reads)
        assert stats["n_jobs"] == n_jobs, (name, stats["n_jobs"])
        assert stats["main_variant"] == n * 1000 + 80 + (lw != 64), (name, stats["main_variant"])
        assert passes[0] == (variant, n_jobs, 4 if mid_seed else 2, lw), (name, passes)
        # (per read: the pass that finished the last of its jobs)
        assert sum(1 for d in devs if d["kernel_pass"] == 0) * 10 >= len(devs) * 9, (name, [d["kernel_pass"] for d in devs])


# ---- C2: one lanes wave takes group after group ---------------------------------------------------------------------------
@TRACE
@pytest.mark.parametrize("spread,slots", [(0, 1), (0, 2), (5, 1), (12, 3)])
@pytest.mark.parametrize("variant", ["<10,64>", "<24,32>", "<56,16>", "dense-short"])
def test_lanes_wave_takes_group_after_group(variant, spread, slots, trace, monkeypatch, capfd):
    """the C1 batches on at most `slots` waves.  Each batch is given TWICE in one run (its reads, then its reads again), so that
    under every setting a wave takes a second group (e.g. 2 x 25 jobs on 3 waves of 12 lanes; 25 alone would be one group each);
    both copies must equal the oracle's results and the full-wave run's.  Jobs are handed out longest first, so a later group is
    shorter than what its wave held before -- and in the dense-short batch needs more band nodes and more of the arena."""
    kernel = "<10,64>" if variant == "dense-short" else variant
    n, lw = LANES_VARIANTS[kernel]
    full = full_wave_results(monkeypatch, capfd, variant, trace)
    monkeypatch.setenv("GA_LANES", "1")
    monkeypatch.setenv("GA_LANES_SPREAD", str(spread))
    monkeypatch.setenv("GA_TEST_WAVE_SLOTS", str(slots))
    for (name, g, reads, seeds, oras), (full_devs, _, _) in zip(cases.wave_batches(variant), full):
        devs, stats, passes = run_batch(capfd, g, reads + reads, seeds + seeds, oras + oras, trace, "%s %s spread %d on %d waves" % (variant, name, spread, slots))
        cases.same_results(devs, full_devs + full_devs, name)
        lanes = min(lw, spread) if spread else lw
        line = passes[0]
        assert line == (kernel, 2 * len(reads), slots, lanes), (name, passes)
        assert line[1] > line[2] * line[3], (name, "no wave took a second group", line)
        # (the lanes kernel itself must finish these jobs, the dense-short batch's short reads included: a job it hands on to the
        # ladder is not a job that ran on another group's leavings)
        assert sum(1 for d in devs if d["kernel_pass"] == 0) * 10 >= len(devs) * 9, (name, [d["kernel_pass"] for d in devs])


# ---- C3: one ladder wave takes job after job ------------------------------------------------------------------------------
def ladder_lines(capfd, monkeypatch, slots, fn):
    """run a case of parity_cases.py with the wave-per-read kernels only, at most `slots` waves per launch
    -> (its debug lines, what the case returned)"""
    monkeypatch.setenv("GA_LANES", "0")
    monkeypatch.setenv("GA_TEST_WAVE_SLOTS", str(slots))
    capfd.readouterr()
    result = fn()
    err = capfd.readouterr().err
    print(err, end="")
    passes = cases.debug_passes(err)
    assert passes and all(p[2] <= slots for p in passes), passes
    return passes, result


def took_job_after_job(passes, variant, slots, min_jobs=None):
    """some launch of `variant` ran on `slots` waves with more jobs than that (and at least min_jobs)"""
    found = [p for p in cases.passes_of(passes, variant) if p[2] == slots and p[1] > slots and p[1] >= (min_jobs or 0)]
    assert found, (variant, "never had more jobs than waves", cases.passes_of(passes, variant))


SLOTS = pytest.mark.parametrize("slots", [1, 2])


@TRACE
@SLOTS
@pytest.mark.parametrize("node_len,snp,indel,sv", [(32, 40, 300, 3000), (5, 40, 0, 0)])
def test_ladder_wave_lean_variants(node_len, snp, indel, sv, slots, trace, monkeypatch, capfd):
    """<32,false> over everything, then <64,false> for what 32 band nodes do not hold; no read is let off"""
    passes, _ = ladder_lines(capfd, monkeypatch, slots, lambda: cases.case_random_graphs(node_len, snp, indel, sv, every_read=True, trace=trace))
    took_job_after_job(passes, "<32,0>", slots, 12)
    took_job_after_job(passes, "<64,0>", slots)
    if node_len == 5:
        took_job_after_job(passes, "<256,1>", slots)      # bands of more than 64 nodes of 5 bp (bandwidth 64)


@TRACE
@SLOTS
def test_ladder_wave_general_variant_cycles(slots, trace, monkeypatch, capfd):
    passes, (n_ok, n_all) = ladder_lines(capfd, monkeypatch, slots, lambda: cases.case_cyclic_graphs(8, 35, 8, 2, 5, trace=trace))
    took_job_after_job(passes, "<64,1>", slots)
    assert n_ok * 10 >= n_all * 9, (n_ok, n_all)


@TRACE
@SLOTS
def test_ladder_wave_general_variant_ramp(slots, trace, monkeypatch, capfd):
    passes, (n_ok, n_all) = ladder_lines(capfd, monkeypatch, slots, lambda: cases.case_ramp_redo(16, 10, 40, 0.06, trace=trace))
    took_job_after_job(passes, "<64,1>", slots)
    assert n_ok * 10 >= n_all * 9, (n_ok, n_all)


@TRACE
@SLOTS
@pytest.mark.parametrize("branches,branch_len,shared,stem,bw,ramp", [(8, 30000, 150, 600, 35, 0), (5, 50000, 100, 333, 35, 60)])
def test_ladder_wave_sparse_variant(branches, branch_len, shared, stem, bw, ramp, slots, trace, monkeypatch, capfd):
    """seven sparse jobs and more pass through one wave's generation-stamped tables, which are zeroed once per launch.
    (Seven reads, of which the oracle ends one of the first case's in an assertion: at the inputs the issue of this test fixes, six
    of seven align there, all seven in the second case -- so "nine reads of ten align" is asserted where it can hold.)"""
    passes, (devs, oras) = ladder_lines(capfd, monkeypatch, slots, lambda: cases.case_sparse_method_and_override(branches, branch_len, shared, stem, bw, ramp, trace=trace))
    took_job_after_job(passes, "<256,1,sparse>", slots, 7)
    n_ok = sum(1 for o in oras if o["status"] == 0 and not o["failed"])
    assert n_ok >= len(oras) - 1 and (branches != 5 or n_ok == len(oras)), (n_ok, len(oras))


@TRACE
@SLOTS
def test_ladder_wave_mixed_exits(slots, trace, monkeypatch, capfd):
    """an assertion, a normal job, a sparse job, the assertion again, degenerate reads, normal jobs: one after the other on one wave"""
    passes, _ = ladder_lines(capfd, monkeypatch, slots, lambda: cases.case_mixed_exits_on_one_wave(trace=trace))
    took_job_after_job(passes, "<32,0>", slots, 8)
    took_job_after_job(passes, "<256,1,sparse>", slots, 4)


# ---- C4: the lanes ladder's hop to a wider variant as a later pass ----------------------------------------------------------
@TRACE
@pytest.mark.parametrize("per_stretch", [600, 100])
def test_lanes_ladder_hop(per_stretch, trace, monkeypatch, capfd):
    """600 reads on a stretch of 8-bp nodes and 600 on one of 4-bp nodes overflow <10,64> and (the latter) <24,32>: 512 jobs and more
    are left over, so the wider variants get launches of their own; with 100 reads per stretch they must not, and the wave-per-read
    ladder finishes those jobs"""
    monkeypatch.setenv("GA_LANES", "1")
    nodes, edges, reads, seeds, stretch, oras = cases.hop_batch(per_stretch)
    g = types.SimpleNamespace(nodes=nodes, edges=edges)
    devs, stats, passes = run_batch(capfd, g, reads, seeds, oras, trace, "hop %d" % per_stretch)
    assert stats["main_variant"] == 10080
    assert passes[0][0] == "<10,64>" and passes[0][1] == len(reads), passes
    by_stretch = lambda which: [d["kernel_pass"] for d, s in zip(devs, stretch) if s == which]
    assert set(by_stretch(0)) == {0}
    if per_stretch == 600:
        assert [p[0] for p in passes[:3]] == ["<10,64>", "<24,32>", "<56,16>"], passes
        assert passes[1][1] >= 512 and passes[2][1] >= 512, passes
        # (the 8-bp reads are finished by the second pass, the 4-bp reads by the third; a few may climb further)
        assert by_stretch(1).count(1) * 10 >= per_stretch * 9 and by_stretch(2).count(2) * 10 >= per_stretch * 9
    else:
        assert [p[0] for p in passes if p[0] in LANES_VARIANTS] == ["<10,64>"], passes
        left = sum(1 for d in devs if d["kernel_pass"] > 0)
        assert left >= 2 * per_stretch * 9 // 10 and min(by_stretch(1) + by_stretch(2)) >= 1
        assert cases.passes_of(passes, "<64,0>")[0][1] == left, passes
