"""GPU parity for the two builds of the lanes = reads kernel's traceback (csrc/ga_lanes.h, lane_finish<N, FORM>): every size of the
kernel exists once per output form, node runs (`ga_lanes_kernel`) and moves (`ga_lanes_moves_kernel`), and the host emulation runs
neither of them: it keeps the form that is chosen at run time.  So the same reads go through the device three times --

  * as they come: no result needs a cell list, the kernel hands back node runs (batch statistics `reserved` = 1) where the host
    chooses them, which it does for graphs whose nodes are 40 bp long and more on average,
  * with flags = GA_F_TRACE: moves, and TraceItem lists from the host's replay of them,
  * with GA_RUNS=0 and no flags: moves (`reserved` = 0),

-- with GA_LANES=1 (the lanes kernel goes first) in full waves (GA_LANES_SPREAD=0).  The three runs must agree read by read, each must
equal the CPU oracle (parity_common.compare_read), and the first pass must have finished the reads itself (every read of the linear
graph, nine of ten of the bubble graph's: the seeds below were checked for that with the host emulation), or the test would say
nothing about these kernels.

Batches: 96 reads = one full wave and one of 32 lanes, 300 to 1 500 bp long (five slices and more; the short reads are done while the
others still trace) on a chain and on bubble graphs of 64-bp nodes; and 40 reads of 3 000 bp on the chain: many window refills and
slice crossings within one lane's bursts.

The bubble graph that carries the checks above is "bubbles-runs": synth.bubble_graph(30000, node_len=64) with a SNP every 300 bp
(43 bp per node on average), where the first run is the node-run kernel and the ten band nodes of <10,64> hold nine reads of ten
(91 of 96 on the host emulation and on the device).  The generator's default, a SNP every 100 bp ("bubbles"), has nodes of 24 bp on
average: the host chooses moves for it in all three runs, and the device's ladder starts such a graph with the wider <24,32>, which
finishes the reads (96 of 96): that case is the moves build of <24,32> three times, with and without the replay of the moves, under
the same nine-in-ten condition.  (The host emulation starts it with <10,64>, whose ten band nodes hold 18 reads of 96.)"""
import functools

import pytest

from graphaligner_amd import binding, synth
import parity_cases as cases
import parity_common as pc

pytestmark = pytest.mark.gpu

LENGTHS = (300, 450, 600, 800, 950, 1100, 1300, 1500)           # 12 reads of each
FORMS = ("runs", "trace-items", "moves")
SAME = ("status", "failed", "score", "query_position", "alignment_start", "alignment_end", "mappings")


@functools.lru_cache(maxsize=None)
def batch(name):
    """(graph, reads, seeds, share of the reads that the first pass must finish), built once per process and left unchanged"""
    if name == "linear":
        g, seed, first = synth.linear_graph(30000, node_len=64, seed=61), 100, 1.0
    elif name == "bubbles":
        g, seed, first = synth.bubble_graph(30000, node_len=64, seed=62), 200, 0.9
    elif name == "bubbles-runs":
        g, seed, first = synth.bubble_graph(30000, node_len=64, seed=63, snp_every=300), 400, 0.9
    else:
        g = synth.linear_graph(30000, node_len=64, seed=61)
        reads, seeds = synth.simulate_reads(g, 40, 3000, 0.04, 0.04, 0.04, seed=300)
        return g, reads, seeds, 1.0
    reads, seeds = [], []
    for k, length in enumerate(LENGTHS):
        r, s = synth.simulate_reads(g, 12, length, 0.04, 0.04, 0.04, seed=seed + k)
        reads, seeds = reads + r, seeds + s
    return g, reads, seeds, first


def run_forms(name, monkeypatch, lib_path=None):
    """the batch in the three forms -> {form: (results, batch statistics)}; every read compared with the oracle"""
    g, reads, seeds, _ = batch(name)
    oras = pc.oracle_results(g.nodes, g.edges, reads, seeds, 35)
    gg = binding.Graph(g.nodes, g.edges, lib_path=lib_path)
    monkeypatch.setenv("GA_LANES", "1")
    monkeypatch.setenv("GA_LANES_SPREAD", "0")
    monkeypatch.delenv("GA_TEST_WAVE_SLOTS", raising=False)
    out = {}
    for form in FORMS:
        if form == "moves":
            monkeypatch.setenv("GA_RUNS", "0")
        else:
            monkeypatch.delenv("GA_RUNS", raising=False)
        out[form] = cases.run_compared(gg, reads, seeds, oras, 35, trace=form == "trace-items", ctx="%s as %s" % (name, form))
    return out


def check_forms(name, out, on_device=True):
    _, reads, _, first = batch(name)
    for form in FORMS:
        devs, stats = out[form]
        assert stats["reserved"] == (1 if form == "runs" and name != "bubbles" else 0), (name, form, "output form", stats["reserved"])
        # (the narrow variant goes first on graphs of long nodes; the default bubble graph starts with a wider one)
        assert not on_device or stats["main_variant"] == 10080 or (name == "bubbles" and stats["main_variant"] % 1000 in (80, 81)), (name, form, stats["main_variant"])
        done = sum(1 for d in devs if d["kernel_pass"] == 0)
        print("%s as %s: %d of %d reads finished by the first pass" % (name, form, done, len(devs)))
        assert done >= first * len(devs) or (name == "bubbles" and not on_device), (name, form, "finished by the first pass", done, len(devs))
    for form in FORMS[1:]:
        for i, (x, y) in enumerate(zip(out["runs"][0], out[form][0])):
            for key in SAME:
                assert x[key] == y[key], (name, "runs against", form, "read", i, key, x[key], y[key])


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need a real MI355X"


@pytest.mark.parametrize("name", ["linear", "bubbles", "bubbles-runs", "long-chain"])
def test_three_forms_agree_and_equal_the_oracle(name, monkeypatch, capfd):
    monkeypatch.setenv("GA_DEBUG_PASSES", "1")
    capfd.readouterr()
    out = run_forms(name, monkeypatch)
    err = capfd.readouterr().err
    print(err, end="")
    check_forms(name, out)
    # what ran first, once per form: the narrow variant over all reads in full waves
    n = len(batch(name)[1])
    firsts = [p for p in cases.debug_passes(err) if p[0] in ("<10,64>", "<24,32>", "<56,16>") and p[1] == n]
    assert len(firsts) == 3, cases.debug_passes(err)
    assert name == "bubbles" or all(p == ("<10,64>", n, (n + 63) // 64, 64) for p in firsts), cases.debug_passes(err)
