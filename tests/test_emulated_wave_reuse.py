"""What a job finds in its buffers.  On the device a wave's scratch slot and its LDS are never cleared: a wave's first job meets
whatever the allocation held, every later one the leavings of the job before -- a longer read, a job that ended in an assertion, a
sparse-method job whose generation-stamped tables are zeroed once per launch.  The emulated back end (tests/emul) normally gives
every job freshly zeroed buffers; its two switches take that comfort away:

  GA_EMUL_POISON=1   every buffer a job or a lanes group gets is filled with 0xA5 first (not the sparse tables)
  GA_EMUL_REUSE=1    one WaveState and one set of slot buffers per wave-per-read variant, one scratch + LDS image per lanes
                     variant, kept and never cleared across the jobs / groups of a run, as by a wave that takes job after job

Each switch off / on (both off is what test_device_logic_emulated.py runs), every case against the oracle, every field.  The
block flush, the shared arena and the 64 / 32 / 16 lane strides of the real lanes kernel are not emulated: test_gpu_waves.py."""
import pytest

import parity_cases as cases
import parity_common as pc


@pytest.fixture(scope="module")
def lib():
    return pc.emul_lib_path()


@pytest.fixture(autouse=True, params=[(1, 0), (0, 1), (1, 1)], ids=["poison", "reuse", "poison+reuse"])
def _switches(request, monkeypatch):
    poison, reuse = request.param
    monkeypatch.setenv("GA_EMUL_POISON", str(poison))
    monkeypatch.setenv("GA_EMUL_REUSE", str(reuse))


def test_linear(lib):
    cases.case_wave_primitives_on_hardware(lib)


@pytest.mark.parametrize("node_len,snp,indel,sv", [(64, 100, 1000, 0), (8, 15, 60, 0)])
def test_random_graphs(lib, node_len, snp, indel, sv):
    cases.case_random_graphs(node_len, snp, indel, sv, lib)


def test_cyclic_graphs(lib):
    cases.case_cyclic_graphs(8, 35, 8, 2, 5, lib)


def test_ramp_redo(lib):
    cases.case_ramp_redo(16, 10, 40, 0.06, lib)


def test_short_and_edge_reads(lib):
    cases.case_short_and_edge_reads(lib)


def test_sparse_method_and_override(lib):
    cases.case_sparse_method_and_override(8, 30000, 150, 600, 35, 0, lib)


def test_sparse_sharp_edges(lib):
    cases.case_sparse_sharp_edges(lib)


@pytest.mark.parametrize("trace", [True, False], ids=["trace-items", "flags-0"])
def test_mixed_exits_on_one_wave(lib, trace):
    cases.case_mixed_exits_on_one_wave(lib, trace)
