"""Bit-vector bands of more than 256 nodes: the ladder's pass with 4 096 band nodes, checked on the host (tests/emul: the
device program with run_job<4096,true> behind <256,true>) against real libstdc++ containers and against the oracle.  The GPU
tests of the same cases are in test_wide_bands_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import oracle_binding as ob
import parity_common as pc
import wide_cases as wc


@pytest.fixture(scope="module")
def lib():
    return pc.emul_lib_path()


@pytest.fixture(scope="module")
def wide(lib):
    L = C.CDLL(lib)
    L.ga_emul_wide_hash_order.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.ga_emul_wide_unordered_map_order.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.ga_emul_wide_state_bytes.restype = C.c_uint64
    return L


# ---- the bucket schedule and the iteration order ----------------------------------------------------------------------------
SIZES = [257, 258, 541, 542, 1109, 1110, 2357, 2358, 4096]


def _keys(kind, n, rng):
    if kind == "random":
        return rng.choice(int(rng.choice([5000, 200000, 4000000])), size=n, replace=False).astype(np.uint32)
    # keys that collide: a few residues modulo the table size, so that while the table has that many buckets almost every key goes
    # into an occupied bucket
    mod = int(kind)
    residues = rng.choice(mod, size=3, replace=False)
    keys = (residues[rng.integers(0, 3, size=n)] + mod * np.arange(n)).astype(np.uint32)
    return rng.permutation(keys)


def test_bucket_schedule_of_this_libstdcxx(wide):
    """the growth the device code assumes: 13, 29, 59, 127, 257, 541, 1109, 2357, 5087 buckets, the table growing when the key arrives
    that no longer fits"""
    keys = np.arange(4096, dtype=np.uint32)
    out = np.zeros(4096, dtype=np.int64)
    buckets = np.zeros(4096, dtype=np.int32)
    assert wide.ga_emul_wide_unordered_map_order(keys.ctypes.data, 4096, out.ctypes.data, buckets.ctypes.data) == 4096
    schedule = [13, 29, 59, 127, 257, 541, 1109, 2357, 5087]
    for i in range(4096):
        assert buckets[i] == next(b for b in schedule if i + 1 <= b), (i, buckets[i])


@pytest.mark.parametrize("kind", ["random", "541", "1109"])
@pytest.mark.parametrize("n", SIZES)
def test_hash_order_equals_a_real_unordered_map(wide, n, kind):
    rng = np.random.default_rng(n * 7 + len(kind))
    L = ob.lib()
    L.gao_frozen_order.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_void_p]
    for trial in range(3):
        keys = _keys(kind, n, rng)
        assert len(set(keys.tolist())) == n
        out = np.zeros(n, dtype=np.int32)
        assert wide.ga_emul_wide_hash_order(keys.ctypes.data, n, out.ctypes.data) == n
        real = np.zeros(n, dtype=np.int64)
        assert wide.ga_emul_wide_unordered_map_order(keys.ctypes.data, n, real.ctypes.data, None) == n
        assert sorted(out.tolist()) == list(range(n))
        assert (keys[out].astype(np.int64) == real).all(), (n, kind, trial)
        # ... and the oracle's frozen slice (the map the reference iterates) agrees
        k64 = keys.astype(np.int64)
        o = np.zeros(n, dtype=np.int64)
        assert L.gao_frozen_order(ob._p(k64), n, int(keys.max()) + 1, ob._p(o)) == n
        assert (o == real).all()


def test_state_is_far_beyond_lds(wide):
    """why the state of this variant lies in HBM: some 190 bytes per band node against 160 KiB of LDS"""
    assert 160 * 1024 < wide.ga_emul_wide_state_bytes() < 1 << 20


# ---- parity with the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trace", [True, False], ids=["trace-items", "flags-0"])
@pytest.mark.parametrize("name", list(wc.CASES))
def test_parity(lib, name, trace):
    wc.check_case(wc.CASES[name], lib, trace=trace, ctx=name)


@pytest.mark.parametrize("switch", ["GA_EMUL_POISON", "GA_EMUL_REUSE"])
@pytest.mark.parametrize("name", ["300x64", "cyclic-700x16-ramp", "2000x12"])
def test_parity_with_unclean_buffers(lib, name, switch, monkeypatch):
    """the state is not cleared between jobs on the device (nor is LDS): poisoned before first use / one state for job after job"""
    monkeypatch.setenv(switch, "1")
    wc.check_case(wc.CASES[name], lib, ctx="%s %s" % (name, switch))


def test_new_ground(lib):
    """the ladder without the pass gives these reads up (GA_S_CAPACITY); with it they align"""
    nodes, edges, reads, seeds = wc.fan_batch(*[wc.CASES["300x64"][i] for i in (0, 1, 2, 3, 6)])
    with pc.emul_profile("emul"):
        old, _ = pc.run_both(nodes, edges, reads, seeds, 35, lib_path=lib)
    assert [d["status"] for d in old] == [10] * len(reads)
    with pc.emul_profile("emul_wide"):
        new, _ = pc.run_both(nodes, edges, reads, seeds, 35, lib_path=lib)
    assert [d["status"] for d in new] == [0] * len(reads)


def test_the_limit(lib):
    wc.check_limit(lib)
