"""Bands of 200 000 cells and more with more than 256 nodes: the ladder's last pass, run_job<4096,true,true> (the sparse method and
the backtrace override with 4 096 band nodes and the tables of SparseLimits<4096>), checked on the host (tests/emul); the ladder
without that pass is the same library with the pass withheld (parity_common.PROFILES).  The GPU tests of the same cases are in test_wide_sparse_gpu.py.  Without the pass every
fan read here ends as GA_S_CAPACITY (status 10)."""
import ctypes as C

import numpy as np
import pytest

import parity_common as pc
import redo_sparse_cases as rc
import wide_cases as wc
import wide_sparse_cases as wsc


@pytest.fixture(scope="module")
def lib():
    return pc.emul_lib_path()


@pytest.fixture(scope="module")
def hooks(lib):
    L = C.CDLL(lib)
    L.ga_emul_wide_sparse_node_slots.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.ga_emul_wide_sparse_node_map_size.restype = C.c_uint32
    L.ga_emul_wide_sparse_node_hash.argtypes = [C.c_uint32]
    L.ga_emul_wide_sparse_node_hash.restype = C.c_uint32
    L.ga_emul_wide_sparse_limits.argtypes = [C.c_void_p]
    L.ga_emul_wide_sparse_mem_bytes.argtypes = [C.c_int, C.c_uint32]
    L.ga_emul_wide_sparse_mem_bytes.restype = C.c_uint64
    L.ga_emul_wide_sparse_jobs_taken.restype = C.c_uint64
    return L


# ---- the hashed node -> slot lookup ---------------------------------------------------------------------------------------------
def _mix64(k):
    """ga_sparse.h's mix64 on an array of keys"""
    k = k.astype(np.uint64)
    k ^= k >> np.uint64(29)
    k *= np.uint64(0x9E3779B97F4A7C15)
    k ^= k >> np.uint64(32)
    return k & np.uint64(0xFFFFFFFF)


def _colliding_keys(hooks, n, size):
    """n distinct node numbers that fall into only three home positions of the table: almost every probe runs along a cluster"""
    keys = np.arange(3000000, dtype=np.uint64)
    home = _mix64(keys) & np.uint64(size - 1)
    picked = keys[np.isin(home, home[:3])][:n].astype(np.uint32)
    assert len(picked) == n and len(set(home[:3].tolist())) == 3
    assert {hooks.ga_emul_wide_sparse_node_hash(int(k)) for k in picked} == set(int(h) for h in home[:3])      # the test's hash is the table's
    return picked


@pytest.mark.parametrize("kind", ["random", "dense", "colliding"])
def test_node_slots_equal_a_dictionary(hooks, kind):
    """find-or-insert through the table gives every node the slot a plain dictionary gives it, slots are handed out in first-touch
    order, and a table started anew (next stamp) holds nothing of the round before"""
    rng = np.random.default_rng(len(kind))
    size = hooks.ga_emul_wide_sparse_node_map_size()
    assert size >= 4 * 4096 and size & (size - 1) == 0
    if kind == "random":
        nodes = rng.choice(4000000, size=4096, replace=False).astype(np.uint32)
    elif kind == "dense":
        nodes = (np.arange(4096) + 7).astype(np.uint32)          # a fan's branches: consecutive node numbers
    else:
        nodes = rng.permutation(_colliding_keys(hooks, 200, size))
    # every node touched several times, in an order that interleaves first touches with repeats
    touches = np.concatenate([nodes[: len(nodes) // 2], rng.choice(nodes[: len(nodes) // 2], size=len(nodes)), nodes, rng.permutation(nodes)]).astype(np.uint32)
    expect, order = {}, []
    for t in touches.tolist():
        if t not in expect:
            expect[t] = len(order)
            order.append(t)
    for rounds in (1, 2, 5):
        slots = np.full(len(touches), -7, dtype=np.int32)
        got_order = np.zeros(4096, dtype=np.uint32)
        n = hooks.ga_emul_wide_sparse_node_slots(touches.ctypes.data, len(touches), rounds, slots.ctypes.data, got_order.ctypes.data)
        assert n == len(order), (kind, rounds, n, len(order))
        assert slots.tolist() == [expect[t] for t in touches.tolist()], (kind, rounds)
        assert got_order[:n].tolist() == order, (kind, rounds)


def test_more_nodes_than_slots(hooks):
    touches = np.arange(4097, dtype=np.uint32)
    slots = np.zeros(4097, dtype=np.int32)
    order = np.zeros(4096, dtype=np.uint32)
    assert hooks.ga_emul_wide_sparse_node_slots(touches.ctypes.data, 4097, 1, slots.ctypes.data, order.ctypes.data) == -1


def test_limits_per_variant(hooks):
    """the 256 variant's tables are what they were (its capacity misses are pinned); the 4 096 variant's hold at least 2^17 cells per
    row (the row set is at most half full) and 2^18 touched columns"""
    v = np.zeros(10, dtype=np.uint32)
    hooks.ga_emul_wide_sparse_limits(v.ctypes.data)
    assert v[:5].tolist() == [1 << 14, 1 << 17, 1 << 16, 1 << 19, 0]
    set_size, map_size, words, entries, node_map = (int(x) for x in v[5:])
    assert set_size // 2 >= 1 << 17 and words >= 1 << 18 and map_size >= 2 * words and node_map >= 4 * 4096
    assert entries * (1 << 14) >= (1 << 19) * set_size          # the queue in proportion to the cells of a row
    up = lambda x: (x + 255) & ~255
    for bw in (1, 10, 35, 70):
        assert hooks.ga_emul_wide_sparse_mem_bytes(256, bw) == 256 + up(8 * (bw + 1)) + (16 << 19) + (12 << 14) + (16 << 17) + (36 << 16) + (8 << 16)
        assert hooks.ga_emul_wide_sparse_mem_bytes(4096, bw) > hooks.ga_emul_wide_sparse_mem_bytes(256, bw)


# ---- parity with the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trace", [True, False], ids=["trace-items", "flags-0"])
@pytest.mark.parametrize("name", list(wsc.CASES))
def test_parity(lib, hooks, name, trace):
    devs, oras = wsc.check_case(name, lib, trace=trace, ctx=name)
    # the reads went through the new pass (the tail-seeded read's backward part may not)
    assert hooks.ga_emul_wide_sparse_jobs_taken() >= 3


def test_enough_reads_align_over_sparse_slices():
    """the suite does not pass on assertions alone"""
    total = 0
    for name, (case, statuses, sparse) in wsc.CASES.items():
        nodes, edges, reads, seeds = wsc.batch(case)
        oras = pc.oracle_results(nodes, edges, reads, seeds, case[4], case[5])
        wsc.check_oracle(name, oras)
        total += wsc.sparse_aligned(oras)
    assert total >= wsc.MIN_SPARSE_ALIGNED, total


@pytest.mark.parametrize("switch", ["GA_EMUL_POISON", "GA_EMUL_REUSE"])
@pytest.mark.parametrize("name", wsc.SMALLEST)
def test_parity_with_unclean_buffers(lib, name, switch, monkeypatch):
    """the state and the tables are not cleared between jobs on the device: poisoned before first use / one state, one set of
    tables for job after job"""
    monkeypatch.setenv(switch, "1")
    wsc.check_case(name, lib, ctx="%s %s" % (name, switch))


def test_new_ground(lib):
    """the ladder without the pass gives these reads up (GA_S_CAPACITY); with it they align"""
    case = wsc.CASES["300x700"][0]
    nodes, edges, reads, seeds = wsc.batch(case)
    with pc.emul_profile("emul_wide"):
        old, _ = pc.run_both(nodes, edges, reads, seeds, case[4], lib_path=lib)
    assert [d["status"] for d in old] == [10] * len(reads)
    with pc.emul_profile("emul_wide_sparse"):
        new, _ = pc.run_both(nodes, edges, reads, seeds, case[4], lib_path=lib)
    assert [d["status"] for d in new] == [0] * len(reads)


def test_the_limit(lib):
    wsc.check_limit(lib)


# ---- the two ladders agree where the new pass has nothing to do ---------------------------------------------------------------------
def _same(a, b, ctx, columns=True):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        for key in ("status", "failed", "score", "query_position", "alignment_start", "alignment_end", "mappings") + (("columns",) if columns else ()):
            assert x[key] == y[key], (ctx, "read", i, key, x[key], y[key])
        assert x["trace"].shape == y["trace"].shape and (x["trace"] == y["trace"]).all(), (ctx, "read", i, "trace items")


def test_ladders_agree_on_a_wide_bit_vector_case(lib, hooks):
    case = wc.CASES["300x64"]
    nodes, edges, reads, seeds = wc.fan_batch(*[case[i] for i in (0, 1, 2, 3, 6)])
    with pc.emul_profile("emul_wide"):
        a, _ = pc.run_both(nodes, edges, reads, seeds, case[4], ramp=case[5], lib_path=lib)
    with pc.emul_profile("emul_wide_sparse"):
        b, _ = pc.run_both(nodes, edges, reads, seeds, case[4], ramp=case[5], lib_path=lib)
    assert hooks.ga_emul_wide_sparse_jobs_taken() == 0
    _same(a, b, "300x64")
    assert [d["status"] for d in b] == [0] * len(reads)


def test_ladders_agree_on_the_bit_vector_limit(lib):
    """here the new pass has something to do: by the product's rule (ga_ladder.h) it takes every job that <256,true,true> left with
    GA_CAP_NODES, these bit-vector bands of more than 4 096 nodes too, and gives up on them as every pass before it.  What the caller
    gets is the same -- status 10, failed, no alignment -- except `columns`: a failed read carries the column count of the pass that ran
    it last, so with the pass withheld it is that of <256,true,true>."""
    with pc.emul_profile("emul_wide"):
        a, _ = wc.check_limit(lib)
    with pc.emul_profile("emul_wide_sparse"):
        b, _ = wc.check_limit(lib)
    _same(a, b, "wide_cases.LIMIT", columns=False)


def test_ladders_agree_on_the_pinned_capacity_misses(lib, hooks):
    """the 256 variant's own per-row limit: its misses are GA_CAP_HEAP, which the new pass does not take"""
    g, reads, seeds, draws, oras = rc.capacity_batch()
    bw, ramp = rc.CAPACITY_FAN[4], rc.CAPACITY_FAN[5]
    with pc.emul_profile("emul_wide"):
        a, _ = pc.run_both(g.nodes, g.edges, reads, seeds, bw, ramp=ramp, lib_path=lib)
    with pc.emul_profile("emul_wide_sparse"):
        b, _ = pc.run_both(g.nodes, g.edges, reads, seeds, bw, ramp=ramp, lib_path=lib)
    assert hooks.ga_emul_wide_sparse_jobs_taken() == 0
    _same(a, b, "capacity batch")
    assert {d for d, x in zip(draws, b) if x["status"] == 10} == set(rc.CAPACITY_MISSES)
    for d, x, o in zip(draws, b, oras):
        if d not in rc.CAPACITY_MISSES:
            pc.compare_read(x, o, "capacity batch, draw %d" % d)
