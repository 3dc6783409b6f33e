"""The ladder's policy (graphaligner_amd/csrc/ga_ladder.h) on its own: gald::climb, the function both the device back end and the host
emulation call, over a scripted back end (tests/emul/ga_emul_hooks.cpp: ga_emul_ladder_climb).  The script says which status a job has
after a variant ran it; what comes back is the job list each launched pass was given, which pass touched each job last, and the retried
count.  No kernel runs: milliseconds."""
import ctypes as C

import numpy as np
import pytest

import parity_common as pc

# gald::Variant, in its order
VARIANTS = ("<10,64>", "<24,32>", "<56,16>", "<32,false>", "<64,false>", "<64,true>", "<256,true>", "<4096,true>", "<256,true,true>", "<4096,true,true>")
V = {name: i for i, name in enumerate(VARIANTS)}
# job statuses (graphaligner_amd/csrc/ga_types.h)
OK, ASSERTION, BAND, BAD_SEED = 0, 1, 2, 3
CAP_NODES, CAP_COLS, CAP_ARENA, CAP_TRACE, CAP_HEAP = 10, 11, 12, 13, 14
CYCLE, RAMP, PUNT, NOT_RUN = 20, 21, 22, 99


@pytest.fixture(scope="module")
def hooks():
    L = C.CDLL(pc.emul_lib_path())
    L.ga_emul_ladder_climb.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ga_emul_ladder_climb.restype = C.c_int
    L.ga_emul_ladder_first_pass.argtypes = [C.c_double, C.c_int, C.c_void_p]
    return L


def first_pass(hooks, mean_node_length, forced):
    """the product's first-pass struct for a graph: (lanes first, starting lanes size, minJobsLater)"""
    out = np.zeros(3, dtype=np.int32)
    hooks.ga_emul_ladder_first_pass(float(mean_node_length), forced, out.ctypes.data)
    return bool(out[0]), VARIANTS[out[1]], int(out[2])


def climb(hooks, n, fp, after):
    """after: {variant name: status or per-job list of statuses}; a variant not named finishes every job it gets (GA_OK).
    Returns ([(variant, first, [jobs])] per launch, passOf, retried)"""
    table = np.zeros((len(VARIANTS), n), dtype=np.int32)
    for name, st in after.items():
        table[V[name], :] = st
    launches = np.zeros(3 * len(VARIANTS), dtype=np.int32)
    lists = np.zeros(len(VARIANTS) * n, dtype=np.uint32)
    pass_of = np.zeros(n, dtype=np.uint8)
    retried = C.c_uint64(12345)
    k = hooks.ga_emul_ladder_climb(n, int(fp[0]), V[fp[1]], fp[2], table.ctypes.data, launches.ctypes.data, lists.ctypes.data, pass_of.ctypes.data, C.byref(retried))
    assert 0 <= k <= len(VARIANTS)
    out, at = [], 0
    for i in range(k):
        v, first, size = (int(x) for x in launches[3 * i:3 * i + 3])
        out.append((VARIANTS[v], bool(first), [int(j) for j in lists[at:at + size]]))
        at += size
    return out, [int(p) for p in pass_of], retried.value


def everywhere(status):
    return {name: status for name in VARIANTS}


AFTER_LANES = {
    CAP_NODES: ["<64,false>", "<256,true>", "<4096,true>", "<256,true,true>", "<4096,true,true>"],
    CAP_HEAP: ["<64,false>", "<256,true>", "<4096,true>", "<256,true,true>"],
    CAP_COLS: ["<64,false>", "<256,true>", "<256,true,true>"],
    CAP_ARENA: ["<64,false>", "<256,true>", "<256,true,true>"],
    CAP_TRACE: ["<64,false>", "<256,true>", "<256,true,true>"],
    PUNT: ["<64,false>", "<256,true>", "<256,true,true>"],
    CYCLE: ["<64,true>", "<256,true>", "<256,true,true>"],
    RAMP: ["<64,true>", "<256,true>", "<256,true,true>"],
    BAND: ["<256,true,true>"],
    OK: [],
    ASSERTION: [],
    BAD_SEED: [],
}


@pytest.mark.parametrize("status", sorted(AFTER_LANES))
def test_rungs_by_status_lanes_first(hooks, status):
    """one job, lanes first with the product's thresholds, and a status that every variant returns again"""
    fp = first_pass(hooks, 64.0, -1)
    assert fp == (True, "<10,64>", 512)
    launches, pass_of, retried = climb(hooks, 1, fp, everywhere(status))
    assert launches[0] == ("<10,64>", True, [0])
    assert [v for v, first, jobs in launches[1:]] == AFTER_LANES[status]
    assert all(not first and jobs == [0] for v, first, jobs in launches[1:])
    # passOf counts launched passes only; the lanes pass is not a retry
    assert pass_of == [len(launches) - 1] and retried == len(launches) - 1


@pytest.mark.parametrize("status", sorted(AFTER_LANES))
def test_rungs_by_status_wave_per_read_first(hooks, status):
    """<32,false> gets all jobs, then the same rungs; the retried count restarts behind it"""
    fp = first_pass(hooks, 64.0, 0)
    assert not fp[0]
    launches, pass_of, retried = climb(hooks, 3, fp, everywhere(status))
    assert launches[0] == ("<32,false>", True, [0, 1, 2])
    assert [v for v, first, jobs in launches[1:]] == AFTER_LANES[status]
    assert all(not first and jobs == [0, 1, 2] for v, first, jobs in launches[1:])
    assert pass_of == [len(launches) - 1] * 3 and retried == 3 * (len(launches) - 1)


def test_later_lanes_sizes_need_enough_jobs(hooks):
    fp = first_pass(hooks, 64.0, 1)
    leave10 = [CAP_NODES] * 520 + [OK] * 80
    leave24 = [CAP_NODES if j < 100 else OK for j in range(600)]
    launches, pass_of, retried = climb(hooks, 600, fp, {"<10,64>": leave10, "<24,32>": leave24})
    assert [(v, first, len(jobs)) for v, first, jobs in launches] == [("<10,64>", True, 600), ("<24,32>", False, 520), ("<64,false>", False, 100)]
    assert launches[1][2] == list(range(520)) and launches[2][2] == list(range(100))
    assert pass_of == [2] * 100 + [1] * 420 + [0] * 80 and retried == 100
    # one job fewer than the threshold: no <24,32>, the stragglers take the wave-per-read rungs
    launches, pass_of, retried = climb(hooks, 600, fp, {"<10,64>": [CAP_NODES] * 511 + [OK] * 89})
    assert [(v, len(jobs)) for v, first, jobs in launches] == [("<10,64>", 600), ("<64,false>", 511)]
    assert pass_of == [1] * 511 + [0] * 89 and retried == 511
    # all three sizes, each for what the size before could not hold; what a size declines waits for the wave-per-read rungs
    leave10 = [CAP_COLS] * 600 + [PUNT] * 50
    leave24 = [CAP_ARENA] * 550 + [OK] * 100
    launches, pass_of, retried = climb(hooks, 650, fp, {"<10,64>": leave10, "<24,32>": leave24})
    assert [(v, len(jobs)) for v, first, jobs in launches] == [("<10,64>", 650), ("<24,32>", 600), ("<56,16>", 550), ("<64,false>", 50)]
    assert launches[3][2] == list(range(600, 650))


@pytest.mark.parametrize("mean,start", [(50, "<10,64>"), (40, "<10,64>"), (20, "<24,32>"), (14, "<24,32>"), (8, "<56,16>")])
def test_starting_lanes_size(hooks, mean, start):
    fp = first_pass(hooks, mean, 1)
    assert fp == (True, start, 512)
    launches, pass_of, retried = climb(hooks, 2, fp, everywhere(CAP_NODES))
    # (two jobs: no later lanes size)
    assert [v for v, first, jobs in launches] == [start] + AFTER_LANES[CAP_NODES]
    # unset, the graph's shape decides which kernel goes first
    assert first_pass(hooks, mean, -1)[0] == (mean >= 40) and not first_pass(hooks, mean, 0)[0]


def test_rungs_select_from_all_jobs_in_hand_out_order(hooks):
    """a wave-per-read rung takes every job whose status it takes, whichever pass left it: here <256,true> gets what <64,false> and
    what <64,true> left, merged in hand-out order, and a pass that is not launched does not count in passOf"""
    fp = first_pass(hooks, 64.0, 1)
    launches, pass_of, retried = climb(hooks, 4, fp, {"<10,64>": [CYCLE, PUNT, OK, CYCLE], "<64,false>": CAP_ARENA, "<64,true>": [RAMP, OK, OK, OK]})
    assert launches == [("<10,64>", True, [0, 1, 2, 3]), ("<64,false>", False, [1]), ("<64,true>", False, [0, 3]), ("<256,true>", False, [0, 1])]
    assert pass_of == [3, 3, 0, 2] and retried == 5
    assert climb(hooks, 0, fp, {}) == ([], [], 0)
