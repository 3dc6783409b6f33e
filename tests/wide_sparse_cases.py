"""Cases for the ladder's last pass: bands of 200 000 cells and more with more than 256 nodes -- the sparse method and the backtrace
override with 4 096 band nodes (run_job<4096,true,true>, ga_wide_sparse_kernel).  Shared by tests/test_wide_sparse.py (host emulation,
tests/emul) and tests/test_wide_sparse_gpu.py (the product library).

The graphs are the fans of wide_cases.fan_batch with LONG branches or very many of them: when an alignment nears the stem's end the
projected band holds the stem and every branch -- 300 to 4 000 nodes and more than 200 000 cells, where the reference leaves its bit
vectors.  What the oracle does with each case is asserted here from its own results (statuses, sparse slices), so that a case
cannot quietly stop being a wide sparse one; every read is then compared with the oracle in every field."""

import parity_common as pc
import wide_cases as wc


# name -> ((branches, branch_len, shared, tail_len, band, ramp, cyclic), the oracle's status per read, its sparse slices per read
# (None: a read the oracle ends in an assertion))
CASES = {
    "300x700": ((300, 700, 16, 64, 10, 0, False), (0, 0, 0), (1, 3, 1)),
    "700x300-tails": ((700, 300, 8, 300, 5, 0, False), (0, 0, 0, 0), (2, 2, 1, 0)),   # the fourth read is seeded in a tail: its backward part meets no such band
    "700x300-ramp": ((700, 300, 8, 64, 3, 8, False), (0, 0, 0), (3, 1, 1)),  # read 0 redoes at width 8
    "300x700-ramp": ((300, 700, 16, 64, 5, 12, False), (0, 1, 0), (1, None, 1)),           # read 1: "diagonal >= here" after a redo over sparse slices
    "cyclic-700x300": ((700, 300, 8, 64, 5, 0, True), (1, 0, 0), (None, 1, 2)),
    "1500x140": ((1500, 140, 8, 64, 4, 0, False), (0, 0, 0), (1, 1, 1)),
    "3000x70": ((3000, 70, 6, 40, 4, 0, False), (0, 0, 0), (1, 1, 1)),
    "4000x52": ((4000, 52, 6, 40, 3, 0, False), (1, 0, 1), (None, 1, None)),                 # 4 001 / 4 002 nodes: next to the limit
}
# 4 208 nodes in read 2's widest sparse slice: more than the tables hold.  Reads 0 and 1 end in an assertion in the oracle, which the
# library may reach (status 1) or not (status 10)
LIMIT = (4200, 50, 6, 40, 3, 0, False)
SMALLEST = ("300x700", "700x300-ramp", "300x700-ramp")
MIN_SPARSE_ALIGNED = 15      # reads across CASES that the oracle aligns over at least one sparse slice


def batch(case):
    branches, branch_len, shared, tail_len, bw, ramp, cyclic = case
    return wc.fan_batch(branches, branch_len, shared, tail_len, cyclic)


def check_oracle(name, oras):
    """the case is what the table above says it is"""
    case, statuses, sparse = CASES[name]
    assert tuple(o["status"] for o in oras) == statuses, (name, [(o["status"], o["message"]) for o in oras])
    for i, o in enumerate(oras):
        if o["status"] == 0:
            assert not o["failed"] and o["sparse_slices"] == sparse[i], (name, i, o["sparse_slices"], o["failed"])
    assert sum(1 for o in oras if o["status"] == 0 and o["sparse_slices"] >= 1) >= 1, name


def check_case(name, lib=None, trace=True, ctx=""):
    """one case against the oracle: every field of every read; a read the oracle ends with status 1 comes back with status 1 (that
    is compare_read's first line), and no read comes back as GA_S_CAPACITY"""
    case = CASES[name][0]
    nodes, edges, reads, seeds = batch(case)
    devs, oras = pc.check_parity(nodes, edges, reads, seeds, case[4], ramp=case[5], lib_path=lib, trace=trace,
                                 ctx="%s %s fan %d x %d bw %d/%d" % (ctx, name, case[0], case[1], case[4], case[5]))
    check_oracle(name, oras)
    assert all(d["status"] != 10 for d in devs), [d["status"] for d in devs]
    assert [d["status"] for d in devs] == [o["status"] for o in oras]
    # the three reads through the fan were finished by a later pass than the first
    assert all(d["kernel_pass"] > 0 for d in devs[:3]), [d["kernel_pass"] for d in devs]
    return devs, oras


def sparse_aligned(oras):
    return sum(1 for o in oras if o["status"] == 0 and not o["failed"] and o["sparse_slices"] >= 1)


def check_limit(lib=None):
    """more nodes in a sparse slice than the widest tables hold: GA_S_CAPACITY for the read the oracle aligns, and nothing worse"""
    nodes, edges, reads, seeds = batch(LIMIT)
    devs, oras = pc.run_both(nodes, edges, reads, seeds, LIMIT[4], ramp=LIMIT[5], lib_path=lib)
    assert oras[2]["status"] == 0 and oras[2]["sparse_slices"] >= 1, (oras[2]["status"], oras[2]["sparse_slices"])
    assert devs[2]["status"] == 10 and devs[2]["failed"], (devs[2]["status"], devs[2]["failed"])
    for d, o in zip(devs[:2], oras[:2]):
        assert o["status"] == 1, o["status"]
        assert d["status"] in (1, 10), d["status"]
    return devs, oras
