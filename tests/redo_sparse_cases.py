"""Fixed reads whose -B ramp redo lands on a sparse-method slice or meets a backtrace-override window (events: redo_events.py).
The descriptions below were found on the CPU by tools/find_redo_events.py with the oracle alone; nothing here searches.  A read is
described by its fan graph, an rng seed, a draw index, its length and its error rate, and is rebuilt from those."""
import functools

import numpy as np

from graphaligner_amd import synth
import oracle_binding as ob
import redo_events as ev

# (branches, branch length, shared prefix, stem length, bandwidth, ramp bandwidth): synth.FanGraph(head_len=200, stem_len=stem,
# n_branches=b, branch_len=bl, shared=sh, seed=b)
FANS = [(8, 30000, 150, 600, 35, 60), (12, 20000, 300, 400, 15, 40), (16, 15000, 200, 500, 20, 45), (6, 40000, 250, 500, 20, 64), (12, 20000, 200, 500, 20, 45)]
LENGTHS = [1300 + 64 * m for m in range(8)]
ERRORS = [0.11, 0.13, 0.15, 0.17]


@functools.lru_cache(maxsize=None)
def fan_graph(fan):
    b, bl, sh, stem, bw, ramp = fan
    return synth.FanGraph(head_len=200, stem_len=stem, n_branches=b, branch_len=bl, shared=sh, seed=b)


def draw_shape(draw):
    """the length and error rate the search gives draw number `draw`"""
    return LENGTHS[draw % len(LENGTHS)], ERRORS[(draw // len(LENGTHS)) % len(ERRORS)]


def build_read(fan, seed, draw, length, err):
    """(read, seed position) of one description: the generator is seeded with (seed, draw), picks the branch and then the errors"""
    g = fan_graph(fan)
    rng = np.random.default_rng([seed, draw])
    branch = int(rng.integers(0, fan[0]))
    return g.read_through(branch, 0, length, rng, sub=err, ins=err, dele=err)


# ---- the chosen descriptions: (index into FANS, rng seed, draw, length, error rate, events the oracle's records must show) ----
# From `tools/find_redo_events.py --draws 400` and `--first 400 --draws 2000` (seed 1: 12 000 reads, 17 145 redos, 1 338 of them
# landing on a sparse slice).  W3 was not seen in them, nor in 2 000 reads each at error rates 0.21 and 0.25 (--err): DESIGN.md
# section 5 lists it as not pinned.
CASES = [
    (0, 1, 25, 1364, 0.17, ('CK', 'U1', 'W1')),   # asserts: i <= 1 || table.slices[i].j > table.slic, 1295 bp, 2 redos
    (0, 1, 44, 1556, 0.13, ('L1', 'L1b', 'U1')),   # aligns, 1562 bp, 4 redos
    (0, 1, 55, 1748, 0.15, ('U1', 'W1')),   # aligns, 1688 bp, 4 redos
    (0, 1, 60, 1556, 0.17, ('L1', 'L1b')),   # fails, 1652 bp, 6 redos
    (0, 1, 169, 1364, 0.13, ('L1', 'L1b', 'U1', 'W1')),   # aligns, 1326 bp, 1 redos
    (0, 1, 211, 1492, 0.15, ('CK', 'U1', 'W1')),   # asserts: i <= 1 || table.slices[i].j > table.slic, 1678 bp, 4 redos
    (0, 1, 503, 1748, 0.15, ('W2',)),   # asserts: i <= 1 || table.slices[i].j > table.slic, 1684 bp, 1 redos
    (0, 1, 695, 1748, 0.15, ('CK', 'U1')),   # aligns, 1742 bp, 1 redos
    (1, 1, 41, 1364, 0.13, ('L1', 'L1b', 'U1')),   # aligns, 1314 bp, 1 redos
    (1, 1, 114, 1428, 0.15, ('U1', 'W2')),   # aligns, 1394 bp, 3 redos
    (1, 1, 313, 1364, 0.17, ('L1', 'L1b', 'U1', 'W1')),   # asserts: overrideLastJ > startSlice * W @1689, 1349 bp, 4 redos
    (1, 1, 852, 1556, 0.15, ('L2', 'U1')),   # fails, 1543 bp, 2 redos
    (1, 1, 2202, 1428, 0.17, ('L1', 'L1b', 'L2', 'U1')),   # aligns, 1335 bp, 6 redos
    (2, 1, 2, 1428, 0.11, ('L1', 'L1b', 'U1')),   # aligns, 1440 bp, 1 redos
    (2, 1, 12, 1556, 0.13, ('L1', 'L1b', 'U1')),   # aligns, 1439 bp, 1 redos
    (2, 1, 28, 1556, 0.17, ('L1', 'L1b', 'U1')),   # asserts: diagonal >= here @802, 1538 bp, 3 redos
    (2, 1, 52, 1556, 0.15, ('CK', 'U1', 'W1')),   # asserts: i <= 1 || table.slices[i].j > table.slic, 1523 bp, 1 redos
    (2, 1, 84, 1556, 0.15, ('U1', 'W1')),   # aligns, 1659 bp, 4 redos
    (2, 1, 212, 1556, 0.15, ('CK', 'U1', 'W1')),   # fails, 1561 bp, 7 redos
    (2, 1, 281, 1364, 0.17, ('U1', 'W2')),   # fails, 1301 bp, 1 redos
    (3, 1, 2, 1428, 0.11, ('L1', 'L1b', 'U1')),   # aligns, 1440 bp, 1 redos
    (3, 1, 20, 1556, 0.15, ('L1', 'L1b', 'U1')),   # asserts: diagonal >= here @802, 1561 bp, 4 redos
    (3, 1, 25, 1364, 0.17, ('U1', 'W1')),   # fails, 1295 bp, 4 redos
    (3, 1, 83, 1492, 0.15, ('U1', 'W2')),   # aligns, 1525 bp, 3 redos
    (3, 1, 642, 1428, 0.11, ('CK', 'U1', 'W1')),   # aligns, 1564 bp, 1 redos
    (3, 1, 756, 1556, 0.15, ('L2', 'U1')),   # aligns, 1557 bp, 2 redos
    (4, 1, 2, 1428, 0.11, ('L1', 'L1b', 'U1')),   # aligns, 1440 bp, 1 redos
    (4, 1, 25, 1364, 0.17, ('U1', 'W2')),   # aligns, 1295 bp, 1 redos
    (4, 1, 31, 1748, 0.17, ('L1', 'L1b')),   # fails, 1742 bp, 5 redos
    (4, 1, 49, 1364, 0.15, ('U1', 'W1')),   # aligns, 1399 bp, 1 redos
    (4, 1, 1384, 1300, 0.13, ('L2', 'U1')),   # asserts: i <= 1 || table.slices[i].j > table.slic, 1371 bp, 2 redos
    # the reads that decided loadRecordState's scoreEndExists bits: with every column of a sparse landing slice
    # taken as existing, the device program counted 400 columns more than the oracle on the first and ended the others in an assertion
    (1, 1, 1174, 1684, 0.15, ('L1', 'L1b', 'U1')),   # aligns, 1647 bp
    (3, 1, 600, 1300, 0.17, ('L1', 'L1b')),   # fails, 1341 bp, two sparse landings
    (3, 1, 697, 1364, 0.17, ('L1', 'L1b')),   # fails, 1336 bp
    (3, 1, 760, 1300, 0.17, ('L1', 'L1b', 'U1', 'W1')),   # fails, 1342 bp, two sparse landings
    (3, 1, 1321, 1364, 0.13, ('L1', 'L1b')),   # fails, 1488 bp
]
PINNED = ("L1", "L1b", "L2", "W1", "W2", "U1", "CK")
MAX_READ = 1800
W = 64


@functools.lru_cache(maxsize=None)
def batches():
    """[(fan, graph, reads, seeds, descriptions, oracle results, classifications)], one batch per fan, built once per process and left
    unchanged.  Each batch is listed longest read first: the order in which one wave takes the jobs when it takes them all
    (GA_TEST_WAVE_SLOTS=1, GA_EMUL_REUSE=1).  The oracle ran with record=True; its slice records are classified and dropped (they are
    hundreds of megabytes)."""
    out = []
    for k, fan in enumerate(FANS):
        g = fan_graph(fan)
        og = ob.OracleGraph(g.nodes, g.edges)
        rows = []
        for d in (c for c in CASES if c[0] == k):
            r, s = build_read(fan, *d[1:5])
            o = og.align(r, [s], fan[4], fan[5], record=True)
            c = ev.classify(o.pop("slice_records"), fan[5], {0: (len(r) + W - 1) // W})
            rows.append((r, s, d, o, c))
        rows.sort(key=lambda x: -len(x[0]))
        if rows:
            out.append((fan, g) + tuple([x[i] for x in rows] for i in range(5)))
    return out


def aligned(o):
    return o["status"] == 0 and not o["failed"]


def check_conditions():
    """what the list has to show on the oracle alone, asserted before anything is compared with it -> {event: reads}"""
    bs = batches()
    rows = [(d, o, c, r) for _, _, reads, _, descs, oras, classes in bs for d, o, c, r in zip(descs, oras, classes, reads)]
    for d, o, c, r in rows:
        assert len(r) <= MAX_READ, (d, len(r))
        assert set(d[5]) <= c["events"], ("the oracle's records do not show", d, sorted(c["events"]))
    count = lambda e, pred=lambda o: True: sum(1 for d, o, c, _ in rows if e in c["events"] and pred(o))
    assert count("L1") >= 8 and count("L1", aligned) >= 4, (count("L1"), count("L1", aligned))
    assert count("L1b") >= 3, count("L1b")
    for e in PINNED:
        assert count(e) >= 1, e
    assert len(rows) >= 24 and len(bs) >= 3, (len(rows), len(bs))
    # on one wave (longest first) a read that fails or asserts comes before an L1 read that aligns
    n_after = 0
    for _, _, reads, _, _, oras, classes in bs:
        bad = [len(r) for r, o in zip(reads, oras) if not aligned(o)]
        n_after += sum(1 for r, o, c in zip(reads, oras, classes) if bad and aligned(o) and "L1" in c["events"] and len(r) < max(bad))
    assert n_after >= 4, n_after
    return {e: count(e) for e in ev.EVENTS}


# what ONE wave is given on the GPU (GA_TEST_WAVE_SLOTS=1; a sparse-method job keeps a wave busy for seconds, so a handful): per fan,
# draws in the order the wave takes them -- a read that ends in an assertion or without an alignment, then L1 reads
ONE_WAVE = {1: (313, 2202, 41), 3: (20, 1321, 2), 4: (31, 2, 1384)}


def one_wave_batch(fan_index):
    """the reads of ONE_WAVE[fan_index] out of that fan's batch, in the batch's order (longest first), as batches() gives them"""
    fan, g, reads, seeds, descs, oras, classes = [b for b in batches() if b[0] == FANS[fan_index]][0]
    keep = [i for i, d in enumerate(descs) if d[2] in ONE_WAVE[fan_index]]
    assert [descs[i][2] for i in keep] == list(ONE_WAVE[fan_index]), [descs[i][2] for i in keep]
    first = keep[0]
    assert not aligned(oras[first]) and any(aligned(oras[i]) and "L1" in classes[i]["events"] for i in keep[1:])
    return (fan, g) + tuple([x[i] for i in keep] for x in (reads, seeds, descs, oras, classes))


def check_sparse_reads_climbed(devs, oras):
    """no read whose oracle run shows a sparse slice was finished by the first pass"""
    assert all(d["kernel_pass"] > 0 for d, o in zip(devs, oras) if o["sparse_slices"] > 0), [d["kernel_pass"] for d in devs]


def sparse_parts(oras):
    """the parts (jobs) of a batch whose oracle run shows a sparse-method slice; every read here has one part (seed at its first base)"""
    return sum(1 for o in oras if o["sparse_slices"] > 0)


# ---- a loud capacity miss: 40 branches at bandwidth 35 / 70, reads at error rate 0.15 ---------------------------------------------
# With 40 branches in the band and the ramp width of 70, one row of a sparse-method slice can hold more than 8 192 cells within
# the bandwidth of its minimum: more than the row set of ga_sparse.h takes (kSetSize / 2), which answers GA_CAP_HEAP, and the read
# comes back as GA_S_CAPACITY (include/graphaligner_amd.h) where the oracle goes on.  Status 10 is
# allowed for the draws named here and for no other read.
CAPACITY_FAN = (40, 6000, 250, 400, 35, 70)
CAPACITY_DRAWS = [2, 4, 8, 20, 30]
CAPACITY_ERR = 0.15
CAPACITY_MISSES = {20: "the oracle aligns the read", 30: "the oracle ends in an assertion (status 1)"}


@functools.lru_cache(maxsize=None)
def capacity_batch():
    """(graph, reads, seeds, draws, oracle results), longest first"""
    g = fan_graph(CAPACITY_FAN)
    og = ob.OracleGraph(g.nodes, g.edges)
    rows = []
    for d in CAPACITY_DRAWS:
        r, s = build_read(CAPACITY_FAN, 1, d, draw_shape(d)[0], CAPACITY_ERR)
        rows.append((r, s, d, og.align(r, [s], CAPACITY_FAN[4], CAPACITY_FAN[5])))
    rows.sort(key=lambda x: -len(x[0]))
    return (g,) + tuple([x[i] for x in rows] for i in range(4))
