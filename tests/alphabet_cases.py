"""The probe sets that pin the read alphabet, shared by test_alphabet.py (host emulation) and test_alphabet_gpu.py (product).

A probe is an error-free read over a linear graph with ONE byte replaced.  alphabet_model.expected gives its status and score from
the reference's text; the oracle gives every field for the probes that can reach it (a read with byte 0 cannot: the oracle takes a
C string, so those probes are checked against the model alone).

Where a read position lands, from GaEqFill (ga_backend.h) and ga_batch_prepare: a seed at read position s of a read of n bases
makes a backward job of s rows when s > 0 -- row k is the complement of seq[s - 1 - k], so read position p is row s - 1 - p and
read position 0 is the part's LAST real row -- and a forward job of n - s rows when s < n - 1 -- row k is seq[s + k], so the seed's
own base is forward row 0 and the read's last base the part's last real row.  Rows n .. padded - 1 of a job are the pad code.  With
the seed on the last base that base is in no job at all.

Every read's seed base lies on the same graph base, three bases into its node on both graphs: the first rows of both parts have
their diagonal predecessor inside the seed node, where the initial slice is 0.
"""
import functools

import numpy as np

from graphaligner_amd import binding, synth
import alphabet_model as am
import oracle_binding as ob
import parity_common as pc

BW = 35
GRAPH_BP = 4000
ANCHOR = 24 * 64 + 3            # the graph base under every seed: offset 3 of a 64-bp node and of an 8-bp node
GRAPHS = {"64bp-nodes": (64, 91), "8bp-nodes": (8, 92)}

LETTERS = "ACGTNURYKMSWBVDH"
EDGE_BYTES = tuple(ord(c) for c in LETTERS + LETTERS.lower()) + (0, 1, ord("-"), ord("*"), ord(" "), ord("X"), 127, 128, 200, 255)
assert len(EDGE_BYTES) == 42 and len(set(EDGE_BYTES)) == 42

MAIN_READ = (600, 300)          # (bases, seed position): parts of 300 rows, 20 padding rows each
MID_ROW = 100
EDGE_ROWS = (0, 1, 62, 63, 64, 127)
# (backward rows, forward rows): no padding row (256, 320), one (255, 319), 63 (193, 257, 321), each length in both directions
PART_LENGTHS = ((193, 321), (255, 320), (256, 319), (257, 257), (319, 256), (320, 255), (321, 193))
ONE_PART_READS = ((400, 0), (400, 399))     # seed on the first base (no backward part) and on the last (no forward part)
BIG_READ = (400, 200)


@functools.lru_cache(maxsize=None)
def graph(name):
    node_len, seed = GRAPHS[name]
    return synth.linear_graph(GRAPH_BP, node_len=node_len, seed=seed)


def path_of(g, n, s):
    """the graph bases under a read of n bases whose position s lies on ANCHOR"""
    a = ANCHOR - s
    assert a >= 0 and a + n <= len(g.genome)
    return bytes(g.genome[a:a + n].tobytes())


def seed_of(g, s):
    return (int(g.node_at[ANCHOR]), s, False)


def position_of(n, s, part, row):
    """the read position that is row `row` of the backward / forward part"""
    p = s - 1 - row if part == "backward" else s + row
    assert am.part_of(n, s, p) == (part, row), (n, s, part, row)
    return p


def _rows_probes(n, s, rows_bw, rows_fw, byte_values):
    out = []
    for part, rows in (("backward", rows_bw), ("forward", rows_fw)):
        for row in rows:
            p = position_of(n, s, part, row)
            out += [(n, s, p, b) for b in byte_values]
    return out


def main_probes():
    """every byte value once per direction at a mid-slice row; the edge bytes at every edge row of both parts"""
    n, s = MAIN_READ
    bw_rows, fw_rows = am.part_lengths(n, s)
    probes = _rows_probes(n, s, (MID_ROW,), (MID_ROW,), range(256))
    probes += _rows_probes(n, s, EDGE_ROWS + (bw_rows - 2, bw_rows - 1), EDGE_ROWS + (fw_rows - 2, fw_rows - 1), EDGE_BYTES)
    return probes


def length_probes():
    """the edge bytes on the last real row of parts of every length in PART_LENGTHS, and on the rows of reads with one part"""
    probes = []
    for bw_rows, fw_rows in PART_LENGTHS:
        n, s = bw_rows + fw_rows, bw_rows
        assert am.part_lengths(n, s) == (bw_rows, fw_rows)
        probes += _rows_probes(n, s, (bw_rows - 1,), (fw_rows - 1,), EDGE_BYTES)
    n, s = ONE_PART_READS[0]
    probes += _rows_probes(n, s, (), (0, n - 1), EDGE_BYTES)
    n, s = ONE_PART_READS[1]
    probes += _rows_probes(n, s, (0, s - 1), (), EDGE_BYTES)
    probes += [(n, s, n - 1, b) for b in EDGE_BYTES]        # the base no part holds
    return probes


def all_probes():
    return main_probes() + length_probes()


def big_probes():
    """the probe list the large batch cycles through: BIG_READ with every byte value mid-slice and the edge bytes on the edge rows.
    A byte that ReverseComplement refuses ends the read before any job is made (ga_batch_prepare), so a read with such a byte in
    its backward part adds no fill; the backward probes here are the 30 bytes it accepts ('U' and 'u' among them, which end in the
    assertion only along the trace), so that every read of the batch has its two fills"""
    n, s = BIG_READ
    turned = [b for b in range(256) if am.backward_char(b) is not None]
    probes = _rows_probes(n, s, (MID_ROW,), (), turned) + _rows_probes(n, s, (), (MID_ROW,), range(256))
    probes += _rows_probes(n, s, (0, 63, 64, s - 1), (), [b for b in EDGE_BYTES if b in turned])
    probes += _rows_probes(n, s, (), (0, 63, 64, n - s - 1), EDGE_BYTES)
    return probes


def forward_only_probes():
    """probes of the read seeded on its first base whose byte the model accepts: the shape that qualifies for node runs"""
    n, s = ONE_PART_READS[0]
    probes = _rows_probes(n, s, (), (0, 1, 63, 64, MID_ROW, n - 1), EDGE_BYTES)
    return [p for p in probes if am.forward_set(p[3]) is not None]


def read_of(g, probe):
    n, s, p, b = probe
    r = bytearray(path_of(g, n, s))
    r[p] = b
    return bytes(r)


def model_of(g, probe):
    n, s, p, b = probe
    return am.expected(path_of(g, n, s), s, p, b)


def reaches_oracle(probe):
    return probe[3] != 0


def describe(probe):
    n, s, p, b = probe
    part, row = am.part_of(n, s, p)
    return "byte %d (%r) at read position %d = %s row %s of a %d-base read seeded at %d" % (b, chr(b), p, part, row, n, s)


_ORACLE = {}
_ORACLE_GRAPHS = {}


def oracle_of(name, probe):
    """the oracle's result for a probe, computed once per process and left unchanged; None for a probe that cannot reach it"""
    if not reaches_oracle(probe):
        return None
    key = (name, probe)
    if key not in _ORACLE:
        g = graph(name)
        if name not in _ORACLE_GRAPHS:
            _ORACLE_GRAPHS[name] = ob.OracleGraph(g.nodes, g.edges)
        _ORACLE[key] = _ORACLE_GRAPHS[name].align(read_of(g, probe), [seed_of(g, probe[1])], BW)
    return _ORACLE[key]


def check_model_result(res, want, ctx):
    """res: a result dict of the product's binding or of the oracle's (the status numbers 0 and 1 are the same in both)"""
    status, score = want
    assert res["status"] == status, (ctx, "status", res["status"], "model", status)
    if status == am.GA_S_OK:
        assert not res["failed"], (ctx, "failed")
        assert res["score"] == score, (ctx, "score", res["score"], "model", score)


def check_model_against_oracle(name, probes):
    n = 0
    for probe in probes:
        ora = oracle_of(name, probe)
        if ora is not None:
            check_model_result(ora, model_of(graph(name), probe), "oracle, %s: %s" % (name, describe(probe)))
            n += 1
    return n


def run_probes(name, probes, trace, lib_path=None):
    """one batch of the probes' reads through the library -> (results, batch statistics)"""
    g = graph(name)
    gg = binding.Graph(g.nodes, g.edges, lib_path=lib_path)
    b = gg.prepare([read_of(g, p) for p in probes], [[seed_of(g, p[1])] for p in probes], BW, 0, binding.GA_F_TRACE if trace else 0)
    b.run()
    stats = b.stats()
    devs = b.collect()
    assert len(devs) == len(probes)
    return devs, stats


def check_probes(name, probes, devs, trace, oracle_every=1):
    """every result against the model; against the oracle, field by field, every `oracle_every`-th probe that can reach it"""
    g = graph(name)
    k = 0
    for probe, d in zip(probes, devs):
        ctx = "%s, %s: %s" % (name, "trace items" if trace else "flags 0", describe(probe))
        check_model_result(d, model_of(g, probe), ctx)
        if not trace:
            assert d["trace"].shape[0] == 0, ctx
        if reaches_oracle(probe):
            if k % oracle_every == 0:
                pc.compare_read(d, pc.expected(oracle_of(name, probe), trace), ctx)
            k += 1


def case_probes(name, probes, trace, lib_path=None):
    devs, _ = run_probes(name, probes, trace, lib_path)
    check_probes(name, probes, devs, trace)
    return devs


def case_node_runs_see_the_alphabet(lib_path=None):
    """valid forward-only probes on the 64-bp graph with flags = 0: the batch hands back node runs (ga_batch_stats.reserved == 1, as
    case_results_without_trace_items asserts it); one invalid probe more switches the whole batch to moves and changes no other
    read's result"""
    name = "64bp-nodes"
    probes = forward_only_probes()
    assert len(probes) >= 150 and all(model_of(graph(name), p)[0] == am.GA_S_OK for p in probes)
    devs, stats = run_probes(name, probes, False, lib_path)
    assert stats["reserved"] == 1, stats
    check_probes(name, probes, devs, False)
    n, s = ONE_PART_READS[0]
    bad = (n, s, position_of(n, s, "forward", MID_ROW), ord("u"))
    assert model_of(graph(name), bad)[0] == am.GA_S_ASSERTION
    devs2, stats2 = run_probes(name, probes + [bad], False, lib_path)
    assert stats2["reserved"] == 0, stats2
    check_probes(name, probes + [bad], devs2, False)
    for i, (x, y) in enumerate(zip(devs, devs2)):
        for field in ("status", "failed", "score", "query_position", "alignment_start", "alignment_end", "mappings", "columns"):
            assert x[field] == y[field], ("an invalid read changed another read's result", describe(probes[i]), field)


def case_more_fills_than_blocks(cus, lib_path=None, name="64bp-nodes"):
    """cus * 32 + 200 reads with mid seeds, two fills each: more fills than the cus * 64 blocks the match-word kernel is launched
    with, so its grid-stride loop goes round.  Every read against the model, every 16th that can reach the oracle against it"""
    cycle = big_probes()
    n_reads = cus * 32 + 200
    probes = [cycle[i % len(cycle)] for i in range(n_reads)]
    devs, stats = run_probes(name, probes, False, lib_path)
    assert stats["n_jobs"] > cus * 64, (stats["n_jobs"], cus)
    check_probes(name, probes, devs, False, oracle_every=16)
    return stats


# ---- the sparse variant reads the row codes by itself (ga_sparse.h) ---------------------------------------------------------------
FAN = (8, 30000, 150, 600, 35, 0)       # parity_cases.SPARSE_FANS[0]
_FAN_CODES = "NRYKMSWBDVnrykmswbdvacgt"       # (no H: it would end every read with a backward part in the assertion)


@functools.lru_cache(maxsize=None)
def fan_batch():
    """eight reads on case_sparse_method_and_override's first fan with ambiguity codes and lower case inside the branches (read
    positions past head, stem and the branches' common beginning): three of that case's reads from the stem on and two of its reads
    seeded inside a branch, two more reads from the stem on, and one of them once more with an invalid byte there"""
    import parity_cases as cases
    branches, branch_len, shared, stem, bw, ramp = FAN
    g = synth.FanGraph(head_len=200, stem_len=stem, n_branches=branches, branch_len=branch_len, shared=shared, seed=branches)
    reads, seeds = cases._fan_reads(g, branches, bw)
    reads, seeds = [reads[k] for k in (0, 2, 3, 4, 5)], [seeds[k] for k in (0, 2, 3, 4, 5)]
    rng = np.random.default_rng(17)
    for k in range(2):
        r, s = g.read_through(int(rng.integers(0, branches)), 0, 1600 + 500 * k, rng)
        reads.append(r); seeds.append(s)
    first = 200 + stem + shared + 60
    out = []
    for r in reads:
        b = bytearray(r.encode())
        assert len(b) > first + 300
        for p in rng.choice(np.arange(first, len(b)), size=16, replace=False):
            b[int(p)] = ord(_FAN_CODES[int(rng.integers(len(_FAN_CODES)))])
        out.append(bytes(b))
    b = bytearray(out[0])
    b[first + 100] = ord("H")       # (a read from the stem on has no backward part: 'H' is an ordinary code there)
    out[0] = bytes(b)
    b = bytearray(out[2])
    b[first + 200] = ord("X")
    out.append(bytes(b))
    seeds = seeds + [seeds[2]]
    oras = pc.oracle_results(g.nodes, g.edges, out, seeds, bw, ramp)
    return g, out, seeds, oras


def case_sparse_variant_sees_the_alphabet(trace, lib_path=None):
    """fan_batch's reads against the oracle alone (no model of a fan); no part whose oracle run shows a sparse slice was finished by the
    first pass.  -> (results, oracle results, the number of such parts that align)"""
    g, reads, seeds, oras = fan_batch()
    bw, ramp = FAN[4], FAN[5]
    assert sum(1 for o in oras if o["status"] == 0 and not o["failed"]) >= 4 and any(o["status"] == 1 for o in oras)
    need = sum(1 for o in oras if o["sparse_slices"] > 0 and o["status"] == 0)
    assert need >= 4, need
    gg = binding.Graph(g.nodes, g.edges, lib_path=lib_path)
    b = gg.prepare(reads, [[s] for s in seeds], bw, ramp, binding.GA_F_TRACE if trace else 0)
    b.run()
    devs = b.collect()
    for i, (d, o) in enumerate(zip(devs, oras)):
        pc.compare_read(d, pc.expected(o, trace), "fan read %d with ambiguity codes" % i)
    assert all(d["kernel_pass"] > 0 for d, o in zip(devs, oras) if o["sparse_slices"] > 0 and o["status"] == 0), [d["kernel_pass"] for d in devs]
    return devs, oras, need
