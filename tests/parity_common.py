"""shared helpers for the parity tests: run the same reads through the C ABI (real GPU library
or the host emulation of the device program) and through the CPU oracle, then compare every
field the reference's AlignmentResult carries."""
import contextlib
import os
import subprocess

import numpy as np

from graphaligner_amd import binding, synth
import oracle_binding as ob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL_SO = os.path.join(ROOT, "tests", "_build", "libga_emul.so")

# oracle status -> ABI status
_STATUS_MAP = {0: 0, 1: 1, 2: 2, 3: 3}


def emul_lib_path():
    """the one host emulation (tests/emul): with nothing set it does what the product's back end does"""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emul")])
    return EMUL_SO


# GA_EMUL_WITHOUT (tests/emul/ga_emul.h) for the capability sets that the tests name: what the back ends of earlier stages of the
# project lacked.  A graph uploaded under a profile answers with the interface's defaults for what it withholds, which is what the
# tests of the host code's refusals, of the host-built tables and of one ladder against another need.
PROFILES = {
    "emul": "wide,wide_sparse,words,ops,seeding",                # the ladder up to <256,true,true>, words from the host, no seeding
    "emul_wide": "wide_sparse,words,ops,seeding",                # ... with <4096,true>
    "emul_wide_sparse": "words,ops,seeding",                     # ... and <4096,true,true>
    "emul_seed": "walks,loci,topology,seeded",                   # build and find only
    "emul_seed_walks": "loci,topology,seeded",                   # ... with buildWalks
    "emul_seed_loci": "topology,seeded",                         # ... and findLoci
    "emul_seed_coord": "seeded",                                 # ... and setCoordinate: everything but seeded batches (the two-call path)
    "emul_seed_plan": "words,ops",                               # seeded batches over words from the host, no GA_F_OPS
    "emul_ops": "seeding",                                       # GA_F_OPS over the back end's own words, no seeding
}


@contextlib.contextmanager
def emul_profile(name):
    """graphs uploaded inside the block withhold what PROFILES[name] lists (the switch is read at every upload)"""
    before = os.environ.get("GA_EMUL_WITHOUT")
    os.environ["GA_EMUL_WITHOUT"] = PROFILES[name]
    try:
        yield
    finally:
        if before is None:
            del os.environ["GA_EMUL_WITHOUT"]
        else:
            os.environ["GA_EMUL_WITHOUT"] = before


def compare_read(dev, ora, ctx=""):
    """dev: dict from graphaligner_amd.binding; ora: dict from oracle_binding"""
    assert dev["status"] == _STATUS_MAP[ora["status"]], (ctx, "status", dev["status"], ora["status"], ora["message"])
    assert dev["failed"] == ora["failed"], (ctx, "failed")
    if ora["status"] != 0 or ora["failed"]:
        return
    assert dev["score"] == ora["score"], (ctx, "score", dev["score"], ora["score"])
    assert dev["query_position"] == ora["query_position"], (ctx, "query_position")
    assert dev["alignment_start"] == ora["alignment_start"], (ctx, "alignment_start")
    assert dev["alignment_end"] == ora["alignment_end"], (ctx, "alignment_end")
    assert len(dev["mappings"]) == len(ora["mappings"]), (ctx, "n mappings", len(dev["mappings"]), len(ora["mappings"]))
    for i, (a, b) in enumerate(zip(dev["mappings"], ora["mappings"])):
        assert tuple(a) == tuple(b), (ctx, "mapping", i, a, b)
    if dev["trace"].shape[0] or ora["trace"].shape[0]:
        assert dev["trace"].shape == ora["trace"].shape, (ctx, "trace items", dev["trace"].shape, ora["trace"].shape)
        assert (dev["trace"] == ora["trace"]).all(), (ctx, "trace items differ")
    assert dev["columns"] == ora["columns"], (ctx, "column updates", dev["columns"], ora["columns"])


# the oracle's results for a batch, computed once per process and left unchanged (the same case runs under several settings of
# the library: which kernel goes first, how many waves a launch may start, with and without TraceItem lists)
_ORACLE_MEMO = {}


def expected(ora, trace=True):
    """what compare_read is given for a run with or without TraceItem lists (flags = GA_F_TRACE / 0)"""
    return ora if trace else dict(ora, trace=np.zeros((0, 7), dtype=np.int64))


def oracle_results(nodes, edges, reads, seeds, bw, ramp=0, overlap=0):
    key = (tuple(map(tuple, nodes)), tuple(map(tuple, edges)), tuple(reads), repr(seeds), bw, ramp, overlap)
    if key not in _ORACLE_MEMO:
        og = ob.OracleGraph(nodes, edges, overlap=overlap)
        oras = []
        for r, s in zip(reads, seeds):
            lst = [s] if (len(s) == 3 and not isinstance(s[0], (tuple, list))) else list(s)
            oras.append(og.align(r, lst, bw, ramp))
        _ORACLE_MEMO[key] = oras
    return _ORACLE_MEMO[key]


def run_both(nodes, edges, reads, seeds, bw, ramp=0, overlap=0, lib_path=None, trace=True):
    g = binding.Graph(nodes, edges, overlap=overlap, lib_path=lib_path)
    devs = g.align(reads, seeds, bw, ramp, flags=binding.GA_F_TRACE if trace else 0)
    return devs, oracle_results(nodes, edges, reads, seeds, bw, ramp, overlap)


def check_parity(nodes, edges, reads, seeds, bw, ramp=0, overlap=0, lib_path=None, ctx="", trace=True):
    devs, oras = run_both(nodes, edges, reads, seeds, bw, ramp, overlap, lib_path, trace)
    for i, (d, o) in enumerate(zip(devs, oras)):
        compare_read(d, expected(o, trace), "%s read %d seed %s" % (ctx, i, seeds[i]))
    return devs, oras
