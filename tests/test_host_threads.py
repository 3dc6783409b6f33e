"""The host threads (GA_HOST_THREADS) must not show in the results: the read copies, the match words and the result assembly of one batch
are cut into pieces for 1 thread and for 5 (with 600 reads: 3 copy threads, 5 fill and 5 assembly threads), and every read's results
are the same.  Runs the device program through the host emulation (no GPU needed)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from graphaligner_amd import binding, synth  # noqa: E402
import parity_common as pc  # noqa: E402

FLAGS = [0, binding.GA_F_TRACE, binding.GA_F_TRACE | binding.GA_F_OPS]
READ_FIELDS = ("status", "failed", "score", "alignment_start", "alignment_end", "query_position", "column_updates", "n_mappings", "n_trace")
_cache = {}


def _inputs():
    if "inputs" not in _cache:
        g = synth.linear_graph(30000, node_len=64, seed=5)
        reads, seeds = synth.simulate_reads(g, 400, 400, seed=3)
        more, mseeds = synth.simulate_reads(g, 200, 400, seed=4, mid_seed=True)
        reads, seeds = reads + more, seeds + mseeds
        reads[7] = reads[7][:50] + "X" + reads[7][51:]
        _cache["inputs"] = (binding.Graph(g.nodes, g.edges, lib_path=pc.emul_lib_path()), reads, seeds)
    return _cache["inputs"]


def _table(ptr, n, ctype):
    return np.frombuffer(C.string_at(ptr, n * C.sizeof(ctype)), dtype=np.dtype(ctype)) if n else np.zeros(0, dtype=np.dtype(ctype))


def _per_read(graph, batch):
    """every read's results as comparable values, read from the raw arrays of ga_results_t"""
    want_ops = bool(batch.flags & binding.GA_F_OPS)
    out = C.POINTER(binding.GaResultsOps if want_ops else binding.GaResults)()
    assert graph.L.ga_batch_collect(batch.h, C.byref(out)) == 0
    try:
        R = out.contents
        recs = _table(R.reads, R.n_reads, binding.GaReadResult)
        maps = _table(R.mappings, R.n_mappings, binding.GaMapping)
        trace = _table(R.trace, R.n_trace, binding.GaTraceItem)
        edit = C.string_at(R.edit_bytes, R.n_edit_bytes) if R.n_edit_bytes else b""
        read_ops = _table(R.read_ops, R.n_reads, binding.GaReadOps) if want_ops else None
        ops = _table(R.ops, R.n_ops, C.c_uint32) if want_ops else None
        per_read = []
        for i, r in enumerate(recs):
            m = maps[int(r["first_mapping"]):int(r["first_mapping"] + r["n_mappings"])]
            one = {f: int(r[f]) for f in READ_FIELDS}
            one["mappings"] = m.tobytes()
            one["edits"] = [edit[int(o):int(o + n)] for o, n in zip(m["edit_seq_off"], m["to_length"])]
            one["trace"] = trace[int(r["first_trace"]):int(r["first_trace"] + r["n_trace"])].tobytes()
            if want_ops:
                ro = read_ops[i]
                one["ops"] = ops[int(ro["first_op"]):int(ro["first_op"]) + int(ro["n_ops"])].tobytes()
                one["op_counts"] = tuple(int(ro[f]) for f in ("n_ops", "n_match", "n_mismatch", "n_insertion", "n_deletion"))
            per_read.append(one)
        return per_read
    finally:
        graph.L.ga_results_free(out)


def _results(flags, threads):
    """prepare, run and collect the batch with GA_HOST_THREADS = threads (once per pair: the tests share the results)"""
    if (flags, threads) not in _cache:
        graph, reads, seeds = _inputs()
        before = os.environ.get("GA_HOST_THREADS")
        os.environ["GA_HOST_THREADS"] = threads
        try:
            batch = graph.prepare(reads, seeds, 35, flags=flags)
            batch.run()
            _cache[(flags, threads)] = _per_read(graph, batch)
            batch.close()
        finally:
            if before is None:
                del os.environ["GA_HOST_THREADS"]
            else:
                os.environ["GA_HOST_THREADS"] = before
    return _cache[(flags, threads)]


def _assert_same(a, b, what):
    assert len(a) == len(b) == 600
    for i, (x, y) in enumerate(zip(a, b)):
        for key in x:
            assert x[key] == y[key], "%s: read %d differs in %s" % (what, i, key)


@pytest.mark.parametrize("flags", FLAGS)
def test_results_do_not_depend_on_the_thread_count(flags):
    one, five = _results(flags, "1"), _results(flags, "5")
    _assert_same(one, five, "flags %d, 1 thread against 5" % flags)
    aligned = sum(1 for r in five if r["status"] == 0 and not r["failed"])
    assert aligned >= 450, "only %d of 600 reads aligned: the comparison would pass on failures" % aligned
    if flags & binding.GA_F_TRACE:
        assert sum(1 for r in five if r["n_trace"]) >= 450
    if flags & binding.GA_F_OPS:
        assert sum(1 for r in five if r["op_counts"][0]) >= 450


def test_zero_threads_is_one_thread():
    flags = binding.GA_F_TRACE | binding.GA_F_OPS
    _assert_same(_results(flags, "1"), _results(flags, "0"), "GA_HOST_THREADS=0 against 1")
