"""The read alphabet on the host: alphabet_model.py (the rule as the reference's text states it) against the oracle, and the probe
sets of alphabet_cases.py through the host emulation of the device program.

The emulation runs here with its own match words withheld (profile "emul" of parity_common.PROFILES: it takes the finished words and
ignores GaEqSource), so what runs are the two host restatements of the rule: the match-word builder of ga_batch_prepare feeds the
lanes = reads program, buildRows feeds the wave-per-read ladder.  GA_LANES chooses the first pass of the
product and of the emulation, so that with the ladder first every job takes its rows from buildRows.  The kernel's own statement of the rule is test_alphabet_gpu.py's.
"""
import pytest

import alphabet_cases as ac
import alphabet_model as am
import parity_common as pc

GRAPH = pytest.mark.parametrize("name", sorted(ac.GRAPHS))


@pytest.fixture(scope="module")
def lib():
    return pc.emul_lib_path()


@pytest.fixture(autouse=True)
def host_built_tables(monkeypatch):
    """every graph of this module is uploaded with the back end's own match words withheld: the tables under test are the host's"""
    monkeypatch.setenv("GA_EMUL_WITHOUT", pc.PROFILES["emul"])


def test_model_tables():
    """the tables by count, and the bytes that differ between the three rules"""
    fw = [b for b in range(256) if am.forward_set(b) is not None]
    bw = [b for b in range(256) if am.backward_char(b) is not None]
    assert len(fw) == 30 and len(bw) == 30
    assert sorted(set(fw) - set(bw)) == [ord("H"), ord("h")] and sorted(set(bw) - set(fw)) == [ord("U"), ord("u")]
    assert all(b < 128 for b in fw + bw)
    for b in fw:
        assert am.forward_set(b) == am.forward_set(ord(chr(b).upper()))
    for b in bw:
        assert am.backward_char(b).isupper() and am.backward_char(b) == am.backward_char(ord(chr(b).upper()))
    assert am.forward_set(ord("K")) == frozenset("GT") and am.forward_set(ord("m")) == frozenset("AC")
    assert am.backward_char(ord("u")) == "A" and am.backward_char(ord("d")) == "H" and am.backward_char(ord("h")) is None
    # a backward part meets the complement: for every byte both rules accept, the turned letter's set is the complement of the set
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    for b in set(fw) & set(bw):
        assert am.forward_set(ord(am.backward_char(b))) == frozenset(comp[x] for x in am.forward_set(b)), chr(b)


def test_probe_geometry():
    """rows and parts as GaEqFill lays them out, and every edge the probe sets promise"""
    assert am.part_of(600, 300, 299) == ("backward", 0) and am.part_of(600, 300, 0) == ("backward", 299)
    assert am.part_of(600, 300, 300) == ("forward", 0) and am.part_of(600, 300, 599) == ("forward", 299)
    assert am.part_of(400, 399, 399) == (None, None) and am.part_lengths(400, 399) == (399, 0) and am.part_lengths(400, 0) == (0, 400)
    probes = ac.all_probes()
    assert len(set(probes)) == len(probes)
    seen = {}
    for n, s, p, b in probes:
        part, row = am.part_of(n, s, p)
        rows = am.part_lengths(n, s)[0 if part == "backward" else 1] if part else 0
        seen.setdefault((part, row, rows), set()).add(b)
    n, s = ac.MAIN_READ
    for part in ("backward", "forward"):
        assert seen[(part, ac.MID_ROW, 300)] == set(range(256))
        for row in ac.EDGE_ROWS + (298, 299):
            assert seen[(part, row, 300)] >= set(ac.EDGE_BYTES), (part, row)
        for rows in (193, 255, 256, 257, 319, 320, 321):
            assert seen[(part, rows - 1, rows)] >= set(ac.EDGE_BYTES), (part, rows)
    assert seen[("forward", 399, 400)] >= set(ac.EDGE_BYTES) and seen[("backward", 398, 399)] >= set(ac.EDGE_BYTES)
    assert seen[(None, None, 0)] >= set(ac.EDGE_BYTES)


@GRAPH
def test_model_equals_the_oracle(name):
    probes = ac.all_probes() + ac.big_probes() + ac.forward_only_probes()
    n = ac.check_model_against_oracle(name, probes)
    assert n == sum(1 for p in probes if p[3] != 0) and n >= len(probes) * 9 // 10


def test_model_says_something():
    """both statuses and both scores occur, in both directions, and 'U' behaves as the docstring says"""
    g = ac.graph("64bp-nodes")
    seen = {(am.part_of(p[0], p[1], p[2])[0],) + ac.model_of(g, p) for p in ac.all_probes()}
    for part in ("backward", "forward"):
        assert {(part, 0, 0), (part, 0, 1), (part, 1, None)} <= seen
    n, s = ac.MAIN_READ
    path = ac.path_of(g, n, s)
    for b in (ord("U"), ord("u")):
        assert am.expected(path, s, 150, b) == (1, None) and am.expected(path, s, 450, b) == (1, None)
        assert am.expected(path, s, 0, b) == (0, 0 if path[0:1] == b"T" else 1)
    for b in (ord("H"), ord("h")):
        assert am.expected(path, s, 150, b) == (1, None)
        assert am.expected(path, s, 450, b) == (0, 1 if path[450:451] == b"G" else 0)


@GRAPH
@pytest.mark.parametrize("trace", [True, False], ids=["trace-items", "flags-0"])
@pytest.mark.parametrize("lanes", ["0", "1"], ids=["ladder-first", "lanes-first"])
def test_probes_on_the_emulation(lib, name, lanes, trace, monkeypatch):
    monkeypatch.setenv("GA_LANES", lanes)
    ac.case_probes(name, ac.all_probes(), trace, lib)


def test_node_runs_see_the_alphabet_on_the_emulation(lib, monkeypatch):
    monkeypatch.delenv("GA_LANES", raising=False)
    ac.case_node_runs_see_the_alphabet(lib)


@pytest.mark.parametrize("trace", [True, False], ids=["trace-items", "flags-0"])
def test_sparse_variant_sees_the_alphabet_on_the_emulation(lib, trace, monkeypatch):
    """ambiguity codes, lower case and one invalid byte inside the branches of a fan whose bands take the sparse method"""
    monkeypatch.delenv("GA_LANES", raising=False)
    ac.case_sparse_variant_sees_the_alphabet(trace, lib)


def _expected_codes():
    """per byte value the row code the model asks for, forwards and backwards (layout of ga_backend.h: bits 0-3 the match set over
    A C G T, bits 4-6 the exact-compare code A0 C1 G2 T3 or 7 for none, bit 7 outside the alphabet); None: any code with bit 7"""
    fw, bw = [], []
    for b in range(256):
        for out, part in ((fw, "forward"), (bw, "backward")):
            bases = am.forward_set(b) if part == "forward" else (am.forward_set(ord(am.backward_char(b))) if am.backward_char(b) else None)
            if bases is None:
                out.append(None)
                continue
            exact = am.exact_letter(b, part)
            out.append(sum(1 << "ACGT".index(x) for x in bases) | (("ACGT".index(exact) if exact else 7) << 4))
    return fw, bw


def test_row_codes_and_match_words_state_the_rule(lib):
    """the tables themselves, byte by byte: the match words ga_batch_prepare builds and the row codes buildRows builds for the probe
    batch (kept by a hook of the emulation back end) against the model -- match sets, the exact-compare code of every row and of
    every slice's last row (which no alignment result has been seen to depend on), the flag for a row
    outside the alphabet, the padding, and which read position is which row of which job"""
    import ctypes as C
    import numpy as np
    L = C.CDLL(lib)
    L.ga_emul_kept_sizes.argtypes = [C.c_void_p]
    L.ga_emul_kept_copy.argtypes = [C.c_void_p] * 3
    name = "64bp-nodes"
    g = ac.graph(name)
    probes = ac.all_probes()
    L.ga_emul_keep_tables(1)
    try:
        ac.run_probes(name, probes, False, lib)
        sizes = np.zeros(3, dtype=np.uint64)
        L.ga_emul_kept_sizes(sizes.ctypes.data_as(C.c_void_p))
        eq, rows, jobs = np.zeros(int(sizes[0]), dtype=np.uint64), np.zeros(int(sizes[1]), dtype=np.uint8), np.zeros((int(sizes[2]), 2), dtype=np.uint64)
        L.ga_emul_kept_copy(*(a.ctypes.data_as(C.c_void_p) for a in (eq, rows, jobs)))
    finally:
        L.ga_emul_keep_tables(0)
    fw, bw = _expected_codes()
    pad = fw[ord("N")]
    assert pad == 0x7f and fw[ord("a")] == 0x71 and bw[ord("a")] == 0x38 and bw[ord("u")] == 0x01 and fw[ord("u")] is None
    refused = [pr for pr in probes if am.part_lengths(pr[0], pr[1])[0] and any(am.backward_char(c) is None for c in ac.read_of(g, pr)[:pr[1]])]
    n_jobs = sum(sum(1 for rows in am.part_lengths(pr[0], pr[1]) if rows) for pr in probes if pr not in set(refused))
    assert len(jobs) == n_jobs, ("jobs made", len(jobs), "the model has", n_jobs, "(reads whose prefix ReverseComplement refuses make none)")
    k = 0
    checked = 0
    for probe in probes:
        n, s, p, b = probe
        read = ac.read_of(g, probe)
        bw_rows, fw_rows = am.part_lengths(n, s)
        parts = []
        if bw_rows:
            if any(am.backward_char(c) is None for c in read[:s]):
                continue                        # ReverseComplement refuses the prefix: the read ends before any job is made
            parts.append((bw, read[:s][::-1]))
        if fw_rows:
            parts.append((fw, read[s:]))
        for lut, chars in parts:
            off, padded = int(jobs[k, 0]), int(jobs[k, 1])
            k += 1
            assert padded == (len(chars) + 63) // 64 * 64 and off % 64 == 0, ac.describe(probe)
            want = [lut[c] for c in chars] + [pad] * (padded - len(chars))
            got = rows[off:off + padded]
            for r, (w, c) in enumerate(zip(want, got)):
                assert (c & 0x80 and w is None) or c == w, (ac.describe(probe), "row", r, "code", hex(c), "model", w)
            for sl in range(padded // 64):
                w64, words = want[sl * 64:sl * 64 + 64], eq[(off // 64 + sl) * 5:(off // 64 + sl) * 5 + 5]
                for bit in range(4):
                    assert int(words[bit]) == sum(1 << i for i, w in enumerate(w64) if w is not None and w >> bit & 1), (ac.describe(probe), "slice", sl, "word", bit)
                invalid = any(w is None for w in w64)
                assert int(words[4]) >> 3 == int(invalid), (ac.describe(probe), "slice", sl, "invalid flag")
                if w64[63] is not None:
                    assert int(words[4]) & 7 == w64[63] >> 4, (ac.describe(probe), "slice", sl, "exact code of the last row", int(words[4]) & 7, w64[63] >> 4)
            checked += 1
    assert k == len(jobs) and checked >= len(probes)
