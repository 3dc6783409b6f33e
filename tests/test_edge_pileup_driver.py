"""The driver's --edge-support-out file against edge_model for a small FASTQ -- exactly the edges of the bigraph whose folded count is
>= 1 --, alone and together with --pileup-out, and the driver's other output unchanged by the option, through the product library on the
GPU (the host emulation of tests/emul has no pileups); the option's parsing needs no GPU."""
import gzip

import pytest

from graphaligner_amd import aligner, binding
import edge_model as em
import oracle_binding as ob
import test_pileup_driver as tpd


def _drive(tmp_path, lib, edge_support, pileup):
    """test_pileup_driver._drive with the options of this test"""
    real = aligner.parse_args

    def parse(args):
        extra = ["--edge-support-out", str(tmp_path / "edges.txt")] if edge_support else []
        return real([a for a in args] + extra)
    aligner.parse_args = parse
    try:
        return tpd._drive(tmp_path, lib, pileup)
    finally:
        aligner.parse_args = real


def _check(tmp_path, lib):
    g, names, reads, seeds, written, out, err = _drive(tmp_path / "with", lib, True, False)
    _, _, _, _, written0, out0, err0 = _drive(tmp_path / "without", lib, False, False)
    _, _, _, _, written2, out2, err2 = _drive(tmp_path / "both", lib, True, True)
    _, _, _, _, _, _, _ = _drive(tmp_path / "pileup", lib, False, True)
    assert out == out0 == out2 and err == err0 == err2
    assert gzip.decompress((tmp_path / "with" / "out.gam").read_bytes()) == gzip.decompress((tmp_path / "without" / "out.gam").read_bytes())
    assert not (tmp_path / "without" / "edges.txt").exists() and not (tmp_path / "with" / "pileup.tsv").exists()
    assert [n for n, _ in written] == [n for n, _ in written0] == [n for n, _ in written2] and len(written) == 6
    # together with --pileup-out both files are what each option writes alone
    assert (tmp_path / "both" / "edges.txt").read_text() == (tmp_path / "with" / "edges.txt").read_text()
    assert (tmp_path / "both" / "pileup.tsv").read_text() == (tmp_path / "pileup" / "pileup.tsv").read_text()
    og = ob.OracleGraph(g.nodes, g.edges)
    bp = binding.Graph(g.nodes, g.edges, lib_path=lib).bp
    slots = em.slot_table([n for n, _ in g.nodes], g.edges)
    model = em.Model(slots)
    for n, _ in written:
        k = names.index(n)
        model.add(og.align(reads[k], [seeds[k]], 35), bp)
    assert model.reads == 6 and model.items > 100
    want = {key: c for key, c in em.fold(slots, model.plane()).items() if c >= 1}
    got, last = {}, None
    for line in (tmp_path / "with" / "edges.txt").read_text().splitlines():
        f = [int(x) for x in line.split(" ")]
        assert len(f) == 5 and f[1] in (0, 1) and f[3] in (0, 1) and f[4] >= 1, line
        key = (2 * f[0] + f[1], 2 * f[2] + f[3])
        assert key not in got and (last is None or key > last), line
        got[key] = f[4]
        last = key
    assert got == want and sum(got.values()) == model.items
    # (both strands are crossed: some written edge sums a directed edge and its mirror)
    assert any(model.counts.get((a, b), 0) and model.counts.get((b ^ 1, a ^ 1), 0) for a, b in want)


def test_edge_support_out_option_is_parsed():
    base = ["-g", "g.gfa", "-f", "r.fastq", "-s", "s.gam", "-t", "1", "-b", "35"]
    p = aligner.parse_args(base + ["--edge-support-out", "e.txt"])
    assert p.edgeSupportFile == "e.txt" and p.pileupFile == ""
    p = aligner.parse_args(base + ["--edge-support-out", "e.txt", "--pileup-out", "p.tsv"])
    assert p.edgeSupportFile == "e.txt" and p.pileupFile == "p.tsv"
    assert aligner.parse_args(base).edgeSupportFile == ""


@pytest.mark.gpu
def test_edge_support_out_gpu(tmp_path):
    import torch
    assert torch.cuda.is_available(), "this test needs a real MI355X"
    _check(tmp_path, None)
