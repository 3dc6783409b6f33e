"""The driver's --sites-out and --supported-edges-out files against site_model over the planes that pileup_model and edge_model sum from the
oracle's TraceItem lists, for a small FASTQ, and the driver's other output and files unchanged by the options, through the product
library on the GPU (the host emulation of tests/emul has no pileups); the options' parsing needs no GPU."""
import gzip
import io

import numpy as np
import pytest

from graphaligner_amd import aligner, binding
import oracle_binding as ob
import site_cases as sc
import test_pileup_driver as tpd

assert binding.GA_SITES_FOLD == 1
BASE = ["-g", "g.gfa", "-f", "r.fastq", "-s", "s.gam", "-t", "1", "-b", "35"]


def _drive(tmp_path, lib, extra):
    """test_pileup_driver._drive (with --pileup-out) and more options"""
    real = aligner.parse_args

    def parse(args):
        return real([a for a in args] + [x if not x.startswith("@") else str(tmp_path / x[1:]) for x in extra])
    aligner.parse_args = parse
    try:
        return tpd._drive(tmp_path, lib, True)
    finally:
        aligner.parse_args = real


def _check(tmp_path, lib):
    old = ["--edge-support-out", "@edges.txt"]
    g, names, reads, seeds, written, out, err = _drive(tmp_path / "fold", lib, old + ["--sites-out", "@sites.tsv", "--sites-fold", "--sites-min-depth", "2", "--sites-min-alt", "1",
                                                                                  "--sites-frac", "1/4", "--supported-edges-out", "@supported.txt", "--min-edge-support", "2"])
    _, _, _, _, written0, out0, err0 = _drive(tmp_path / "without", lib, old)
    _, _, _, _, _, out1, err1 = _drive(tmp_path / "plain", lib, ["--sites-out", "@sites.tsv", "--supported-edges-out", "@supported.txt"])
    # the existing output and files are what they are without the options
    assert out == out0 == out1 and err == err0 == err1
    assert gzip.decompress((tmp_path / "fold" / "out.gam").read_bytes()) == gzip.decompress((tmp_path / "without" / "out.gam").read_bytes())
    for f in ("pileup.tsv", "edges.txt"):
        assert (tmp_path / "fold" / f).read_text() == (tmp_path / "without" / f).read_text()
    assert not (tmp_path / "without" / "sites.tsv").exists() and not (tmp_path / "plain" / "edges.txt").exists()
    assert [n for n, _ in written] == [n for n, _ in written0] and len(written) == 6
    # the model: the planes of the six written reads from the oracle's lists
    og = ob.OracleGraph(g.nodes, g.edges)
    keep = [names.index(n) for n, _ in written]
    oras = [og.align(reads[k], [seeds[k]], 35) for k in keep]
    c = sc.SiteCase("driver", ("bases", "edges"), g.nodes, g.edges, [reads[k] for k in keep], [seeds[k] for k in keep], 35, oracle=lambda: oras)
    gg = binding.Graph(g.nodes, g.edges, lib_path=lib)
    planes = c.model_planes(gg, "bases")
    text = {}
    for n, s in g.nodes:
        text[(n, 0)], text[(n, 1)] = s, s[::-1].translate(str.maketrans("ACGT", "TGCA"))
    for sub, fold, q in (("fold", True, dict(min_depth=2, min_alt=1, alt_frac=(1, 4))), ("plain", False, dict())):
        want_e, want_F = c.want(planes, "bases", fold, **q)
        assert len(want_e) > 0
        if fold:
            assert c.both_strands(planes, "bases", c.want(planes, "bases", True)[0]).any()
        lines = (tmp_path / sub / "sites.tsv").read_text().splitlines()
        assert len(lines) == len(want_e)
        node = np.searchsorted(c.node_start, want_e, side="right") - 1
        for line, e, F, nd in zip(lines, want_e, want_F, node):
            f = line.split("\t")
            did, off = c.ids[nd], int(e - c.node_start[nd])
            assert len(f) == 12 and f[:3] == [str(did // 2), "-" if did & 1 else "+", str(off)] and f[3] == text[(did // 2, did & 1)][off], line
            assert [int(x) for x in f[4:]] == F.tolist(), line
            assert not (fold and did & 1)
    # supported edges: the lines of --edge-support-out at the threshold
    edge_lines = (tmp_path / "fold" / "edges.txt").read_text().splitlines()
    assert (tmp_path / "plain" / "supported.txt").read_text().splitlines() == edge_lines and len(edge_lines) > 0
    at2 = [l for l in edge_lines if int(l.split(" ")[4]) >= 2]
    assert (tmp_path / "fold" / "supported.txt").read_text().splitlines() == at2 and 0 < len(at2) < len(edge_lines)


def test_sites_options_are_parsed():
    p = aligner.parse_args(BASE)
    assert p.sitesFile == "" and p.supportedEdgesFile == "" and p.sitesMinDepth == 1 and p.sitesMinAlt == 0 and p.sitesFrac == (0, 1) and not p.sitesFold and p.minEdgeSupport == 1
    p = aligner.parse_args(BASE + ["--sites-out", "s.tsv", "--sites-min-depth", "3", "--sites-min-alt", "2", "--sites-frac", "1/4", "--sites-fold"])
    assert p.sitesFile == "s.tsv" and (p.sitesMinDepth, p.sitesMinAlt, p.sitesFrac, p.sitesFold) == (3, 2, (1, 4), True) and p.pileupFile == "" and p.edgeSupportFile == ""
    p = aligner.parse_args(BASE + ["--supported-edges-out", "e.txt", "--min-edge-support", "5"])
    assert p.supportedEdgesFile == "e.txt" and p.minEdgeSupport == 5 and p.sitesFile == ""
    for bad in (["--sites-min-depth", "0"], ["--sites-frac", "3/2"], ["--sites-frac", "1/65536"], ["--sites-frac", "1/0"], ["--min-edge-support", "0"]):
        with pytest.raises(SystemExit):
            aligner.parse_args(BASE + bad, err=io.StringIO())


@pytest.mark.gpu
def test_sites_out_gpu(tmp_path):
    import torch
    assert torch.cuda.is_available(), "this test needs a real MI355X"
    _check(tmp_path, None)
