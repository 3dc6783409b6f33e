"""The driver's --corrected-out file for the small FASTQ of test_ops_driver.py, on the GPU (the host emulation of the back end writes no
path sequences): one FASTA record per aligned read, every sequence the binding's, and the driver's other output unchanged by the option."""
import gzip
import io

import pytest

from graphaligner_amd import aligner, binding, synth
import test_aligner_driver as tad


def _drive(tmp_path, corrected):
    """the graph, reads and seeds of test_ops_driver._drive, through the product library"""
    g = synth.bubble_graph(30000, node_len=32, seed=21)
    reads, seeds = synth.simulate_reads(g, 6, 1200, seed=77, mid_seed=True)
    reads.append(reads[0][:100])                     # too short: the engine asserts
    seeds.append(seeds[0])
    names = ["r%d/x:%d" % (i, i) for i in range(len(reads))] + ["orphan"]
    reads.append("ACGT" * 80)                        # a read without seed hits
    tmp_path.mkdir(exist_ok=True)
    (tmp_path / "g.gfa").write_text(g.gfa())
    with open(tmp_path / "reads.fastq", "w") as f:
        for n, r in zip(names, reads):
            f.write("@%s\n%s\n+\n%s\n" % (n, r, "I" * len(r)))
    (tmp_path / "seeds.gam").write_bytes(tad._seed_gam([(n, s) for n, s in zip(names, seeds)]))
    args = ["-g", str(tmp_path / "g.gfa"), "-f", str(tmp_path / "reads.fastq"), "-s", str(tmp_path / "seeds.gam"), "-a", str(tmp_path / "out.gam"), "-t", "1", "-b", "35"]
    p = aligner.parse_args(args + (["--corrected-out", str(tmp_path / "corrected.fa")] if corrected else []))
    p.outputDir = str(tmp_path)
    out, err = io.StringIO(), io.StringIO()
    written = aligner.align_reads(p, out=out, err=err)
    return g, names, reads, seeds, written, out.getvalue().replace(str(tmp_path), "DIR"), err.getvalue()


@pytest.mark.gpu
def test_corrected_out_gpu(tmp_path):
    import torch
    assert torch.cuda.is_available(), "this test needs a real MI355X"
    g, names, reads, seeds, written, out, err = _drive(tmp_path / "with", True)
    _, _, _, _, written0, out0, err0 = _drive(tmp_path / "without", False)
    assert out == out0 and err == err0
    # (a GAM file is gzip members, whose headers carry the time of writing: the bytes compared are the members' contents)
    assert gzip.decompress((tmp_path / "with" / "out.gam").read_bytes()) == gzip.decompress((tmp_path / "without" / "out.gam").read_bytes())
    assert not (tmp_path / "without" / "corrected.fa").exists()
    assert all("path_seq" in a and "path_seq" not in b for (_, a), (_, b) in zip(written, written0))
    lines = (tmp_path / "with" / "corrected.fa").read_text().splitlines()
    assert len(lines) == 2 * len(written) == 12
    assert [l for l in lines[0::2]] == [">" + n for n, _ in written]
    # the binding's own answer for the same reads (the driver's reads without an alignment are not in the file)
    gg = binding.Graph(g.nodes, g.edges)
    direct = gg.align(reads[:len(seeds)], seeds, 35, 0, binding.GA_F_PATHSEQ)
    by_name = dict(zip(names, direct))
    for name, seq in zip(lines[0::2], lines[1::2]):
        d = by_name[name[1:]]
        assert d["status"] == 0 and not d["failed"] and seq.encode() == d["path_seq"] and 0 < d["path_seq_backward"] < len(seq)
