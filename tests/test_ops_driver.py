"""The driver's --ops-out file against ops_model for a small FASTQ, and the driver's other output unchanged by the option (host build of
tests/emul; the `gpu` test runs the same through the product library)."""
import gzip
import io

import pytest

from graphaligner_amd import aligner, binding, synth
import ops_model as om
import oracle_binding as ob
import parity_common as pc
import test_aligner_driver as tad


def _drive(tmp_path, lib, ops):
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
    p = aligner.parse_args(args + (["--ops-out", str(tmp_path / "ops.tsv")] if ops else []))
    p.outputDir = str(tmp_path)
    out, err = io.StringIO(), io.StringIO()
    written = aligner.align_reads(p, lib_path=lib, out=out, err=err)
    return g, names, reads, seeds, written, out.getvalue().replace(str(tmp_path), "DIR"), err.getvalue()


def _check(tmp_path, lib):
    g, names, reads, seeds, written, out, err = _drive(tmp_path / "with", lib, True)
    _, _, _, _, written0, out0, err0 = _drive(tmp_path / "without", lib, False)
    assert out == out0 and err == err0
    # (a GAM file is gzip members, whose headers carry the time of writing: the bytes compared are the members' contents)
    assert gzip.decompress((tmp_path / "with" / "out.gam").read_bytes()) == gzip.decompress((tmp_path / "without" / "out.gam").read_bytes())
    assert not (tmp_path / "without" / "ops.tsv").exists()
    for (n, a), (n0, b) in zip(written, written0):
        assert n == n0 and "ops" in a and "ops" not in b
        trace_a = open(tmp_path / "with" / aligner._safe("trace_0_%s.trace" % n)).read()
        assert trace_a == open(tmp_path / "without" / aligner._safe("trace_0_%s.trace" % n)).read()
    og = ob.OracleGraph(g.nodes, g.edges)
    lines = (tmp_path / "with" / "ops.tsv").read_text().splitlines()
    assert [l.split("\t")[0] for l in lines] == [n for n, _ in written] and len(lines) == 6
    for line in lines:
        name, m, x, i, d, identity, runs = line.split("\t")
        k = names.index(name)
        want = om.oracle_ops(og.align(reads[k], [seeds[k]], 35))
        assert runs == binding.ops_string(want) and "|" in runs
        assert (int(m), int(x), int(i), int(d)) == om.counts_of(want)
        assert identity == "%.6f" % (int(m) / (int(m) + int(x) + int(i) + int(d)))


def test_ops_out_emulated(tmp_path):
    _check(tmp_path, pc.emul_lib_path())


@pytest.mark.gpu
def test_ops_out_gpu(tmp_path):
    import torch
    assert torch.cuda.is_available(), "this test needs a real MI355X"
    _check(tmp_path, None)
