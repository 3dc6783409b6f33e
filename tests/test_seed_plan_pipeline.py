"""The pipelines with seeds=None: sharding.run_overlapped, align_queued and align_sharded with find_seeds=dict(params=..., loci=...) make
seeded batches (Graph.prepare_seeded) and must give what the same functions give with the seeds of Graph.find_seeds passed in, for all
three result forms.  Host build of tests/emul."""
import pytest

from graphaligner_amd import binding, sharding, synth
import parity_common as pc
import seed_plan_common as spc

SUMMARY_FIELDS = ("status", "failed", "score", "n_mappings", "alignment_start", "alignment_end", "query_position", "column_updates")


@pytest.fixture(scope="module")
def world():
    g = synth.bubble_graph(40000, node_len=32, seed=11)
    G = binding.Graph(g.nodes, g.edges, lib_path=pc.emul_lib_path())
    G.build_seed_index()
    reads = spc.mixed_reads(g, 26, length=700, seed=9)
    reads = [r[: 400 + (53 * i) % 300] if len(r) > 300 else r for i, r in enumerate(reads)]      # ragged lengths
    return G, reads, ["r%03d" % i for i in range(len(reads))]


@pytest.mark.parametrize("loci", [False, True], ids=["hits", "loci"])
def test_queue_without_seeds_equals_queue_with_seeds(world, loci):
    G, reads, names = world
    how = dict(params=dict(max_seeds=2), loci=loci)
    seeds = G.find_seeds(reads, loci=loci, max_seeds=2).seeds
    assert sum(1 for s in seeds if s) >= 20 and sum(1 for s in seeds if not s) >= 4
    spc.same_results(sharding.align_queued(G, reads, None, 35, chunk_reads=7, find_seeds=how), sharding.align_queued(G, reads, seeds, 35, chunk_reads=7))
    a = sharding.align_queued(G, reads, None, 35, chunk_reads=7, summary=True, find_seeds=how)
    b = sharding.align_queued(G, reads, seeds, 35, chunk_reads=7, summary=True)
    assert all((a[f] == b[f]).all() for f in SUMMARY_FIELDS)
    assert sharding.align_queued(G, reads, None, 35, chunk_reads=7, gam=True, names=names, find_seeds=how) == \
        sharding.align_queued(G, reads, seeds, 35, chunk_reads=7, gam=True, names=names)
    spc.same_results(sharding.align_sharded(G, reads, None, 35, find_seeds=how), sharding.align_sharded(G, reads, seeds, 35))


def test_overlapped_inputs_without_seeds(world):
    G, reads, names = world
    how = dict(params=None, loci=True)
    seeds = G.find_seeds(reads, loci=True).seeds
    cuts = [(0, 9), (9, 10), (10, len(reads))]
    for form in (dict(), dict(summary=True), dict(gam=True)):
        if form.get("gam"):
            with_seeds = [(k, binding.ReadSet(reads[a:b], seeds[a:b], names[a:b])) for k, (a, b) in enumerate(cuts)]
            without = [(k, binding.ReadSet(reads[a:b], [[]] * (b - a), names[a:b])) for k, (a, b) in enumerate(cuts)]
        else:
            with_seeds = [(k, (reads[a:b], seeds[a:b])) for k, (a, b) in enumerate(cuts)]
            without = [(k, (reads[a:b], None)) for k, (a, b) in enumerate(cuts)]
        want = sharding.run_overlapped(G, with_seeds, 35, **form)
        got = sharding.run_overlapped(G, without, 35, find_seeds=how, **form)
        assert [k for k, _ in got] == [k for k, _ in want] == [0, 1, 2]
        for (_, x), (_, y) in zip(got, want):
            if form.get("gam"):
                assert x == y
            elif form.get("summary"):
                assert all((x[f] == y[f]).all() for f in SUMMARY_FIELDS)
            else:
                spc.same_results(x, y)
    with pytest.raises(ValueError):
        sharding.align_queued(G, reads, None, 35)
