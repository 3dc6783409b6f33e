"""The seed engine's buffers through their life on the GPU: ONE loaded graph keeps one engine, whose index is replaced by every build,
whose coordinate is replaced in place, and whose hit, label and work buffers are kept between the finds and grown when a find needs
more; a seeded batch launches the seeding kernel over the same hit buffers.  A buffer freed twice, kept too small, or an index left
half replaced would show in what a later call returns.  So the calls run in a row on one graph -- in-node index, finds with a small
and a large hit buffer, the first grouped find, the walk index over the live one, the topology coordinate and the file order again, a
refused build, a seeded batch, the in-node index again -- and every result must equal what the same call gives on a graph loaded
and indexed for that call alone: seeds, support, hit counts, truncated flags and locus fields, the index entries, the coordinate and
the statistics but for their times.  Integers throughout: there is no tolerance.
On this graph (nodes of 8 bp, k = 15) the in-node index has no entry: the calls under it, in the first and in the last block, check
the buffers' allocation and growth and the build of an empty index, and their comparisons are of empty results; what is found is
compared under the walk index, where 18 of the 26 reads have seeds and max_hits=16 cuts the hits of 24."""
import pytest

from graphaligner_amd import binding, synth
import seed_common as sc
import seed_coord_common as scc
import seed_loci_common as slc

pytestmark = pytest.mark.gpu
BW = 35


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need a real MI355X"


def _no_ms(stats):
    return {k: v for k, v in stats.items() if not k.endswith("_ms")}


def _state(G, walk):
    """the index and its coordinate as they lie in device memory, and the statistics (walk: those of a walk index too)"""
    keys, nodes, offs = G.seed_index_entries()
    st = _no_ms(G.seed_index_stats())
    walk = G.seed_index_walk_stats() if walk else None
    return dict(keys=keys.tobytes(), nodes=nodes.tobytes(), offs=offs.tobytes(), coordinate=G.seed_coordinate().tobytes(), stats=st,
                coord_stats=_no_ms(G.seed_coord_stats()), walk_stats=walk)


def _finds(G, reads):
    return slc.plain(G.find_seeds(reads)), slc.plain(G.find_seeds(reads, loci=True))


def _seeded(G, reads):
    b = G.prepare_seeded(reads, None, True, BW)
    b.run()
    res = b.collect(summary=True)
    seeds = slc.plain(b.seeds())
    b.close()
    return seeds, (str(res.dtype), res.shape, res.tobytes())


def test_one_engine_through_its_buffer_life_equals_a_fresh_graph_per_call():
    g = synth.bubble_graph(30000, node_len=8, seed=3)
    nodes = scc.shuffled(g.nodes)
    reads = sc.spiked_reads(g)

    def fresh(max_walks, coordinate="file"):
        G = binding.Graph(nodes, g.edges)
        G.build_seed_index(max_walks=max_walks, coordinate=coordinate)
        return G

    def small(G):
        return slc.plain(G.find_seeds(reads, max_hits=16))

    def small_loci(G):
        return slc.plain(G.find_seeds(reads, loci=True, max_hits=16))

    worn = binding.Graph(nodes, g.edges)
    # the in-node index: a small hit buffer, a grown one, the first label buffer, nothing shrinks
    worn.build_seed_index()
    assert _state(worn, False) == _state(fresh(0), False)
    assert small(worn) == small(fresh(0))
    assert slc.plain(worn.find_seeds(reads)) == slc.plain(fresh(0).find_seeds(reads))
    assert slc.plain(worn.find_seeds(reads, loci=True)) == slc.plain(fresh(0).find_seeds(reads, loci=True))
    assert small_loci(worn) == small_loci(fresh(0))

    # the walk index over the live index
    worn.build_seed_index(max_walks=64)
    walk = _state(worn, True)
    assert walk == _state(fresh(64), True)
    assert walk["walk_stats"]["max_walks"] == 64 and walk["walk_stats"]["duplicates_dropped"] >= 0 and walk["stats"]["entries"] > 0
    found = _finds(worn, reads)
    assert found == _finds(fresh(64), reads)
    # (not a comparison of empty sets: a dozen reads have seeds, and max_hits=16 cuts some reads' hits and not others')
    assert sum(1 for s in found[0][0] if s) >= 12 and sum(1 for s in found[1][0] if s) >= 12
    cut = worn.find_seeds(reads, max_hits=16).truncated
    assert any(cut) and not all(cut)
    assert small(worn) == small(fresh(64)) and small_loci(worn) == small_loci(fresh(64))

    # the coordinate replaced in place, and put back
    worn.set_seed_coordinate("topology")
    topo = _state(worn, True)
    assert topo == _state(fresh(64, "topology"), True) and topo["coordinate"] != walk["coordinate"] and topo["coord_stats"]["kind"] == 1
    assert _finds(worn, reads) == _finds(fresh(64, "topology"), reads)
    worn.set_seed_coordinate("file")
    assert _state(worn, True) == walk
    assert _finds(worn, reads) == found

    # a build refused for its parameters leaves the index in place and usable
    with pytest.raises(RuntimeError, match=r"\(100\)"):
        worn.build_seed_index(max_walks=257)
    assert worn.L.ga_graph_build_seed_index_walks(worn.h, 15, 2, 257) == 100    # GA_E_INVALID
    assert _state(worn, True) == walk
    assert _finds(worn, reads) == found

    # a seeded batch: the same hit and label buffers, through the launch over resident reads
    seeded = _seeded(worn, reads)
    assert seeded == _seeded(fresh(64), reads)
    assert seeded[0] == found[1]
    assert slc.plain(worn.find_seeds(reads, loci=True)) == found[1]

    # the in-node index again
    worn.build_seed_index()
    assert _state(worn, False) == _state(fresh(0), False)
    assert slc.plain(worn.find_seeds(reads)) == slc.plain(fresh(0).find_seeds(reads))
