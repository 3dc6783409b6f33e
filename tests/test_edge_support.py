"""Edge support without a GPU: binding.fold_edge_support, and the rule of edge_model.py held against the mappings of the same oracle
results.  (A pileup kind that sums the rule's counts on the device is not in the tree; edge_model is what it is to be checked against.)
Without binding.fold_edge_support every test here fails at the import check below."""
import numpy as np
import pytest

from graphaligner_amd import binding, synth
import edge_model as em
import ops_cases as oc
import oracle_binding as ob
import parity_cases as pcases
import parity_common as pc
import pileup_cases as plc

assert callable(binding.fold_edge_support)


def test_fold_sums_an_edge_with_its_mirror():
    edge_list = (np.array([2, 5, 2, 8, 9]), np.array([4, 3, 6, 8, 9]))
    got = binding.fold_edge_support(edge_list, [3, 4, 1, 2, 5])
    # (5 -> 3 is the mirror of 2 -> 4; a self-loop 8 -> 8 and the other strand's 9 -> 9 are one edge of the bigraph)
    assert got == {(2, 4): 7, (2, 6): 1, (8, 8): 7} == em.fold(list(zip(*[x.tolist() for x in edge_list])), [3, 4, 1, 2, 5])
    assert binding.fold_edge_support(([], []), []) == {}
    assert binding.fold_edge_support(([7], [2]), np.array([[4]], dtype=np.uint32)) == {(3, 6): 4}
    with pytest.raises(ValueError):
        binding.fold_edge_support(edge_list, [1, 2])
    # many edges over few ids: repeated edges, self-loops, edges that are their own mirror (a -> a ^ 1)
    rng = np.random.default_rng(5)
    a, b, c = rng.integers(0, 40, size=3000), rng.integers(0, 40, size=3000), rng.integers(0, 1000, size=3000)
    a[:50] = b[:50] ^ 1
    assert binding.fold_edge_support((a, b), c) == em.fold(list(zip(a.tolist(), b.tolist())), c.tolist())


def test_fold_of_a_slot_table_has_one_key_per_bigraph_edge():
    """over the slot table of a bubble graph -- every bigraph edge is there as two directed edges -- the fold has one key per distinct
    bigraph edge, each the sum of its two slots, and nothing is lost"""
    g, _, _ = plc.one_part_and_strands_batch()
    slots = em.slot_table([n for n, _ in g.nodes], g.edges)
    counts = np.arange(1, len(slots) + 1)
    folded = binding.fold_edge_support(([a for a, _ in slots], [b for _, b in slots]), counts)
    distinct = {(f, bool(fs), t, bool(te)) for f, fs, t, te in g.edges}
    assert len(slots) == 2 * len(distinct) and len(folded) == len(distinct)
    assert sum(folded.values()) == int(counts.sum()) and folded == em.fold(slots, counts)
    where = {e: i for i, e in enumerate(slots)}
    for (a, b), c in folded.items():
        assert c == counts[where[(a, b)]] + counts[where[(b ^ 1, a ^ 1)]]


# ---- the rule against the mappings of the same lists, on the oracle alone ---------------------------------------------------------------
def long_self_loop_batch():
    """a node of 40 bases that is its own out-neighbour, and reads that go round it two and three times"""
    rng = np.random.default_rng(19)
    a, loop, b = ("".join(rng.choice(list("ACGT"), size=n)) for n in (300, 40, 300))
    nodes = [(1, a), (2, loop), (3, b)]
    edges = [(1, False, 2, False), (2, False, 2, False), (2, False, 3, False)]
    return nodes, edges, [a + loop * 2 + b, a + loop * 3 + b], [(1, 0, False)] * 2


def _oracle_cases():
    """(name, slot table, graph bp, oracle results, the difference every read must have or None)"""
    emul = pc.emul_lib_path()

    def plain(name, nodes, edges, reads, seeds, bw, exact=None):
        return (name, em.slot_table([n for n, _ in nodes], edges), binding.Graph(nodes, edges, lib_path=emul).bp,
                pc.oracle_results(nodes, edges, reads, seeds, bw), exact)

    g, reads, seeds = plc.one_part_and_strands_batch()
    yield plain("one part and strands", g.nodes, g.edges, reads, seeds, 35)
    g, reads, seeds = plc.fan_batch()
    yield plain("fan", g.nodes, g.edges, reads, seeds, 35, exact=0)
    # (1-bp nodes: the first cell of the one part is a node's last offset, so the crossing out of it is the one not counted)
    g, reads, seeds = oc.round_edge_batch(1)
    yield plain("round edges 1", g.nodes, g.edges, reads, seeds, 35, exact=1)
    g, reads, seeds = oc.round_edge_batch(8)
    yield plain("round edges 8", g.nodes, g.edges, reads, seeds, 35, exact=0)
    nodes, edges, reads, seeds = oc.self_loop_batch()
    yield plain("one-base self-loop", nodes, edges, reads, seeds, 35, exact=0)
    nodes, edges, reads, seeds = long_self_loop_batch()
    yield plain("self-loop on a 40-bp node", nodes, edges, reads, seeds, 35, exact=0)
    node_len, bw, back_edges, self_loops, max_span = pcases.CYCLIC_GRAPHS[1]
    g = synth.cyclic_graph(5000, node_len=node_len, seed=node_len + bw, back_edges=back_edges, self_loops=self_loops, max_span=max_span)
    reads, seeds = synth.walk_reads(g, 8, 900, seed=900 + node_len, mid_seed=True, first_nodes=max(1, len(g.nodes) // 3))
    yield plain("cyclic", g.nodes, g.edges, reads, seeds, bw)
    gfa, segs, links, k, reads, seeds = plc.gfa_overlap_batch()
    og = ob.OracleGraph.from_gfa_segments(segs, links, k)
    yield ("gfa overlap", em.slot_table([n for n, _ in segs], links), binding.Graph(gfa=gfa, lib_path=emul).bp,
           [og.align(r, [sd], 35) for r, sd in zip(reads, seeds)], None)


def test_model_against_the_mappings_of_the_same_reads():
    """every pair of consecutive items in two columns of two nodes is an edge of the graph -- back edges, self-loops and the overlap GFA
    included --, and per read the crossings counted are the read's node changes, len(mappings) - 1, less 0, 1 or 2 (a crossing out of the
    first cell of a part, or across the SPLIT).  A turn through a self-loop on a node longer than one base is a counted crossing that
    starts no new mapping, so it is set aside first: only there is len(mappings) - 1 - count negative.  Where every read of a case must
    have the same difference, that value is asserted."""
    crossings, negative, turns = 0, {}, {}
    for name, slots, bp, oras, exact in _oracle_cases():
        edge_set = set(slots)
        assert len(edge_set) == len(slots)
        model = em.of(oras, bp, slots)
        assert model.reads >= 2, name
        for o, n in zip(oras, model.per_read):
            if n is None:
                continue
            every = em.crossings_of(o, bp, None)
            assert all(e in edge_set for e in every), (name, [e for e in every if e not in edge_set][:3])
            assert len(every) == n
            crossings += n
            loop_turns = sum(1 for a, b in every if a == b)
            diff = len(o["mappings"]) - 1 - n
            assert 0 <= diff + loop_turns <= 2, (name, len(o["mappings"]), n, loop_turns)
            assert exact is None or diff + loop_turns == exact, (name, diff, loop_turns, exact)
            assert (diff < 0) <= (loop_turns > 0), (name, diff, loop_turns)
            negative[name] = negative.get(name, 0) + (diff < 0)
            turns[name] = turns.get(name, 0) + loop_turns
        assert int(model.plane().sum()) == model.items
        if name == "self-loop on a 40-bp node":
            # last offset to offset 0: one count per further turn of the two reads, and both reads' differences negative
            assert model.counts == {(2, 4): 2, (4, 4): 1 + 2, (4, 6): 2} and negative[name] == 2
        if name == "cyclic":
            assert turns[name] > 0 and negative[name] > 0 and any(a > b for (a, b), c in model.counts.items() if c and a % 2 == 0 and b % 2 == 0)      # (a back edge on the forward strand)
    assert crossings > 2000 and all(v == 0 for k, v in negative.items() if k not in ("self-loop on a 40-bp node", "cyclic")), negative


def test_one_base_self_loop_and_both_strands():
    """the one-base loop's own edge is never counted, the edges into and out of the loop node once per read; reads with backward parts
    count some edge and its mirror"""
    nodes, edges, reads, seeds = oc.self_loop_batch()
    bp = binding.Graph(nodes, edges, lib_path=pc.emul_lib_path()).bp
    model = em.of(pc.oracle_results(nodes, edges, reads, seeds, 35), bp, em.slot_table([n for n, _ in nodes], edges))
    assert (4, 4) in model.edge_set and model.counts == {(2, 4): 2, (4, 6): 2}
    g, reads, seeds = plc.one_part_and_strands_batch()
    bp = binding.Graph(g.nodes, g.edges, lib_path=pc.emul_lib_path()).bp
    model = em.of(pc.oracle_results(g.nodes, g.edges, reads, seeds, 35), bp, em.slot_table([n for n, _ in g.nodes], g.edges))
    assert any(model.counts.get((b ^ 1, a ^ 1), 0) > 0 for (a, b), c in model.counts.items() if c > 0)


def test_fold_keeps_what_supported_subgraph_keeps():
    """SupportedSubgraph (SupportedSubgraph.cpp:27-42, 52-68) works on node ids without strand: node b follows node a in some
    alignment's mappings, and an edge from -> to of the graph is kept when (from, to) or (to, from) is such a pair.  Reads that start
    at node starts and cover their region several times over cross no edge only out of a part's first cell or across a SPLIT, so for
    every edge of the bigraph the folded count of the rule is >= 1 exactly when the reference's rule keeps the edge"""
    g, reads, seeds = oc.round_edge_batch(64)
    bp = binding.Graph(g.nodes, g.edges, lib_path=pc.emul_lib_path()).bp
    slots = em.slot_table([n for n, _ in g.nodes], g.edges)
    oras = pc.oracle_results(g.nodes, g.edges, reads, seeds, 35)
    model = em.of(oras, bp, slots)
    folded = binding.fold_edge_support(([a for a, _ in slots], [b for _, b in slots]), model.plane())
    sup = set()
    for o in oras:
        if o["status"] == 0 and not o["failed"]:
            ids = [int(m[0]) >> 1 for m in o["mappings"]]       # (a mapping's node id is the digraph id)
            sup |= set(zip(ids, ids[1:]))
    kept = 0
    for f, fs, t, te in g.edges:
        a, b = 2 * f + (1 if fs else 0), 2 * t + (1 if te else 0)       # the edge's forward copy (BigraphToDigraph.cpp:32-56)
        by_fold = folded[min((a, b), (b ^ 1, a ^ 1))] >= 1
        by_reference = (f, t) in sup or (t, f) in sup
        assert by_fold == by_reference, (f, fs, t, te)
        kept += by_fold
    assert 4 <= kept < len(g.edges)
