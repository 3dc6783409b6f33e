"""Cases for edge support (pileups of kind "edges") of tests/test_edge_pileup.py (slot tables, on the host emulation) and
tests/test_edge_pileup_gpu.py (the product on the GPU; lib_path names another build of the library).  The batches are those of
pileup_cases.py and ops_cases.py; the expected counts are edge_model's, from the oracle's TraceItem lists alone, computed once per process
(parity_common's memo) and left unchanged.  Every batch case has one shape: prepare with GA_F_PILEUP, run, collect, add to a pileup of
kind "edges"; the counts per slot equal the model's plane, items_added equals the model's items, edge_support() equals the model's fold."""
import numpy as np

from graphaligner_amd import binding, synth
import alphabet_cases as ac
import edge_model as em
import ops_cases as oc
import oracle_binding as ob
import parity_cases as pcases
import parity_common as pc
import pileup_cases as plc

F_PILEUP = binding.GA_F_PILEUP


def long_self_loop_batch():
    """a node of 40 bases that is its own out-neighbour, and reads that go round it two and three times (test_edge_support.py's)"""
    rng = np.random.default_rng(19)
    a, loop, b = ("".join(rng.choice(list("ACGT"), size=n)) for n in (300, 40, 300))
    nodes = [(1, a), (2, loop), (3, b)]
    edges = [(1, False, 2, False), (2, False, 2, False), (2, False, 3, False)]
    return nodes, edges, [a + loop * 2 + b, a + loop * 3 + b], [(1, 0, False)] * 2


def cyclic_batch():
    node_len, bw, back_edges, self_loops, max_span = pcases.CYCLIC_GRAPHS[1]
    g = synth.cyclic_graph(5000, node_len=node_len, seed=node_len + bw, back_edges=back_edges, self_loops=self_loops, max_span=max_span)
    reads, seeds = synth.walk_reads(g, 8, 900, seed=900 + node_len, mid_seed=True, first_nodes=max(1, len(g.nodes) // 3))
    return g, reads, seeds, bw


class Case:
    """one batch: how its graph is made (nodes + edges, or a GFA text), the model's slot table, reads, seeds, bandwidth and a function that
    gives the oracle's results"""

    def __init__(self, name, nodes, edges, reads, seeds, bw, gfa=None, oracle=None):
        self.name, self.nodes, self.edges, self.reads, self.seeds, self.bw, self.gfa = name, nodes, edges, reads, seeds, bw, gfa
        self.slots = em.slot_table([n for n, _ in nodes], edges)
        self._oracle = oracle

    def graph(self, lib_path=None):
        return binding.Graph(gfa=self.gfa, lib_path=lib_path) if self.gfa is not None else binding.Graph(self.nodes, self.edges, lib_path=lib_path)

    def oracle(self):
        return self._oracle() if self._oracle else pc.oracle_results(self.nodes, self.edges, self.reads, self.seeds, self.bw)


_GFA_ORACLE = {}


def _gfa_case():
    gfa, segs, links, k, reads, seeds = plc.gfa_overlap_batch()

    def oracle():
        if "oras" not in _GFA_ORACLE:
            og = ob.OracleGraph.from_gfa_segments(segs, links, k)
            _GFA_ORACLE["oras"] = [og.align(r, [sd], 35) for r, sd in zip(reads, seeds)]
        return _GFA_ORACLE["oras"]
    return Case("gfa overlap", segs, links, reads, seeds, 35, gfa=gfa, oracle=oracle)


def graph_cases():
    """the eight batches of test_edge_support.py's cases, by name"""
    out = {}
    g, reads, seeds = plc.one_part_and_strands_batch()
    out["one part and strands"] = Case("one part and strands", g.nodes, g.edges, reads, seeds, 35)
    g, reads, seeds = plc.fan_batch()
    out["fan"] = Case("fan", g.nodes, g.edges, reads, seeds, 35)
    for node_len in (1, 8):
        g, reads, seeds = oc.round_edge_batch(node_len)
        out["round edges %d" % node_len] = Case("round edges %d" % node_len, g.nodes, g.edges, reads, seeds, 35)
    nodes, edges, reads, seeds = oc.self_loop_batch()
    out["one-base self-loop"] = Case("one-base self-loop", nodes, edges, reads, seeds, 35)
    nodes, edges, reads, seeds = long_self_loop_batch()
    out["self-loop on a 40-bp node"] = Case("self-loop on a 40-bp node", nodes, edges, reads, seeds, 35)
    g, reads, seeds, bw = cyclic_batch()
    out["cyclic"] = Case("cyclic", g.nodes, g.edges, reads, seeds, bw)
    out["gfa overlap"] = _gfa_case()
    return out


def several_seeds_case():
    g, reads, multi = plc.several_seeds_batch()
    return Case("several seeds", g.nodes, g.edges, reads, multi, 35)


def alphabet_case(name="64bp-nodes"):
    g = ac.graph(name)
    probes = [p for p in ac.all_probes() if ac.reaches_oracle(p)]
    reads = [ac.read_of(g, p) for p in probes]
    seeds = [[ac.seed_of(g, p[1])] for p in probes]
    return Case("alphabet " + name, g.nodes, g.edges, reads, seeds, ac.BW, oracle=lambda: [ac.oracle_of(name, p) for p in probes])


BATCH_NAMES = ["one part and strands", "fan", "round edges 1", "round edges 8", "one-base self-loop", "self-loop on a 40-bp node", "cyclic", "gfa overlap",
               "several seeds", "alphabet"]


def batch_case(name):
    if name == "several seeds":
        return several_seeds_case()
    if name == "alphabet":
        return alphabet_case()
    return graph_cases()[name]


# ---- the one shape of a batch case ----------------------------------------------------------------------------------------------------
def run_add(gg, reads, seeds, bw, piles):
    """one batch through the staged calls, added to every pileup of `piles` in turn -> (results, batch)"""
    b = gg.prepare(reads, seeds, bw, 0, F_PILEUP)
    b.run()
    devs = b.collect()
    for p in piles:
        p.add(b)
    return devs, b


def compare(gg, pile, slots, model, times=1, ctx=""):
    f, t = gg.edge_slots()
    assert list(zip(f.tolist(), t.tolist())) == slots, (ctx, "slot table")
    counts = pile.counts().astype(np.int64)
    assert counts.shape == (1, len(slots)) and pile.planes == 1 and pile.entries == len(slots), (ctx, counts.shape, len(slots))
    want = model.plane() * times
    if not (counts[0] == want).all():
        bad = np.flatnonzero(counts[0] != want)[:5]
        raise AssertionError((ctx, [(int(s), slots[int(s)], int(counts[0, s]), int(want[s])) for s in bad]))
    assert pile.edge_support() == em.fold(slots, want), (ctx, "fold")
    return counts


def check_case(case, lib_path=None):
    """-> (graph, pileup, model, statistics, batch)"""
    gg = case.graph(lib_path)
    oras = case.oracle()
    model = em.of(oras, gg.bp, case.slots)
    # (what keeps the case from being vacuous)
    assert model.reads >= 2 and model.items >= 1, (case.name, model.reads, model.items)
    pile = gg.pileup("edges")
    devs, b = run_add(gg, case.reads, case.seeds, case.bw, [pile])
    for i, (d, o) in enumerate(zip(devs, oras)):
        assert d["status"] == o["status"] and d["failed"] == o["failed"], (case.name, i, d["status"], o["status"])
    compare(gg, pile, case.slots, model, ctx=case.name)
    st = pile.stats()
    assert st["items_added"] == model.items and st["columns"] == len(case.slots) and st["kind"] == binding.GA_PILEUP_EDGES, (case.name, st, model.items)
    assert st["reads_from_device"] + st["reads_from_host"] == model.reads and st["batches_added"] == 1, (case.name, st, model.reads)
    return gg, pile, model, st, b


def case_seeded_batch(lib_path=None):
    """the graph and reads of test_pileup_gpu.py::test_seeded_batch_equals_two_calls"""
    g = synth.bubble_graph(60000, node_len=64, seed=71)
    reads, _ = synth.simulate_reads(g, 24, 1500, seed=17, mid_seed=True)
    gg = binding.Graph(g.nodes, g.edges, lib_path=lib_path)
    slots = em.slot_table([n for n, _ in g.nodes], g.edges)
    gg.build_seed_index()
    b = gg.prepare_seeded(reads, flags=F_PILEUP)
    b.run()
    b.collect()
    seeded = gg.pileup("edges")
    seeded.add(b)
    found = gg.find_seeds(reads)
    oras = pc.oracle_results(g.nodes, g.edges, reads, [list(s) for s in found.seeds], 35)
    model = em.of(oras, gg.bp, slots)
    assert model.reads >= 12 and model.items >= 1, (model.reads, model.items)
    compare(gg, seeded, slots, model, ctx="seeded batch")
    assert seeded.stats()["items_added"] == model.items
    return model
