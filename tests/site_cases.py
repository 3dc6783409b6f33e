"""Cases for site queries on whole batches (tests/test_pileup_sites_gpu.py on the GPU; tests/test_pileup_sites.py confirms on the CPU, from
the oracle alone, that no case is vacuous).  The batches are those of pileup_cases.py and ops_cases.py; the oracle's results are computed
once per process and left unchanged.  A case knows its graph's tables for site_model (node_start, twin, forward from the nodes in the
order the graph was built in; the mirror slot of every slot from the slot table) and its expected planes from the oracle's TraceItem
lists (pileup_model, edge_model)."""
import numpy as np

from graphaligner_amd import synth
import edge_cases as ec
import edge_model as em
import ops_cases as oc
import pileup_cases as plc
import pileup_model as pm
import site_model as sm

QUERIES = [dict(min_depth=1, min_alt=0), dict(min_depth=1, min_alt=1), dict(min_depth=2, min_alt=1, alt_frac=(1, 4))]
# (what the kinds without alleles are asked: X is 0 there, so a query with min_alt = 1 selects nothing by the rule -- it is still compared)
NAMES = ["round edges 64", "round edges 1", "indels", "one part and strands", "crossings", "fan", "gfa overlap", "added twice"]


class SiteCase:
    def __init__(self, name, kinds, nodes, edges, reads, seeds, bw, times=1, gfa=None, oracle=None, folds=True):
        self.name, self.kinds, self.times, self.folds = name, kinds, times, folds
        self.batch = ec.Case(name, nodes, edges, reads, seeds, bw, gfa=gfa, oracle=oracle)
        if folds:
            ids = [0] + [i for n, _ in nodes for i in (2 * n, 2 * n + 1)] + [0]
            lens = [1] + [len(s) for _, s in nodes for _ in (0, 1)] + [1]
            self.node_start, self.twin, self.forward = sm.tables_of_graph(ids, lens)
            self.ids = ids
        else:
            self.node_start = self.twin = self.forward = None
        place = {e: k for k, e in enumerate(self.batch.slots)}
        self.mirror = np.array([place.get((t ^ 1, f ^ 1), 0xffffffff) if f > 1 and t > 1 else 0xffffffff for f, t in self.batch.slots], dtype=np.int64)

    def graph(self, lib_path=None):
        return self.batch.graph(lib_path)

    def model_planes(self, gg, kind):
        """the expected counters from the oracle's TraceItem lists: (planes, entries) uint32"""
        oras = self.batch.oracle()
        if kind == "edges":
            return (em.of(oras, gg.bp, self.batch.slots).plane() * self.times).astype(np.uint32).reshape(1, -1)
        model = pm.of(oras, gg.bp)
        planes = np.zeros((8, gg.bp), dtype=np.int64)
        for key in model.nodes:
            first, length = gg.node_columns(2 * key[0] + (1 if key[1] else 0))
            planes[:, first:first + length] = model.node(key, length)
        planes *= self.times
        return (pm.depth_of(planes) if kind == "depth" else planes).astype(np.uint32)

    def want(self, planes, kind, fold, **q):
        return sm.sites(planes, kind, fold=fold, node_start=self.node_start, twin=self.twin, forward=self.forward, mirror=self.mirror, **q)

    def both_strands(self, planes, kind, entries):
        return sm.both_strands(planes, kind, entries, self.node_start, self.twin, self.mirror)


_CASES = {}


def _revcomp(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def case(name):
    if name in _CASES:
        return _CASES[name]
    if name.startswith("round edges"):
        # (every read of 321 bases once more as its reverse complement, seeded where synth.simulate_reads seeds a read of the other strand:
        # at the node that starts with the read's first base complemented, backbone position 320 -- its items lie on the reverse copies)
        g, reads, seeds = oc.round_edge_batch(int(name.split()[-1]))
        other = [_revcomp(r) for r in reads if len(r) == 321]
        reads, seeds = reads + other, seeds + [(int(g.node_at[320]), 0, True)] * len(other)
        c = SiteCase(name, ("bases", "depth"), g.nodes, g.edges, reads, seeds, 35)
    elif name == "indels":
        # (every read once more as the reverse complement of its part up to backbone position 384, the first base of node 7, which an
        # insertion read reaches 5 rows later and a deletion read 5 rows earlier: its items lie on the reverse copies)
        nodes, edges, reads, seeds = plc.indel_batch()
        other = [_revcomp(r[:385 + (5 if k % 2 == 0 else -5)]) for k, r in enumerate(reads)]
        reads, seeds = reads + other, seeds + [(7, 0, True)] * len(other)
        c = SiteCase(name, ("bases",), nodes, edges, reads, seeds, 35)
    elif name in ("one part and strands", "added twice"):
        g, reads, seeds = plc.one_part_and_strands_batch()
        c = SiteCase(name, ("bases", "depth", "edges") if name == "one part and strands" else ("bases", "edges"), g.nodes, g.edges, reads, seeds, 35,
                     times=2 if name == "added twice" else 1)
    elif name == "crossings":
        g, batches = oc.random_graph_batches((8, 15, 60, 0), mid_only=False)
        reads, seeds, bw, _ = batches[1]                        # (seeds in the middle: both strands)
        c = SiteCase(name, ("bases", "edges"), g.nodes, g.edges, reads, seeds, bw)
    elif name == "fan":
        # (its four reads lie on the forward strand; two more of the other strand: the reverse complement of head, stem, last branch
        # and the first base of that branch's tail, seeded at the tail's node as synth.simulate_reads seeds a read of the other strand)
        g, reads, seeds = plc.fan_batch()
        rng = np.random.default_rng(78)
        body = np.concatenate([g.head, g.stem, g.branches[9], g.tails[9][:1]])
        for noisy in (False, True):
            r = synth.add_errors(synth.revcomp_bytes(body), 0.03, 0.03, 0.03, rng) if noisy else synth.revcomp_bytes(body)
            reads, seeds = reads + [r.tobytes().decode()], seeds + [(3 + 10 + 9, 0, True)]
        c = SiteCase(name, ("edges", "depth"), g.nodes, g.edges, reads, seeds, 35)
    elif name == "gfa overlap":
        b = ec.batch_case("gfa overlap")
        c = SiteCase(name, ("bases", "depth"), b.nodes, b.edges, b.reads, b.seeds, b.bw, gfa=b.gfa, oracle=b._oracle, folds=False)
    else:
        raise KeyError(name)
    _CASES[name] = c
    return c


def run_case(c, gg):
    """the batch run and added (`times` times) to one pileup of every kind of the case -> {kind: pileup}"""
    piles = {k: gg.pileup(k) for k in c.kinds}
    devs, b = ec.run_add(gg, c.batch.reads, c.batch.seeds, c.batch.bw, list(piles.values()))
    for _ in range(c.times - 1):
        for p in piles.values():
            p.add(b)
    return piles


def compare(c, pile, kind, planes):
    """every query of QUERIES, folded and unfolded, against site_model over `planes`; returns {(fold, query index): entries}"""
    out = {}
    for fold in (True, False):
        for k, q in enumerate(QUERIES):
            if fold and not c.folds and kind != "edges":
                try:
                    pile.sites(fold=True, **q)
                except RuntimeError as e:
                    assert "(100)" in str(e), (c.name, kind)
                else:
                    raise AssertionError((c.name, kind, "fold over a graph with an overlap was not refused"))
                continue
            want_e, want_F = c.want(planes, kind, fold, **q)
            got = pile.sites(fold=fold, **q)
            assert got.total == len(want_e) == len(got), (c.name, kind, fold, q, got.total, len(want_e))
            assert np.array_equal(got["entry"].astype(np.int64), want_e), (c.name, kind, fold, q)
            assert np.array_equal(got["counts"], want_F), (c.name, kind, fold, q)
            out[(fold, k)] = want_e
    return out


def vacuity(c, gg, planes_of):
    """what keeps a case from passing on empty or one-sided results, from `planes_of(kind)`: every kind has a site; every fold case has
    a site to which both strands contribute.  Returns the number of sites of query 1 and of query 2 over the kinds with alleles"""
    n1 = n2 = 0
    for kind in c.kinds:
        planes = planes_of(kind)
        fold = c.folds or kind == "edges"
        e, _ = c.want(planes, kind, fold, **QUERIES[0])
        assert len(e) > 0, (c.name, kind, "no site")
        if fold:
            assert c.both_strands(planes, kind, e).any(), (c.name, kind, "no site with both strands")
        if kind == "bases":
            n1 += len(c.want(planes, kind, fold, **QUERIES[1])[0])
            n2 += len(c.want(planes, kind, fold, **QUERIES[2])[0])
    return n1, n2
