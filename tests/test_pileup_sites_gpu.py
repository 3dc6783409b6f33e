"""Site queries on the GPU: ga_pileup_sites_mark_kernel, the scan and ga_pileup_sites_write_kernel through the product library, on whole
batches (site_cases.py: the batches of pileup_cases.py and ops_cases.py).  For every case and kind the sites of three queries, folded and
unfolded, must equal site_model -- the rule in numpy -- applied to Pileup.counts() of the same pileup; in one case the planes come from
the oracle's TraceItem lists instead, so that the check does not lean on the download.  What keeps a case from passing on empty or
one-sided results is computed from the model (site_cases.vacuity; test_pileup_sites.py confirms the same from the oracle alone, without
a device).  Counts are integers: there is no tolerance.  On a library without the feature every test here fails at binding.GA_SITES_FOLD."""
import pytest

from graphaligner_amd import binding
import site_cases as sc

pytestmark = pytest.mark.gpu

assert binding.GA_SITES_FOLD == 1


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need a real MI355X"


@pytest.fixture(autouse=True, params=["GA_LANES=1", "GA_LANES=0"])
def _first_pass(request, monkeypatch):
    """both first passes: the lanes = reads kernel (its own traceback writes the moves), and the wave-per-read kernels over everything"""
    monkeypatch.delenv("GA_TEST_WAVE_SLOTS", raising=False)
    monkeypatch.setenv("GA_LANES", request.param[-1])


_FEWER = {}


@pytest.mark.parametrize("name", sc.NAMES)
def test_sites_of_a_batch(name):
    c = sc.case(name)
    gg = c.graph()
    piles = sc.run_case(c, gg)
    counts = {kind: piles[kind].counts() for kind in c.kinds}
    n1, n2 = sc.vacuity(c, gg, lambda kind: counts[kind])
    _FEWER[name] = n2 < n1
    for kind in c.kinds:
        pile = piles[kind]
        assert counts[kind].any()
        got = sc.compare(c, pile, kind, counts[kind])
        if c.folds or kind == "edges":
            assert len(got[(True, 0)]) > 0
        # the same bytes twice, a cap, and a range that starts and ends inside a round
        fold = c.folds or kind == "edges"
        a, b = pile.sites(fold=fold), pile.sites(fold=fold)
        assert a.tobytes() == b.tobytes() and a.total == b.total == len(a) > 0 and a.kernel_ms > 0 and a.entries_scanned == pile.entries
        cut = pile.sites(fold=fold, max_sites=max(1, len(a) - 1))
        assert cut.total == len(a) and cut.tobytes() == a[:max(1, len(a) - 1)].tobytes()
        first, n = int(a["entry"][0]) + 1, 70
        part = pile.sites(fold=fold, first=first, n=min(n, pile.entries - first))
        assert part.tobytes() == a[(a["entry"] >= first) & (a["entry"] < first + n)].tobytes()
        if kind == "edges":
            support = pile.edge_support()
            top = max(support.values())
            assert top >= 1
            for t in sorted({1, 2, top, top + 1}):
                assert pile.supported_edges(t) == {k: v for k, v in support.items() if v >= t}, (name, t)
    if name == "added twice":
        assert int(counts["bases"].max()) >= 2
    if name == "one part and strands":
        # the planes from the oracle's TraceItem lists: nothing of this check comes down through ga_pileup_download
        for kind in c.kinds:
            sc.compare(c, piles[kind], kind, c.model_planes(gg, kind))
    if name == "gfa overlap":
        # (edge slots fold through the mirror table and need no precondition)
        e = gg.pileup("edges")
        assert e.sites(fold=True).total == 0


def test_a_stricter_query_selects_fewer_sites_somewhere():
    """the (2, 1, 1/4) query has fewer sites than (1, 1) in at least one case: from the model over the counters of the cases run above,
    and over the oracle's planes where this test runs alone"""
    if not _FEWER:
        c = sc.case("one part and strands")
        gg = c.graph()
        n1, n2 = sc.vacuity(c, gg, lambda kind: c.model_planes(gg, kind))
        _FEWER[c.name] = n2 < n1
    assert any(_FEWER.values())


def test_refusals_and_fields():
    c = sc.case("round edges 64")
    gg = c.graph()
    pile = sc.run_case(c, gg)["bases"]
    for q in (dict(min_depth=0), dict(alt_frac=(0, 0)), dict(alt_frac=(1, 65536)), dict(alt_frac=(2, 1)), dict(first=pile.entries, n=1), dict(first=0, n=pile.entries + 1)):
        with pytest.raises(RuntimeError, match=r"\(100\)"):
            pile.sites(**q)
    assert pile.sites(first=pile.entries, n=0).total == 0
    got = pile.sites(fold=False)
    for s in got[:50]:
        first, length = gg.node_columns(2 * int(s["node_id"]) + int(s["reverse"]))
        assert first + int(s["offset"]) == int(s["entry"]) and int(s["offset"]) < length
        seq = dict(c.batch.nodes)[int(s["node_id"])]
        base = seq[int(s["offset"])] if not s["reverse"] else seq[::-1].translate(str.maketrans("ACGT", "TGCA"))[int(s["offset"])]
        assert s["graph_char"].decode() == base
    assert got["reverse"].any() and not got["reverse"].all()
    with pytest.raises(ValueError):
        pile.supported_edges(1)
