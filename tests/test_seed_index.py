"""The k-mer index of the graph (ga_graph_build_seed_index / ga_graph_seed_index_copy) against the model of tests/seed_model.py,
entry for entry.  CPU: the seeding program of graphaligner_amd/csrc/ga_seed.h built for the host (tests/emul); tests/test_seed_gpu.py
repeats the comparison through the product library."""
import ctypes as C

import pytest

from graphaligner_amd import binding, synth
import parity_common as pc
import seed_common as sc

GRAPHS = {
    "linear": lambda: synth.linear_graph(12000),
    "bubbles32": lambda: synth.bubble_graph(12000, node_len=32, seed=3),
    "cyclic16": lambda: synth.cyclic_graph(3000, node_len=16),
    "short8": lambda: synth.SynthGraph(synth.random_genome(4000, 5), node_len=8, snp_every=40, seed=2),
}


def index_cases():
    for name in GRAPHS:
        for k in (11, 15, 31):
            for s in (0, 2, 5):
                if name == "short8" and k != 11:
                    continue
                yield name, k, s


@pytest.mark.parametrize("name,k,s", list(index_cases()))
def test_index_equals_the_model(name, k, s):
    g = GRAPHS[name]()
    _, st = sc.check_index(g.nodes, g.edges, k, s, pc.emul_lib_path())
    if name == "short8":
        # most nodes are shorter than k: few entries, no crash
        assert st["kmers_seen"] < 0.2 * 2 * sum(len(seq) for _, seq in g.nodes)


@pytest.mark.parametrize("k,s", [(k, s) for k in (11, 15, 31) for s in (0, 2, 5)])
def test_index_of_one_long_node(k, s):
    nodes, edges = sc.big_node_graph(100000)
    _, st = sc.check_index(nodes, edges, k, s, pc.emul_lib_path())
    assert st["kmers_seen"] == 2 * (100000 - k + 1)


def test_rebuild_replaces_the_index_and_bad_arguments_are_refused():
    lib = pc.emul_lib_path()
    L = binding.load(lib)
    g = synth.linear_graph(5000)
    G = binding.Graph(g.nodes, g.edges, lib_path=lib)
    st = binding.GaSeedIndexStats()
    assert L.ga_graph_seed_index_stats(G.h, C.byref(st)) == 100          # no index yet: GA_E_INVALID
    a = G.build_seed_index(k=15, sample_shift=2)
    b = G.build_seed_index(k=11, sample_shift=0)
    assert b["k"] == 11 and b["entries"] == b["kmers_seen"] > a["entries"]
    for k, s in ((10, 2), (32, 2), (15, 9)):
        assert L.ga_graph_build_seed_index(G.h, k, s) == 100
    # before finalize / upload
    h = L.ga_graph_create()
    assert L.ga_graph_add_bigraph_node(h, 1, b"ACGTACGTACGTACGTACGT", 20) == 0
    assert L.ga_graph_build_seed_index(h, 15, 2) == 103                   # GA_E_NOT_FINALIZED
    assert L.ga_graph_finalize(h, 0) == 0
    assert L.ga_graph_build_seed_index(h, 15, 2) == 101                   # GA_E_NO_DEVICE: not uploaded
    L.ga_graph_destroy(h)
    # the parameters of a lookup must be the index's
    with pytest.raises(RuntimeError):
        G.find_seeds(["ACGT" * 200], k=15)
