"""Cases for the ladder's pass with 4 096 band nodes (bit-vector bands of more than 256 nodes), shared by tests/test_wide_bands.py
(host emulation, tests/emul) and tests/test_wide_bands_gpu.py (the product library).

The graphs are fans (synth.FanGraph) of many SHORT branches: when an alignment nears the stem's end the projected band holds the
stem, every branch and, a little later, every tail -- hundreds to thousands of nodes, but fewer than 200 000 cells, so the reference
aligns them with its ordinary bit-vector path.  Every case is compared with the oracle, every field; the oracle must report status 0
and no sparse slice for every read, so that a case cannot quietly turn into a sparse one."""
import functools

import numpy as np

from graphaligner_amd import synth
import parity_common as pc


HEAD_LEN, STEM_LEN, READ_LEN = 300, 600, 1400

# name -> (branches, branch_len, shared, tail_len, band, ramp, cyclic); band nodes = 2 * branches + 2 at the widest slice
CASES = {
    "300x64": (300, 64, 16, 64, 35, 0, False),
    "300x24-long-tails": (300, 24, 8, 300, 35, 0, False),
    "600x16": (600, 16, 8, 300, 35, 0, False),           # crosses the growth to 1 109 buckets
    "1200x16-ramp": (1200, 16, 8, 60, 20, 45, False),    # a ramp redo with 2 402 nodes
    "2000x12": (2000, 12, 6, 40, 35, 0, False),          # 4 002 nodes: near the limit, 5 087 buckets
    "cyclic-300x24": (300, 24, 8, 60, 35, 0, True),      # an extra edge tail k -> branch (k + 1) mod n for every k
    "cyclic-700x16-ramp": (700, 16, 8, 60, 35, 50, True),
}
LIMIT = (4200, 8, 4, 8, 35, 0, False)                    # 8 402 nodes: more than the widest tables hold


@functools.lru_cache(maxsize=None)
def fan_batch(branches, branch_len, shared, tail_len, cyclic):
    """(nodes, edges, reads, seeds) of one fan, built once per process and left unchanged: three reads of up to 1 400 bases through
    head, stem, one branch and its tail (3 % substitutions, insertions and deletions), seeded at the head's first base; where the tails
    are long enough (>= 200) one more read seeded 10 bases into a tail, with the rest of the tail (>= 193 bases) behind the seed: its
    backward part meets the fan from the other strand, as a many-to-one join."""
    g = synth.FanGraph(head_len=HEAD_LEN, stem_len=STEM_LEN, n_branches=branches, branch_len=branch_len, shared=shared, tail_len=tail_len, seed=branches)
    nodes, edges = list(g.nodes), list(g.edges)
    if cyclic:
        edges += [(3 + branches + k, False, 3 + (k + 1) % branches, False) for k in range(branches)]
    rng = np.random.default_rng(branches * 11 + branch_len)
    noisy = lambda a: synth.add_errors(a, 0.03, 0.03, 0.03, rng).tobytes().decode()
    reads, seeds = [], []
    for _ in range(3):
        b = int(rng.integers(0, branches))
        reads.append(noisy(np.concatenate([g.head, g.stem, g.branches[b], g.tails[b]])[:READ_LEN]))
        seeds.append((1, 0, False))
    if tail_len >= 200:
        # (a branch among the first 60: on the other strand the stem has every branch as an in-neighbour, and a traceback move into
        # an in-neighbour whose ordinal is above 62 is a capacity miss of every kernel variant -- a limit the library had before
        # this pass and keeps, see GA_S_CAPACITY in include/graphaligner_amd.h)
        b = int(rng.integers(0, 60))
        pre = noisy(np.concatenate([g.head, g.stem, g.branches[b], g.tails[b][:10]]))
        post = noisy(g.tails[b][10:])
        assert len(g.tails[b]) - 10 >= 193
        reads.append(pre + post)
        seeds.append((3 + branches + b, len(pre), False))
    return nodes, edges, reads, seeds


def check_case(case, lib_path=None, trace=True, ctx=""):
    """one case against the oracle: every field of every read; the oracle aligned every read without a sparse slice"""
    branches, branch_len, shared, tail_len, bw, ramp, cyclic = case
    nodes, edges, reads, seeds = fan_batch(branches, branch_len, shared, tail_len, cyclic)
    devs, oras = pc.check_parity(nodes, edges, reads, seeds, bw, ramp=ramp, lib_path=lib_path, trace=trace,
                                 ctx="%s fan %d x %d bw %d/%d%s" % (ctx, branches, branch_len, bw, ramp, " cyclic" if cyclic else ""))
    assert all(o["status"] == 0 and o["sparse_slices"] == 0 for o in oras), [(o["status"], o["sparse_slices"]) for o in oras]
    assert all(d["status"] == 0 for d in devs)
    # the three reads through the fan were finished by a later pass than the first
    assert all(d["kernel_pass"] > 0 for d in devs[:3]), [d["kernel_pass"] for d in devs]
    return devs, oras


def check_limit(lib_path=None):
    """more band nodes than the widest tables hold: the oracle aligns, the library says GA_S_CAPACITY for each read and nothing worse"""
    branches, branch_len, shared, tail_len, bw, ramp, cyclic = LIMIT
    nodes, edges, reads, seeds = fan_batch(branches, branch_len, shared, tail_len, cyclic)
    devs, oras = pc.run_both(nodes, edges, reads, seeds, bw, ramp=ramp, lib_path=lib_path)
    assert all(o["status"] == 0 and o["sparse_slices"] == 0 for o in oras), [(o["status"], o["sparse_slices"]) for o in oras]
    assert [d["status"] for d in devs] == [10] * len(reads), [d["status"] for d in devs]
    assert all(d["failed"] for d in devs)
    return devs, oras


@functools.lru_cache(maxsize=None)
def mixed_batch():
    """(nodes, edges, reads, seeds, which reads are fan reads), built once per process and left unchanged: the fan of the first case
    and a chain of 64-bp nodes as two components of one graph; 60 ordinary reads on the chain and 4 reads through the fan, shuffled"""
    branches, branch_len, shared, tail_len = CASES["300x64"][:4]
    fan = synth.FanGraph(head_len=HEAD_LEN, stem_len=STEM_LEN, n_branches=branches, branch_len=branch_len, shared=shared, tail_len=tail_len, seed=branches)
    chain = synth.SynthGraph(synth.random_genome(60000, 91), node_len=64, first_id=2 * branches + 3)
    nodes, edges = list(fan.nodes) + list(chain.nodes), list(fan.edges) + list(chain.edges)
    reads, seeds = synth.simulate_reads(chain, 60, 1000, seed=92)
    rng = np.random.default_rng(93)
    is_fan = [False] * len(reads)
    for _ in range(4):
        b = int(rng.integers(0, branches))
        reads.append(synth.add_errors(np.concatenate([fan.head, fan.stem, fan.branches[b], fan.tails[b]])[:READ_LEN], 0.03, 0.03, 0.03, rng).tobytes().decode())
        seeds.append((1, 0, False))
        is_fan.append(True)
    order = rng.permutation(len(reads))
    return nodes, edges, [reads[i] for i in order], [seeds[i] for i in order], [is_fan[i] for i in order]
