"""The pipelines with seeds=None over two ranks (gloo, host build of tests/emul): align_sharded and align_queued with
find_seeds=... gathered on rank 0 equal the same functions with the seeds passed in, for the three result forms."""
import os
import socket
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, lib, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["GA_HOST_THREADS"] = "2"
    import torch.distributed as dist
    from graphaligner_amd import binding, sharding, synth
    import seed_plan_common as spc
    dist.init_process_group("gloo", rank=rank, world_size=world)
    g = synth.bubble_graph(40000, node_len=32, seed=11)
    graph = binding.Graph(g.nodes, g.edges, lib_path=lib)
    graph.build_seed_index()
    reads = spc.mixed_reads(g, 20, length=700, seed=9)
    reads = [r[: 400 + (53 * i) % 300] if len(r) > 300 else r for i, r in enumerate(reads)]
    names = ["r%03d" % i for i in range(len(reads))]
    how = dict(params=dict(max_seeds=2), loci=True)
    seeds = graph.find_seeds(reads, loci=True, max_seeds=2).seeds
    got = [sharding.align_sharded(graph, reads, None, 35, dist=dist, find_seeds=how),
           sharding.align_queued(graph, reads, None, 35, dist=dist, chunk_reads=5, find_seeds=how),
           sharding.align_queued(graph, reads, None, 35, dist=dist, chunk_reads=5, summary=True, find_seeds=how),
           sharding.align_queued(graph, reads, None, 35, dist=dist, chunk_reads=5, gam=True, names=names, find_seeds=how)]
    want = [sharding.align_sharded(graph, reads, seeds, 35, dist=dist),
            sharding.align_queued(graph, reads, seeds, 35, dist=dist, chunk_reads=5),
            sharding.align_queued(graph, reads, seeds, 35, dist=dist, chunk_reads=5, summary=True),
            sharding.align_queued(graph, reads, seeds, 35, dist=dist, chunk_reads=5, gam=True, names=names)]
    if rank == 0:
        try:
            spc.same_results(got[0], want[0])
            spc.same_results(got[1], want[1])
            fields = ("status", "failed", "score", "n_mappings", "alignment_start", "alignment_end", "query_position", "column_updates")
            ok = all((got[2][f] == want[2][f]).all() for f in fields) and got[3] == want[3]
            q.put((ok, sum(1 for r in got[0] if r["status"] == 0 and not r["failed"]), sum(1 for s in seeds if not s), len(got[3])))
        except AssertionError as e:
            q.put((False, repr(e), 0, 0))
    else:
        assert all(x is None for x in got)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_without_seeds_equal_two_ranks_with_seeds():
    import torch.multiprocessing as mp
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import parity_common as pc
    lib = pc.emul_lib_path()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, lib, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=300)
        assert p.exitcode == 0
    ok, aligned, unseeded, gam_len = q.get(timeout=10)
    assert ok is True, aligned
    assert aligned >= 15 and unseeded >= 4 and gam_len > 5000
