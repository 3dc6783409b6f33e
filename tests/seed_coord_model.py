"""The topology coordinate in plain Python (include/graphaligner_amd.h, "topology coordinate"): lists and Python
integers, one sequential walk up the parents per node.  Written from the text of the rule; it shares no code with
graphaligner_amd/csrc/ga_seed.h and is what the tests compare ga_graph_set_seed_coordinate with, node for node.  `with_topology` puts
the coordinate into a seed model (seed_model.Model or seed_walk_model.WalkModel), whose lookup and ranking do not change."""

GAP = 1 << 20


def in_lists_of(nodes, edges, given=None):
    """(n_nodes, lens, in_lists) by node index as the library numbers them: 0 and the last index are the dummy nodes, bigraph node
    number i is 1 + 2i (forward) and 2 + 2i (reverse).  A bigraph edge is two digraph edges (right end of `from` -> right end of `to`,
    and the mirrored one); a node's in-list holds its in-neighbours in the order the edges were added, each once.  `given`: {digraph
    id: [digraph ids]} of nodes whose in-list was handed over as it is (ga_graph_set_neighbors)."""
    n_nodes = 2 * len(nodes) + 2
    lens = [0] * n_nodes
    lens[0] = lens[-1] = 1
    index_of = {}
    for i, (nid, seq) in enumerate(nodes):
        index_of[2 * nid], index_of[2 * nid + 1] = 1 + 2 * i, 2 + 2 * i
        lens[1 + 2 * i] = lens[2 + 2 * i] = len(seq)
    ins = [[] for _ in range(n_nodes)]
    for f, f_rev, t, t_rev in edges:
        for a, b in ((2 * f + int(bool(f_rev)), 2 * t + int(bool(t_rev))), (2 * t + 1 - int(bool(t_rev)), 2 * f + 1 - int(bool(f_rev)))):
            a, b = index_of[a], index_of[b]
            if a not in ins[b]:
                ins[b].append(a)
    for did, lst in (given or {}).items():
        ins[index_of[did]] = [index_of[d] for d in lst]
    return n_nodes, lens, ins


def ceil_log2(x):
    r = 0
    while (1 << r) < x:
        r += 1
    return r


def topology(n_nodes, lens, ins):
    """(lin by node index, stats, parent by node index after the cuts: None for a root and for the dummy nodes)"""
    dummy = (0, n_nodes - 1)
    parent = [None] * n_nodes
    for v in range(n_nodes):
        if v in dummy:
            continue
        for u in ins[v]:
            if u != v and u not in dummy:
                parent[v] = u
                break
    # cycles: walk up from every node; a walk that meets its own trail has found one
    state = [0] * n_nodes                     # 0 new, 1 on the current trail, 2 done
    cycles = []
    for s in range(n_nodes):
        trail, v = [], s
        while v is not None and state[v] == 0:
            state[v] = 1
            trail.append(v)
            v = parent[v]
        if v is not None and state[v] == 1:
            cycles.append(trail[trail.index(v):])
        for t in trail:
            state[t] = 2
    for c in cycles:
        parent[min(c)] = None
    depth, hops, root = [None] * n_nodes, [0] * n_nodes, [None] * n_nodes
    for s in range(n_nodes):
        trail, v = [], s
        while depth[v] is None and parent[v] is not None:
            trail.append(v)
            v = parent[v]
        if depth[v] is None:
            depth[v], hops[v], root[v] = 0, 0, v
        for t in reversed(trail):
            p = parent[t]
            depth[t], hops[t], root[t] = depth[p] + lens[p], hops[p] + 1, root[p]
    real = [v for v in range(n_nodes) if v not in dummy]
    extent = {}
    for v in real:
        extent[root[v]] = max(extent.get(root[v], 0), depth[v] + lens[v])
    base, run = {}, 0
    for r in sorted(extent):
        base[r] = run
        run += extent[r] + GAP
    lin = [0] * n_nodes
    for v in real:
        lin[v] = base[root[v]] + depth[v]
    longest = max([hops[v] for v in real], default=0)
    stats = dict(kind=1, trees=len(extent), cycles_cut=len(cycles), extent_sum=sum(extent.values()),
                 # doubling rounds: with a cycle the first pass runs to its bound; else until 2^r parent steps leave the longest chain
                 cycle_rounds=ceil_log2(n_nodes) if cycles else ceil_log2(longest + 1),
                 depth_rounds=0 if longest == 0 else ceil_log2(longest) + 1)
    return lin, stats, parent


def of_graph(nodes, edges, given=None):
    n_nodes, lens, ins = in_lists_of(nodes, edges, given)
    return topology(n_nodes, lens, ins) + (lens,)


def with_topology(model, nodes, edges):
    """the seed model with its lin replaced by the topology coordinate of (nodes, edges); returns (model, lin, stats)"""
    lin, stats, _, _ = of_graph(nodes, edges)
    model.lin = {index: lin[index] for index in model.lin}
    return model, lin, stats
