"""The job plan of a batch, stated on its own: what getSplitAlignment (GraphAligner.h:2969-3024) does with a read and its seed hits
before any cell is computed, and which rows of the two traces count (:3051-3055, 3069-3073).  Plain Python over digraph ids; it
shares no code with graphaligner_amd/csrc/ga_plan.h or with ga_batch_prepare.

A graph is given as the list of its digraph nodes in node-index order, index 1 first: [(digraph id, length)].  Seeds are what
Graph.find_seeds returns per read: (bigraph node id, read position, reverse)."""

OK, ASSERTION, BAD_SEED = 0, 1, 3
WORD = 64
# CommonUtils.cpp:60-136: the characters ReverseComplement knows, either case; anything else asserts
HAS_COMPLEMENT = set("ACTGNURYKMSWBVD") | set("ACTGNURYKMSWBVD".lower())


def bigraph_nodes(nodes):
    """the digraph nodes of a graph built from bigraph nodes alone (BigraphToDigraph.cpp:27-56): forward 2 * id, reverse 2 * id + 1"""
    out = []
    for nid, seq in nodes:
        out += [(2 * nid, len(seq)), (2 * nid + 1, len(seq))]
    return out


def padded(n):
    return (n + WORD - 1) // WORD * WORD


def plan(dnodes, overlap, reads, seeds):
    """dict(jobs=[(rows_off, n_rows, seed_node, trace_rows)], seeds=[(pos, seedNodeIndex, early, valid, bwJob, fwJob)],
    fills=[(read, off, n, padded, pos, backward)]) of the batch"""
    index_of = {}
    length = {}
    for k, (did, ln) in enumerate(dnodes):
        index_of.setdefault(did, k + 1)
        length[k + 1] = ln
    jobs, plans, fills = [], [], []
    rows = 0
    for i, (seq, hits) in enumerate(zip(reads, seeds)):
        size = len(seq)
        for node_id, pos, reverse in hits:
            plain, flipped = index_of.get(node_id * 2), index_of.get(node_id * 2 + 1)
            if plain is None or flipped is None:                        # nodeLookup.at throws (:423)
                plans.append((pos, 0, BAD_SEED, 0, -1, -1))
                continue
            if not pos < size:
                plans.append((pos, plain, ASSERTION, 0, -1, -1))
                continue
            forward, backward = (flipped, plain) if reverse else (plain, flipped)
            if length[forward] != length[backward]:
                plans.append((pos, plain, ASSERTION, 0, -1, -1))
                continue
            bw_job = fw_job = -1
            if pos > 0:
                part = seq[:pos + overlap]
                if size < pos + overlap or any(c not in HAS_COMPLEMENT for c in part):
                    plans.append((pos, plain, ASSERTION, 0, -1, -1))
                    continue
                n = len(part)
                bw_job = len(jobs)
                jobs.append((rows, padded(n), backward, pos))              # the trace's rows below the seed count (:3069-3073)
                fills.append((i, rows, n, padded(n), 0, 1))
                rows += padded(n)
            if pos < size - 1:
                n = size - pos
                fw_job = len(jobs)
                jobs.append((rows, padded(n), forward, n - overlap if n >= overlap else 0))     # (:3051-3055)
                fills.append((i, rows, n, padded(n), pos, 0))
                rows += padded(n)
            plans.append((pos, plain, OK, 1, bw_job, fw_job))
    return dict(jobs=jobs, seeds=plans, fills=fills)
