"""Writes what tests/test_edge_pileup.py runs -- its graphs with their slot tables, its fabricated graphs with their mirror-slot tables,
and every fabricated stream with the counts edge_stream_model.replay expects -- into one text file, for tests/emul/edges_stream_check.cpp:
a stand-alone program (a main of its own, so it can be built with -fsanitize=address,undefined and run as it is) that puts the same
inputs through the host library's slot entry points and through the host build of the edge-support program.

    python tests/edge_stream_dump.py OUT.txt

Lines: `G nodes edges slots` + `N id sequence` + `E from from_start to to_end` + `S from to`; `X nodes` + five lines (node lengths,
in-list offsets, in-neighbours, twins, expected mirror slots); `C graph start_node start_offset start_row trace_rows backward n_moves
moves-as-hex items nonzero (slot count)...`."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import edge_cases as ec                     # noqa: E402
import edge_model as em                     # noqa: E402
import edge_stream_model as esm             # noqa: E402
import ops_model as om                      # noqa: E402
import test_edge_pileup as tp               # noqa: E402


def main(path):
    streams = items = 0
    with open(path, "w") as f:
        graphs = [(c.nodes, c.edges, c.slots) for c in ec.graph_cases().values() if c.gfa is None]
        nodes = [(1, "ACGTAC"), (2, "GGT"), (3, "TTACG"), (2, "AAAAAAA")]
        edges = [(1, False, 2, False), (2, False, 3, False), (1, False, 2, False), (1, False, 3, True), (3, True, 3, False), (2, False, 3, False)]
        graphs.append((nodes, edges, em.slot_table([n for n, _ in nodes], edges)))
        for nodes, edges, slots in graphs:
            f.write("G %d %d %d\n" % (len(nodes), len(edges), len(slots)))
            for nid, seq in nodes:
                f.write("N %d %s\n" % (nid, seq))
            for a, b, c, d in edges:
                f.write("E %d %d %d %d\n" % (a, int(bool(b)), c, int(bool(d))))
            for a, b in slots:
                f.write("S %d %d\n" % (a, b))
        index = {}
        for name, (graph, _, _, _) in tp.GRAPHS.items():
            index[name] = len(index)
            lens, off, nbr, twin = tp._arrays(graph)
            f.write("X %d\n" % len(lens))
            for arr in (lens, off, nbr[:int(off[-1])], twin, esm.mirror_slots(graph)):
                f.write(" ".join(str(int(x)) for x in arr) + "\n")
        for kind in tp.STREAM_KINDS:
            for name, (graph, start, choose, _) in tp.GRAPHS.items():
                for backward in (False, True):
                    rng = np.random.default_rng(len(kind) * 37 + len(name) + int(backward))
                    for n in tp.STREAM_LENGTHS:
                        moves = esm.route(tp._codes(kind, n, rng), graph, start, lambda node, deg: choose(node, deg, rng))
                        rows = sum(1 for m in moves if m & 3 != om.MOVE_LEFT)
                        for cut in (0, 1, 37, 64):
                            trace_rows = max(rows + 1 - cut, 0)
                            want, want_items = esm.replay(moves, graph, start, rows, trace_rows, backward)
                            nz = np.flatnonzero(want)
                            f.write("C %d %d %d %d %d %d %d %s %d %d %s\n" % (index[name], start[0], start[1], rows, trace_rows, int(backward), len(moves),
                                                                              bytes(moves).hex() or "-", want_items, len(nz),
                                                                              " ".join("%d %d" % (int(s), int(want[s])) for s in nz)))
                            streams += 1
                            items += want_items
    print("%d graphs, %d fabricated graphs, %d streams, %d crossings expected" % (len(graphs), len(index), streams, items))


if __name__ == "__main__":
    main(sys.argv[1])
