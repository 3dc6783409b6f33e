"""Writes the fabricated streams of tests/test_pathseq.py with the bytes pathseq_model.replay expects into one text file, for
tests/emul/pathseq_stream_check.cpp: a stand-alone program (a main of its own, so it can be built with -fsanitize=address,undefined and
run as it is) that puts the same streams through the host build of the path-sequence program.

    python tests/pathseq_stream_dump.py OUT.txt

Lines: `P n_nodes node_len start_row trace_rows backward n_moves moves-as-hex expected-bases` (`-` for none)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import pathseq_model as psm                 # noqa: E402
import test_pathseq as tp                   # noqa: E402


def main(path):
    streams = bases = 0
    with open(path, "w") as f:
        for _, moves, n_nodes, node_len, start_row, trace_rows, backward in tp.streams():
            want = psm.replay(moves, n_nodes, node_len, start_row, trace_rows, backward)
            f.write("P %d %d %d %d %d %d %s %s\n" % (n_nodes, node_len, start_row, trace_rows, int(backward), len(moves), bytes(moves).hex() or "-", want.decode() or "-"))
            streams += 1
            bases += len(want)
    print("%d streams, %d bases expected" % (streams, bases))


if __name__ == "__main__":
    main(sys.argv[1])
