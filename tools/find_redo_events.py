#!/usr/bin/env python3
"""Search for reads whose -B ramp redo lands on a sparse-method slice or meets a backtrace-override window (the events of
tests/redo_events.py), with the CPU oracle alone.  Prints one JSON line per read that shows an event: the FanGraph parameters,
the rng seed, the draw index, the read's length and error rate (tests/redo_sparse_cases.build_read rebuilds the read from these),
the events, and how the oracle's run ended.  tests/redo_sparse_cases.py holds the descriptions chosen from this output.

Draw number d of a fan gets length 1300 + 64 * (d % 8) and error rate (0.11, 0.13, 0.15, 0.17)[(d // 8) % 4] (uniform noise: a
burst of errors confined to the shared stretch produced no redo at all), and a generator seeded with (seed, d).

The bound of the search is --draws per fan (default 400: 2 000 reads over the five fans, a few minutes of CPU on 8 processes).  An
event not seen within it is reported as not found in the summary line; DESIGN.md section 5 names the bound that was run."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

_OG = {}


def one(task):
    fan, seed, draw, err_override = task
    import oracle_binding as ob
    import redo_events as ev
    import redo_sparse_cases as rc
    fan = tuple(fan)
    g = rc.fan_graph(fan)
    if fan not in _OG:
        _OG[fan] = ob.OracleGraph(g.nodes, g.edges)
    length, err = rc.draw_shape(draw)
    if err_override is not None:
        err = err_override
    read, sd = rc.build_read(fan, seed, draw, length, err)
    o = _OG[fan].align(read, [sd], fan[4], fan[5], record=True)
    c = ev.classify(o["slice_records"], fan[5], {0: (len(read) + 63) // 64})
    return dict(fan=list(fan), seed=seed, draw=draw, length=length, err=err, events=sorted(c["events"]), redos=c["n_redos"], sparse_landings=c["n_sparse_landings"],
                partial=c["n_partial"], status=o["status"], failed=o["failed"], message=o["message"][:60], sparse_slices=o["sparse_slices"], windows=o["override_windows"])


def main(argv=None):
    import redo_sparse_cases as rc
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=400, help="reads per fan: the bound of the search")
    ap.add_argument("--first", type=int, default=0, help="first draw index")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--fans", type=int, nargs="*", default=None, help="indices into redo_sparse_cases.FANS (default: all)")
    ap.add_argument("--fan", type=int, nargs=6, action="append", default=None, metavar=("B", "BL", "SH", "STEM", "BW", "RAMP"), help="a fan of your own")
    ap.add_argument("--err", type=float, default=None, help="one error rate for every draw instead of the four of the list")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--all", action="store_true", help="print every read, not only those with an event")
    args = ap.parse_args(argv)
    fans = [tuple(f) for f in args.fan] if args.fan else [rc.FANS[i] for i in (args.fans if args.fans is not None else range(len(rc.FANS)))]
    tasks = [(fan, args.seed, d, args.err) for fan in fans for d in range(args.first, args.first + args.draws)]
    import multiprocessing as mp
    t0 = time.time()
    counts, n_redos, n_landings = {}, 0, 0
    with mp.Pool(args.jobs) as pool:
        for r in pool.imap(one, tasks, chunksize=4):
            n_redos += r["redos"]
            n_landings += r["sparse_landings"]
            for e in r["events"]:
                counts[e] = counts.get(e, 0) + 1
            if r["events"] or args.all:
                print(json.dumps(r), flush=True)
    import redo_events as ev
    print(json.dumps(dict(summary=True, reads=len(tasks), draws_per_fan=args.draws, first=args.first, seed=args.seed, err=args.err, fans=[list(f) for f in fans], redos=n_redos, sparse_landings=n_landings,
                          reads_with=counts, not_found=[e for e in ev.EVENTS if e not in counts], seconds=round(time.time() - t0, 1))))


if __name__ == "__main__":
    main()
