"""Names for what a -B ramp redo met, read off the oracle's slice records (oracle_binding.OracleGraph.align(..., record=True)
["slice_records"]) and nothing else.  Pure Python; the fields used are direction, j, bandwidth, sparse, end, end_exists, written,
min_score and len(end) as the slice's cell count (DPSlice::numCells); for CK also len(nodes).

The oracle records every slice its first pass computes, in the order it computes them, kept or not.  Within one direction a record
whose j is not greater than its predecessor's j is the first slice after a redo: the predecessor is the slice that turned the HMM
"wrong" and was thrown away, and the slice the redo came back to (its landing slice, `rampSlice` of getSqrtSlices,
GraphAligner.h:2648-2719) is the latest earlier record with j - 64 -- none when the redo returns to the seed.  From there this
module replays the bookkeeping that needs no score: which slices are still kept, where rampUntil stands, and the backtrace-override
windows (a run of kept slices of >= 200 000 cells after one of fewer, :2721-2764).

  L1   the redo lands on a sparse-method slice that has columns with written != 0 and end_exists == 0 (touched, their last row not
       confirmed) and the slice computed next is a bit-vector slice
  L1b  L1, and at least one such column has end <= min_score + bandwidth of that next slice: it can enter the next band
  L2   the redo lands on a sparse-method slice and the slice computed next is sparse again
  W1   a redo while a window is open, landing before the window's pre-slice: the window is dropped (:2676)
  W2   a redo that lands before the end of a closed window, which is popped (:2701)
  W3   a redo that lands inside the open window: the reference does not terminate (:2690-2694), reported as an assertion
  CK   (with the direction's slice count given) after the pass, the checkpoint list holds a sparse-method record that is no longer
       the slice kept at its j: `store` is not rewound by a redo (:2772-2786), so the traceback's recompute (:2858-2943) would start
       from a sparse slice the first pass has since replaced
  U1   a slice run at the ramp width with rampUntil == slice has >= 200 000 cells, so rampUntil moves on (:2626-2629) and the slice
       computed next is still at the ramp width

j is compared as the reference compares it, unsigned: the seed slice's -64 is the largest value there is, so a redo that returns
to the seed is "after" every window."""
W = 64
CUTOFF = 200000
SEED_J = (1 << 64) - W          # (size_t)-64

EVENTS = ("L1", "L1b", "L2", "W1", "W2", "W3", "U1", "CK")


def cells(rec):
    return len(rec["end"])


def partial_columns(rec):
    """indices of the columns that were touched and whose last row is not confirmed"""
    return [c for c, (w, e) in enumerate(zip(rec["written"], rec["end_exists"])) if w != 0 and e == 0]


def memory(rec):
    """DPSlice::estimatedMemory (:136-139)"""
    return cells(rec) * 4 + len(rec["nodes"]) * 28


def classify_direction(recs, ramp, n_slices=None):
    """recs: the records of ONE direction in the order computed; ramp: the ramp bandwidth of the run (0: none); n_slices: the slices
    of this direction (its padded length / 64), needed only for CK
    -> {"redos": [...], "events": set of names, "u1": [record index, ...], "ck": [record index, ...]}; one entry per redo:
       dict(at=index of the first record after the redo, landing=index of the landing record or None, events=set)"""
    redos, u1 = [], []
    # the checkpoint list (DPTable::slices, :2772-2786): record indices, None for the seed; `store` is not rewound by a redo
    sampling = 0
    while n_slices is not None and (sampling + 1) * (sampling + 1) <= n_slices:
        sampling += 1
    table, store, store_mem = [], None, 28
    rec_j = lambda k: SEED_J if k is None else recs[k]["j"]
    kept = []                    # indices of the records still kept, by ascending j
    ramp_until = 0
    # window bookkeeping: `last_cells` / `last_j` describe `last` of getSqrtSlices
    overriding = False
    pre_j = SEED_J
    temps = []                   # j of the open window's slices
    closed = []                  # (startj, endj) of the closed windows
    i = 0
    n = len(recs)
    while i < n:
        r = recs[i]
        s = r["j"] // W
        if ramp_until == s and cells(r) >= CUTOFF:
            ramp_until += 1
            if ramp > 0 and r["bandwidth"] == ramp and i + 1 < n and recs[i + 1]["j"] == r["j"] + W and recs[i + 1]["bandwidth"] == ramp:
                u1.append(i)
        if i + 1 < n and recs[i + 1]["j"] <= r["j"]:
            # ---- r turned the HMM wrong: it is thrown away and the pass goes back ----
            nxt = recs[i + 1]
            ramp_until = s
            land_j = nxt["j"] - W
            landing = None
            for k in range(i - 1, -1, -1):
                if recs[k]["j"] == land_j:
                    landing = k
                    break
            kept = [k for k in kept if recs[k]["j"] <= land_j]
            while len(table) > 1 and rec_j(table[-1]) > (SEED_J if landing is None else land_j):
                table.pop()
            lj = SEED_J if landing is None else recs[landing]["j"]
            ev = set()
            if landing is not None and recs[landing]["sparse"]:
                if nxt["sparse"]:
                    ev.add("L2")
                else:
                    part = partial_columns(recs[landing])
                    if part:
                        ev.add("L1")
                        bound = nxt["min_score"] + nxt["bandwidth"]
                        if any(recs[landing]["end"][c] <= bound for c in part):
                            ev.add("L1b")
            if overriding:
                if pre_j > lj:
                    ev.add("W1")
                    overriding = False
                    temps = []
                elif temps and temps[-1] > lj:
                    ev.add("W3")
            if closed and closed[-1][1] > lj:
                ev.add("W2")
                while closed and closed[-1][1] > lj:
                    closed.pop()
            redos.append(dict(at=i + 1, landing=landing, events=ev))
            if "W3" in ev:
                break                # the run ends in the assertion
            i += 1
            continue
        # ---- r is kept (or is the last record of a pass that stopped on it, which changes nothing below) ----
        last_cells = cells(recs[kept[-1]]) if kept else 0
        last_j = recs[kept[-1]]["j"] if kept else SEED_J
        if not overriding and cells(r) >= CUTOFF and last_cells < CUTOFF:
            pre_j = last_j
            overriding = True
            temps = [r["j"]]
        elif overriding:
            if cells(r) < CUTOFF:
                closed.append((temps[0], temps[-1]))
                while table and temps[0] <= rec_j(table[-1]) <= temps[-1]:
                    table.pop()
                table.append(kept[-1] if kept else None)
                store, store_mem = i, memory(r)
                overriding = False
                temps = []
            else:
                temps.append(r["j"])
        if sampling and s % sampling == 0 and (not table or rec_j(store) != rec_j(table[-1])):
            table.append(store)
            store, store_mem = i, memory(r)
        if memory(r) < store_mem:
            store, store_mem = i, memory(r)
        kept.append(i)
        i += 1
    # CK: a checkpoint that is a sparse-method record and no longer the slice kept at its j (taken before a redo went back past it)
    ck = [k for k in table if k is not None and k not in kept and recs[k]["sparse"]] if sampling else []
    events = set()
    for d in redos:
        events |= d["events"]
    if u1:
        events.add("U1")
    if ck:
        events.add("CK")
    return dict(redos=redos, events=events, u1=u1, ck=ck)


def classify(slice_records, ramp, n_slices=None):
    """n_slices: {direction: slices}, for CK.  All directions of one read -> dict(events=set, n_redos, n_sparse_landings, n_partial=[partial columns per L1 landing],
    directions={direction: classify_direction(...)})"""
    by_dir = {}
    for r in slice_records:
        by_dir.setdefault(r["direction"], []).append(r)
    out = dict(events=set(), n_redos=0, n_sparse_landings=0, n_partial=[], directions={})
    for d, recs in by_dir.items():
        c = classify_direction(recs, ramp, (n_slices or {}).get(d))
        out["directions"][d] = c
        out["events"] |= c["events"]
        out["n_redos"] += len(c["redos"])
        for redo in c["redos"]:
            if redo["landing"] is not None and recs[redo["landing"]]["sparse"]:
                out["n_sparse_landings"] += 1
                if "L1" in redo["events"]:
                    out["n_partial"].append(len(partial_columns(recs[redo["landing"]])))
    return out
