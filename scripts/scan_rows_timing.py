"""Times the scan side's ways to the pruned AddFile rows on config 3 (the 10M-file table bench.py
builds) under a partition predicate that keeps about 0.5 % of the live files, and prints one JSON line:

  (i)   whole-side way: fresh state -> dr_filter -> dr_state_export(DR_LIVE) -> index the columns on the host
  (ii)  walk path:      fresh state -> dr_filter -> dr_state_export_rows (first call, then a repeat: the
                        checkpoint-column decode of the first call is cached with the state)
  (iii) gather path:    the same two calls after dr_state_materialize

Every figure is a host clock around library calls that end in a stream synchronise, the median of
--reps fresh states after --warmup untimed ones. The selection's columns of (ii) and (iii) are checked
byte for byte against (i)'s before anything is reported.

  python scripts/scan_rows_timing.py [--scale 1.0] [--reps 5] [--warmup 1] [--workdir DIR]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def _ranges(off, idx):
    lens = off[idx + 1] - off[idx]
    new = np.zeros(len(idx) + 1, dtype=np.int64)
    np.cumsum(lens, out=new[1:])
    src = np.repeat(off[idx] - new[:-1], lens) + np.arange(int(new[-1]), dtype=np.int64)
    return new, src


def host_index(full, rows):
    """The whole export's columns at `rows` (what a host does with dr_state_export and a selection)."""
    out = {k: full[k][rows] for k in ("size", "modification_time", "deletion_timestamp", "deletion_timestamp_valid",
                                      "extended_file_metadata", "stats_null", "pv_null", "tags_null")}
    for s in ("path", "stats"):
        out[s + "_off"], src = _ranges(full[s + "_off"], rows)
        out[s + "_bytes"] = full[s + "_bytes"][src]
    for side in ("pv", "tags"):
        out[side + "_entry_off"], ent = _ranges(full[side + "_entry_off"], rows)
        out[side + "_val_null"] = full[side + "_val_null"][ent]
        for kv in ("key", "val"):
            out["%s_%s_off" % (side, kv)], src = _ranges(full["%s_%s_off" % (side, kv)], ent)
            out["%s_%s_bytes" % (side, kv)] = full["%s_%s_bytes" % (side, kv)][src]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workdir", default=os.environ.get("DR_BENCH_DIR", os.path.join(tempfile.gettempdir(), "dr_bench")))
    args = ap.parse_args()

    from bench import build_table
    from delta_amd import _native as N
    from delta_amd.delta_log import Engine, State
    from delta_amd.predicates import build_program, lower_program, partition_schema

    path = os.path.join(args.workdir, "c3_s%g" % args.scale)  # the table bench.py builds and caches
    exp = build_table(path, 3, args.scale)
    eng = Engine.get(0)
    lib = eng.lib
    staged = eng.stage_log(os.path.join(path, "_delta_log"))
    cutoff = exp["min_file_retention_timestamp"]
    pred = keepalive = None

    def fresh():
        return staged.replay(cutoff)

    def timed(f):
        t = time.perf_counter()
        r = f()
        return r, time.perf_counter() - t

    def do_filter(st):
        nonlocal pred, keepalive
        if pred is None:  # p1 is uniform over 0..999: p1 < 5 keeps about 0.5 % of the files
            meta = next(a["metaData"] for a in st.nonfile if "metaData" in a)
            pred, keepalive = lower_program(build_program(partition_schema(meta), [("<", ("col", "p1"), ("lit", "integer", 5))]))
        sel, n = C.POINTER(C.c_int64)(), C.c_int64()
        eng.check(lib.dr_filter(st.h, C.byref(pred), C.byref(sel), C.byref(n)))
        rows = np.ctypeslib.as_array(sel, shape=(max(n.value, 1),))[:n.value].copy()
        lib.dr_free(C.cast(sel, C.c_void_p))
        return rows

    def rows_call(st, rows, keep=False):
        e, h = N.dr_export(), C.c_void_p()
        eng.check(lib.dr_state_export_rows(st.h, N.DR_LIVE, rows.ctypes.data_as(C.POINTER(C.c_int64)), len(rows),
                                           C.byref(h), C.byref(e)))
        cols = {k: v.copy() for k, v in State._columns(e).items()} if keep else None
        lib.dr_range_release(h)
        return cols

    def whole_way(st):
        rows, tf = timed(lambda: do_filter(st))
        e = N.dr_export()
        _, te = timed(lambda: eng.check(lib.dr_state_export(st.h, N.DR_LIVE, C.byref(e))))
        picked, th = timed(lambda: host_index(State._columns(e), rows))
        return {"filter_s": tf, "export_s": te, "host_index_s": th, "total_s": tf + te + th}, rows, picked

    def rows_way(st, materialize):
        tm = 0.0
        if materialize:
            _, tm = timed(st.materialize)
        rows, tf = timed(lambda: do_filter(st))
        _, t1 = timed(lambda: rows_call(st, rows))
        _, t2 = timed(lambda: rows_call(st, rows))
        return {"materialize_s": tm, "filter_s": tf, "first_call_s": t1, "repeat_call_s": t2,
                "total_first_s": tf + t1}, rows

    res = {"whole": [], "walk": [], "gather": []}
    nsel = nlive = None
    for it in range(args.warmup + args.reps):
        keep = it >= args.warmup
        # the three ways alternate, each on a fresh state of its own
        st = fresh()
        r, rows, picked = whole_way(st)
        nlive = st.counts["num_files"]
        st.release()
        if keep:
            res["whole"].append(r)
        for name, mat in (("walk", False), ("gather", True)):
            st = fresh()
            r, rows2 = rows_way(st, mat)
            if it == 0:  # results first: the same rows, the same bytes in every column
                assert np.array_equal(rows, rows2)
                got = rows_call(st, rows2, keep=True)
                for k, w in picked.items():
                    assert got[k].dtype == w.dtype and got[k].tobytes() == w.tobytes(), (name, k)
            st.release()
            if keep:
                res[name].append(r)
        nsel = len(rows)
        del picked
    staged.release()

    def med(name):
        return {k: round(statistics.median(x[k] for x in res[name]), 6) for k in res[name][0]}

    out = {"workload": "config 3, scale %g" % args.scale, "live_files": nlive, "selected": nsel,
           "predicate": "p1 < 5", "reps": args.reps, "warmup": args.warmup, "statistic": "median, host clock (s)",
           "whole_side_way": med("whole"), "walk_path": med("walk"), "gather_path": med("gather"),
           "columns_equal": True}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
