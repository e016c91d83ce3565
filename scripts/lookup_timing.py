"""Times dr_state_lookup_paths on config 3 (the 10M-file table bench.py builds) for 10^4, 10^6 and
10^7 query paths, half of them present (live files and tombstones, drawn with repeats) and half absent
(a present path with one byte appended), and prints one JSON line (also written to
$OUT_DIR/lookup_timing.json when OUT_DIR is set):

  (1) the index build: k_lookup_build's device time on a fresh state's first lookup, and that first
      call's host clock against a repeat of the same call
  (2) the lookup call end to end (host clock, timing off) and its probe kernel alone (the sum of the
      k_lookup_probe launches of one call, dr_last_timings, timing on) per query count
  (3) the route without the entry point: dr_state_export of both sides, a host dict
      {path: (side, position)} over their columns, and one dict probe per query

Host clocks are medians of --reps calls after one untimed call; the answers of (2) are checked
against (3)'s for every query before anything is reported.

  python scripts/lookup_timing.py [--scale 1.0] [--reps 5] [--sizes 10000,1000000,10000000] [--workdir DIR]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="10000,1000000,10000000")
    ap.add_argument("--workdir", default=os.environ.get("DR_BENCH_DIR", os.path.join(tempfile.gettempdir(), "dr_bench")))
    args = ap.parse_args()
    sizes = [int(x) for x in args.sizes.split(",")]

    from bench import build_table
    from delta_amd import _native as N
    from delta_amd.delta_log import Engine, State

    path = os.path.join(args.workdir, "c3_s%g" % args.scale)  # the table bench.py builds and caches
    exp = build_table(path, 3, args.scale)
    eng = Engine.get(0)
    lib = eng.lib
    staged = eng.stage_log(os.path.join(path, "_delta_log"))
    cutoff = exp["min_file_retention_timestamp"]

    def note(msg):
        print("[lookup_timing] " + msg, file=sys.stderr, flush=True)

    def timed(f):
        t = time.perf_counter()
        r = f()
        return r, time.perf_counter() - t

    def lookup(st, blob, off):
        n = len(off) - 1
        hit, row = np.empty(n, np.uint8), np.empty(n, np.int64)
        eng.check(lib.dr_state_lookup_paths(st.h, blob.ctypes.data, off.ctypes.data, n, 0, hit.ctypes.data, row.ctypes.data))
        return hit, row

    # (3) first: its exports also give the paths the queries are drawn from
    ref = staged.replay(cutoff)
    sides, t_export = [], 0.0
    for which in (N.DR_LIVE, N.DR_TOMBSTONES):
        e = N.dr_export()
        _, t = timed(lambda: eng.check(lib.dr_state_export(ref.h, which, C.byref(e))))
        t_export += t
        cols = State._columns(e)
        sides.append((cols["path_off"].copy(), cols["path_bytes"].copy()))

    def build_dict():
        d = {}
        for which, (off, data) in enumerate(sides):
            raw = data.tobytes()
            o = off.tolist()
            d.update(zip((raw[a:b] for a, b in zip(o[:-1], o[1:])), ((which + 1, r) for r in range(len(o) - 1))))
        return d
    note("both sides exported in %.2f s" % t_export)
    table, t_dict = timed(build_dict)
    note("host dict of %d paths in %.2f s" % (len(table), t_dict))
    n_side = [len(off) - 1 for off, _ in sides]

    # the pool of present paths: both sides' path columns back to back
    pool_off = np.concatenate([sides[0][0][:-1], sides[1][0][:-1] + len(sides[0][1]), [len(sides[0][1]) + len(sides[1][1])]])
    pool = np.concatenate([sides[0][1], sides[1][1]])
    rng = np.random.default_rng(4)

    def queries(nq, chunk=1 << 20):
        blobs, lens_all = [], []
        for lo in range(0, nq, chunk):
            n = min(chunk, nq - lo)
            pick = rng.integers(0, len(pool_off) - 1, size=n)
            absent = rng.random(n) < 0.5
            lens = pool_off[pick + 1] - pool_off[pick]
            qoff = np.zeros(n + 1, np.int64)
            np.cumsum(lens + absent, out=qoff[1:])
            inner = np.arange(int(lens.sum()), dtype=np.int64) - np.repeat(np.cumsum(lens) - lens, lens)
            b = np.empty(int(qoff[-1]), np.uint8)
            b[np.repeat(qoff[:-1], lens) + inner] = pool[np.repeat(pool_off[pick], lens) + inner]
            b[qoff[1:][absent] - 1] = ord("x")
            blobs.append(b)
            lens_all.append(lens + absent)
        off = np.zeros(nq + 1, np.int64)
        np.cumsum(np.concatenate(lens_all), out=off[1:])
        return np.concatenate(blobs + [np.zeros(1, np.uint8)]), off

    out = {"workload": "config 3, scale %g" % args.scale, "live_files": n_side[0], "tombstones": n_side[1],
           "reps": args.reps, "statistic": "median, host clock (s); kernels: device time (ms)",
           "whole_side_route": {"export_both_sides_s": round(t_export, 6), "host_dict_build_s": round(t_dict, 6)},
           "sizes": {}}

    # (1) the index build, on a fresh state
    blob, off = queries(sizes[0])
    st = staged.replay(cutoff)
    eng.set_timing(True)
    _, t_first = timed(lambda: lookup(st, blob, off))
    tm = eng.last_timings()
    eng.set_timing(False)
    _, t_repeat = timed(lambda: lookup(st, blob, off))
    slots = 64
    while slots < 2 * (n_side[0] + n_side[1]):
        slots *= 2
    out["index"] = {"k_lookup_build_ms": round(tm.get("k_lookup_build", 0.0), 4), "first_call_s": round(t_first, 6),
                    "repeat_call_s": round(t_repeat, 6), "queries": sizes[0], "slots": slots, "bytes": 12 * slots}

    # (2) and (3)'s probe, per query count
    for nq in sizes:
        note("%d queries" % nq)
        blob, off = queries(nq)
        (hit, row), _ = timed(lambda: lookup(st, blob, off))  # untimed warm-up, kept for the check
        raw, o = blob.tobytes(), off.tolist()

        def host_probe():
            miss = (0, -1)
            return [table.get(raw[a:b], miss) for a, b in zip(o[:-1], o[1:])]
        want, t_probe = timed(host_probe)
        assert hit.tolist() == [w[0] for w in want] and row.tolist() == [w[1] for w in want], nq
        del want, raw, o
        calls = [timed(lambda: lookup(st, blob, off))[1] for _ in range(args.reps)]
        eng.set_timing(True, "k_lookup_probe")
        kern = []
        for _ in range(args.reps):
            lookup(st, blob, off)
            kern.append(sum(v for k, v in eng.last_timings().items() if k.startswith("k_lookup_probe")))
        eng.set_timing(False)
        out["sizes"][str(nq)] = {"present_fraction": round(float(np.mean(hit != 0)), 4), "query_bytes": int(off[-1]),
                                 "lookup_call_s": round(statistics.median(calls), 6),
                                 "k_lookup_probe_ms": round(statistics.median(kern), 4),
                                 "host_dict_probe_s": round(t_probe, 6)}
    st.release()
    ref.release()
    staged.release()
    line = json.dumps(out)
    print(line)
    if os.environ.get("OUT_DIR"):
        os.makedirs(os.environ["OUT_DIR"], exist_ok=True)
        with open(os.path.join(os.environ["OUT_DIR"], "lookup_timing.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
