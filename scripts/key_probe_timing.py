"""Times dr_state_probe_keys on config 3's state (the largest stats-bearing state scripts/agg_timing.py builds)
with 10^3, 10^5 and 10^6 random keys over minValues.id / maxValues.id, and prints one JSON line per key count:
  (a) State.probe_keys with the bounds' cache columns already built;
  (b) the host route on the same warm cache: State.stats_column for minValues.id and for maxValues.id (two
      8-byte columns and two null masks over PCIe), then numpy.searchsorted over the sorted distinct keys for
      the selection and a difference array for the per-key file counts;
  (c) the device's own kernel times (event timing, dr_last_timings) of the k_probe_* kernels, with
      DR_OPT_PROBE_SEARCH 0 (splitter table in LDS, k_probe_files) and 1 (plain global bisection,
      k_probe_files_plain), each the median of 5 calls.
Host clocks around the calls (each ends in a stream synchronise and the readback of the result): after one
warm-up call, the median, minimum and maximum of --reps calls. (a) and (b) are checked to agree first.

  python scripts/key_probe_timing.py [--scale 1] [--reps 7]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from delta_amd import _native as N  # noqa: E402
from delta_amd.delta_log import DeltaLog  # noqa: E402

LO, HI = (N.DR_SRC_STATS_MIN, ("id",), "long"), (N.DR_SRC_STATS_MAX, ("id",), "long")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--workdir", default=os.environ.get("DR_BENCH_DIR", os.path.join(tempfile.gettempdir(), "dr_bench")))
    args = ap.parse_args()
    table = os.path.join(args.workdir, "c3_s%g" % args.scale)
    bench.build_table(table, 3, args.scale)
    DeltaLog.clear_cache()
    snap = DeltaLog.for_table(table).snapshot
    st, eng = snap.state, snap.state.eng
    n = snap.num_of_files

    def spread(fn):
        fn()  # warm-up: caches built, clocks up
        t = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
        return {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t)}

    def kernels(fn):
        runs = []
        for _ in range(5):
            eng.set_timing(True)
            try:
                fn()
                ms = eng.last_timings()
            finally:
                eng.set_timing(False)
            runs.append({k: v for k, v in ms.items() if k.startswith("k_probe")})
        return {k: round(statistics.median(r.get(k, 0.0) for r in runs), 4) for k in runs[0]}

    try:
        t0 = time.perf_counter()
        mn, mn_null = st.stats_column(*LO)  # builds both columns
        mx, mx_null = st.stats_column(*HI)
        first_ms = (time.perf_counter() - t0) * 1e3
        known = (mn_null == 0) & (mx_null == 0)
        lo_v, hi_v = int(mn[known].min()), int(mx[known].max())
        rng = np.random.default_rng(17)
        for nkeys in (10 ** 3, 10 ** 5, 10 ** 6):
            # keys over the table's id range and as much again beyond it: part of them are pure inserts
            keys = rng.integers(lo_v, hi_v + (hi_v - lo_v) + 1, size=nkeys, dtype=np.int64)

            def device():
                return st.probe_keys(LO, HI, keys)

            def host():
                a, za = st.stats_column(*LO)
                b, zb = st.stats_column(*HI)
                dk, inv = np.unique(keys, return_inverse=True)
                unknown = (za != 0) | (zb != 0)
                first = np.searchsorted(dk, a, side="left")
                last = np.searchsorted(dk, b, side="right")
                hits = np.where(unknown, -1, np.maximum(last - first, 0))
                sel = np.flatnonzero(hits != 0)
                hit = hits > 0
                diff = np.bincount(first[hit], minlength=dk.size + 1) - np.bincount(last[hit], minlength=dk.size + 1)
                return {"selected": sel, "hits": hits[sel], "key_files": np.cumsum(diff)[:dk.size][inv], "unknown": int(unknown.sum())}
            d, h = device(), host()
            assert d["unknown"] == h["unknown"] and all(np.array_equal(d[k], h[k]) for k in ("selected", "hits", "key_files"))
            out = {"files": n, "scale": args.scale, "reps": args.reps, "keys": nkeys, "distinct": int(np.unique(keys).size),
                   "selected": int(d["selected"].size), "unknown": d["unknown"], "keys_in_no_file": int((d["key_files"] == 0).sum()),
                   "first_columns_ms": first_ms, "a_probe_keys": spread(device), "b_stats_columns_searchsorted": spread(host)}
            out["a_beats_b_beyond_spread"] = out["a_probe_keys"]["max_ms"] < out["b_stats_columns_searchsorted"]["min_ms"]
            out["c_kernels_ms_lds"] = kernels(device)
            with eng.options(probe_search=1):
                assert all(np.array_equal(device()[k], d[k]) for k in ("selected", "hits", "key_files"))
                out["c_kernels_ms_plain"] = kernels(device)
                out["a_probe_keys_plain"] = spread(device)
            print(json.dumps(out), flush=True)
    finally:
        snap.release()
        DeltaLog.clear_cache()


if __name__ == "__main__":
    main()
