"""Times dr_state_aggregate on config 3's state and prints one JSON line:
  (a) sum(numRecords) as before: State.stats_column plus a numpy sum (9 bytes a file over PCIe, a host pass);
  (b) the same through dr_state_aggregate, the column cached;
  (c) five specs in one call -- sum(numRecords), sum(size), min(minValues.id), max(maxValues.id), max(modificationTime);
  (d) the same five grouped by dr_state_partition_groups of all live files;
  (e) Snapshot.scan_sizes against the same three sums taken from files_for_scan records, at a partition range
      that keeps about 1 % of the files.
Host clocks around the calls (each ends in a stream synchronise and the readback of the result): after a
warm-up call, the median, minimum and maximum of --reps calls. Kernel times are the device's own (event
timing, dr_last_timings), taken in calls of their own; the reduce kernel's is also given as a fraction of the
time its input columns take at 8 TB/s (rows == NULL: the columns and their null bytes alone; a selection adds
8 bytes a row).

  python scripts/agg_timing.py [--scale 1] [--reps 7]
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

HBM_BYTES_PER_S = 8e12
NREC = ("sum", N.DR_SRC_STATS_NUMRECORDS, (), "long")
FIVE = [NREC, ("sum", "size"), ("min", N.DR_SRC_STATS_MIN, ("id",), "long"), ("max", N.DR_SRC_STATS_MAX, ("id",), "long"), ("max", "mtime")]
FIVE_BYTES = 9 + 8 + 9 + 9 + 8  # per file: an 8-byte value each, a null byte for the three statistics


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
    out = {"files": n, "scale": args.scale, "reps": args.reps, "tile": N.AGG_TILE}
    C = lambda name: ("col", name)  # noqa: E731
    L = lambda t, v: ("lit", t, v)  # noqa: E731

    def spread(fn):
        fn()  # warm-up: caches built, clocks up
        t = []
        for _ in range(max(args.reps, 5)):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
        return {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t)}

    def kernels(fn):
        eng.set_timing(True)
        try:
            fn()
            ms = eng.last_timings()
        finally:
            eng.set_timing(False)
        return {k: round(v, 4) for k, v in ms.items() if k.startswith("k_agg")}

    try:
        t0 = time.perf_counter()
        st.materialize()
        out["materialize_ms"] = (time.perf_counter() - t0) * 1e3

        def old_sum():
            v, z = st.stats_column(N.DR_SRC_STATS_NUMRECORDS)
            return int(v.sum())

        def new_sum():
            return int(st.aggregate([NREC])["value_lo"][0, 0])
        t0 = time.perf_counter()
        want = old_sum()  # builds the column
        out["first_column_ms"] = (time.perf_counter() - t0) * 1e3
        assert new_sum() == want
        out["a_stats_column_numpy"] = spread(old_sum)
        out["b_aggregate_sum"] = spread(new_sum)
        kb = [kernels(new_sum) for _ in range(5)]
        out["b_kernels_ms"] = kb[-1]
        tile_ms = statistics.median(k["k_agg_tiles"] for k in kb)
        out["b_k_agg_tiles_median_ms"] = tile_ms
        out["b_fraction_of_8TBps"] = 9 * n / (tile_ms * 1e-3) / HBM_BYTES_PER_S

        five = lambda: st.aggregate(FIVE)  # noqa: E731
        out["c_five_specs"] = spread(five)
        kc = [kernels(five) for _ in range(5)]
        out["c_kernels_ms"] = kc[-1]
        tile_ms = statistics.median(k["k_agg_tiles"] for k in kc)
        out["c_k_agg_tiles_median_ms"] = tile_ms
        out["c_fraction_of_8TBps"] = FIVE_BYTES * n / (tile_ms * 1e-3) / HBM_BYTES_PER_S

        t0 = time.perf_counter()
        order, off = st.partition_group_offsets(None)
        out["partition_groups_ms"] = (time.perf_counter() - t0) * 1e3
        order, off = np.asarray(order, dtype=np.int64), np.asarray(off, dtype=np.int64)
        out["groups"] = len(off) - 1
        grouped = lambda: st.aggregate(FIVE, order, off)  # noqa: E731
        res = grouped()
        assert int(res["value_lo"][0].sum()) == want
        out["d_five_specs_grouped"] = spread(grouped)
        kd = [kernels(grouped) for _ in range(5)]
        out["d_kernels_ms"] = kd[-1]
        tile_ms = statistics.median(k["k_agg_tiles"] for k in kd)
        out["d_k_agg_tiles_median_ms"] = tile_ms
        out["d_fraction_of_8TBps"] = (FIVE_BYTES + 8) * n / (tile_ms * 1e-3) / HBM_BYTES_PER_S

        # about 1 % of the files: four of the table's partition days
        filters = [(">=", C("p0"), L("date", "2020-03-01")), ("<", C("p0"), L("date", "2020-03-05"))]

        def from_records():
            recs = snap.files_for_scan(filters)
            rows = [json.loads(r["stats"]).get("numRecords") if r.get("stats") else None for r in recs]
            return {"bytesCompressed": sum(r["size"] for r in recs), "rows": None if None in rows else sum(rows), "files": len(recs)}
        sizes = snap.scan_sizes(filters)
        assert sizes["partition"] == from_records(), (sizes, from_records())
        out["selected"] = sizes["partition"]["files"]
        out["e_scan_sizes"] = spread(lambda: snap.scan_sizes(filters))
        out["e_from_records"] = spread(from_records)
    finally:
        snap.release()
        DeltaLog.clear_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
