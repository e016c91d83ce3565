"""Times dr_filter with a date-function predicate on config 4's table and prints one JSON line: the range
`p0 >= DATE'2020-03-01' AND p0 < DATE'2020-03-02'` (plain leaves, the yardstick) beside
`year(p0) = 2020 AND month(p0) IN (3, 4, 5) AND dayofyear(p0) = 61` (function leaves), which select the
same files (one day's: the readback of the selection stays small), under
filter_eval 0 (dictionary codes), 1 (per-file leaves) and 2 (the generic interpreter).

Every figure is a host clock around dr_filter calls (each ends in a stream synchronise and the readback
of the selection): the median, minimum and maximum of --reps calls after --warmup untimed ones, so it
is a call time (launches and readback included), not a kernel time.

  python scripts/filter_dates_timing.py [--scale 0.1] [--reps 5] [--warmup 1]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from delta_amd.delta_log import Engine  # noqa: E402
from delta_amd.predicates import build_program, partition_schema  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workdir", default=os.environ.get("DR_BENCH_DIR", os.path.join(tempfile.gettempdir(), "dr_bench")))
    args = ap.parse_args()
    table = os.path.join(args.workdir, "c4_s%g" % args.scale)
    exp = bench.build_table(table, 4, args.scale)
    eng = Engine.get(0)
    staged = eng.stage_log(os.path.join(table, "_delta_log"))
    st = staged.replay(exp["min_file_retention_timestamp"])
    staged.release()
    schema = partition_schema(next(a["metaData"] for a in st.nonfile if "metaData" in a))
    C = lambda n: ("col", n)  # noqa: E731
    L = lambda t, v: ("lit", t, v)  # noqa: E731
    preds = {
        "range": [(">=", C("p0"), L("date", "2020-03-01")), ("<", C("p0"), L("date", "2020-03-02"))],
        "year_month_day": [("=", ("year", C("p0")), L("integer", 2020)), ("in", ("month", C("p0")), [L("integer", m) for m in (3, 4, 5)]),
                           ("=", ("dayofyear", C("p0")), L("integer", 61))],
    }
    out = {"files": st.counts["num_files"], "scale": args.scale, "reps": args.reps}
    try:
        for name, p in preds.items():
            prog = build_program(schema, p)
            for ev in (0, 1, 2):
                with eng.options(filter_eval=ev):
                    t, n = [], None
                    for it in range(args.warmup + args.reps):
                        t0 = time.perf_counter()
                        n = len(st.filter(prog))
                        if it >= args.warmup:
                            t.append((time.perf_counter() - t0) * 1e3)
                out["%s/eval%d" % (name, ev)] = {"selected": n, "median_ms": round(statistics.median(t), 4),
                                                 "min_ms": round(min(t), 4), "max_ms": round(max(t), 4)}
    finally:
        st.release()
    assert len({v["selected"] for k, v in out.items() if isinstance(v, dict)}) == 1, out
    print(json.dumps(out))


if __name__ == "__main__":
    main()
