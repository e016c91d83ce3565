"""Times data skipping on config 3's state and prints one JSON line: the first dr_filter call for
`id >= a AND id < b` rewritten over the statistics (it materialises the live side and runs k_stats_extract),
the cached call, and the partition-only call on the same state beside them; k_stats_extract's device time
and the bytes of stats it read, as a fraction of 8 TB/s.

The call figures are host clocks around dr_filter (each ends in a stream synchronise and the readback of
the selection): the first call once, the cached and the partition-only one as the median, minimum and
maximum of --reps calls. The kernel time is the device's own (event timing, dr_last_timings).

  python scripts/filter_stats_timing.py [--scale 0.1] [--reps 5]
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
from delta_amd import _native as N  # noqa: E402
from delta_amd import skipping as K  # noqa: E402
from delta_amd.delta_log import Engine  # noqa: E402
from delta_amd.predicates import build_program, partition_schema  # noqa: E402

HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--workdir", default=os.environ.get("DR_BENCH_DIR", os.path.join(tempfile.gettempdir(), "dr_bench")))
    args = ap.parse_args()
    table = os.path.join(args.workdir, "c3_s%g" % args.scale)
    exp = bench.build_table(table, 3, args.scale)
    eng = Engine.get(0)
    staged = eng.stage_log(os.path.join(table, "_delta_log"))
    st = staged.replay(exp["min_file_retention_timestamp"])
    staged.release()
    md = next(a["metaData"] for a in st.nonfile if "metaData" in a)
    C = lambda n: ("col", n)  # noqa: E731
    L = lambda t, v: ("lit", t, v)  # noqa: E731
    n = st.counts["num_files"]
    # the synthetic minValues.id lie in [0, 1000) and maxValues.id = min + numRecords with numRecords below
    # 10^6: this range keeps the files whose max reaches 999 000, about two in a thousand
    a, b = 999_000, 1_000_500
    skip = K.skipping_predicates([("and", (">=", C("id"), L("long", a)), ("<", C("id"), L("long", b)))], md)
    part = [(">=", C("p0"), L("date", "2020-03-01")), ("<", C("p0"), L("date", "2020-03-02"))]
    out = {"files": n, "scale": args.scale, "reps": args.reps}
    try:
        def call(prog):
            t0 = time.perf_counter()
            k = len(st.filter(prog))
            return (time.perf_counter() - t0) * 1e3, k

        def spread(prog):
            t = [call(prog)[0] for _ in range(args.reps)]
            return {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t)}
        pprog = build_program(partition_schema(md), part)
        call(pprog)  # builds the partition column's cache and dictionary
        out["partition_only"] = dict(spread(pprog), selected=call(pprog)[1])
        sprog = build_program(partition_schema(md), skip)
        t0 = time.perf_counter()
        st.materialize()
        out["materialize_ms"] = (time.perf_counter() - t0) * 1e3
        eng.set_timing(True)
        first_ms, k = call(sprog)
        ms = eng.last_timings()
        eng.set_timing(False)
        out["stats_first_call_ms"] = first_ms
        out["k_stats_extract_ms"] = ms.get("k_stats_extract")
        out["first_call_kernels_ms"] = {k: round(v, 3) for k, v in sorted(ms.items(), key=lambda kv: -kv[1])[:6]}
        # the bytes of stats the kernel read: measured on the first rows (a range export), scaled to the side
        head = min(n, 100000)
        stats_bytes = int(st.export_range(N.DR_LIVE, 0, head)["stats_off"][-1]) * n // max(head, 1)
        out["stats_bytes_estimated"] = stats_bytes
        if stats_bytes and out["k_stats_extract_ms"]:
            out["fraction_of_8TBps"] = stats_bytes / (out["k_stats_extract_ms"] * 1e-3) / HBM_BYTES_PER_S
        out["stats_cached"] = dict(spread(sprog), selected=k)
    finally:
        st.release()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
