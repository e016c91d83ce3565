"""Times dr_filter with string pattern predicates and prints one JSON line:

  (i)  a 1,000,000-file table in 8,760 hourly partitions, the hour kept as a timestamp column and as a
       string column: `hourstr LIKE '2020-03-0%'` under filter_eval 0 / 1 / 2, and beside it the
       timestamp range predicate of DESIGN §4j that selects the same files (the yardstick: under
       filter_eval 0 both are one table lookup per file);
  (ii) a 1,000,000-file table with a unique 40-byte string per file (no dictionary: every file is
       matched): `LIKE '%_x%y'`, CONTAINS and STARTSWITH, and an `=` leaf on the same column for scale.

Every figure is a host clock around dr_filter calls (each ends in a stream synchronise and the readback
of the selection): the median, minimum and maximum of --reps calls after --warmup untimed ones, so it
is a call time (launches and readback included), not a kernel time.

  python scripts/filter_like_timing.py [--files 1000000] [--reps 5] [--warmup 1] [--workdir DIR]
"""
import argparse
import datetime as dt
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_table(path, ptypes, n, pv):
    log = os.path.join(path, "_delta_log")
    if os.path.exists(os.path.join(log, "%020d.json" % 0)):
        return log
    os.makedirs(log, exist_ok=True)
    schema = {"type": "struct", "fields": [{"name": c, "type": t, "nullable": True, "metadata": {}} for c, t in ptypes.items()]}
    md = {"id": "like-timing", "format": {"provider": "parquet", "options": {}}, "schemaString": json.dumps(schema),
          "partitionColumns": list(ptypes), "configuration": {}, "createdTime": 1}
    tmp = os.path.join(log, "tmp.json")
    with open(tmp, "w") as f:
        f.write(json.dumps({"protocol": {"minReaderVersion": 1, "minWriterVersion": 2}}) + "\n")
        f.write(json.dumps({"metaData": md}) + "\n")
        for k in range(n):
            f.write('{"add":{"path":"f%d","partitionValues":%s,"size":1,"modificationTime":1000,"dataChange":true}}\n'
                    % (k, json.dumps(pv(k), separators=(",", ":"))))
    os.rename(tmp, os.path.join(log, "%020d.json" % 0))
    return log


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workdir", default=os.environ.get("DR_BENCH_DIR", os.path.join(tempfile.gettempdir(), "dr_bench")))
    args = ap.parse_args()

    from delta_amd.delta_log import Engine
    from delta_amd.predicates import build_program, timestamp_micros

    eng = Engine.get(0)
    C = lambda n: ("col", n)  # noqa: E731
    S = lambda v: ("lit", "string", v)  # noqa: E731

    def timed_calls(st, prog):
        n, t = None, []
        for it in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            sel = st.filter(prog)
            if it >= args.warmup:
                t.append((time.perf_counter() - t0) * 1e3)
            n = len(sel)
        return {"selected": n, "median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4)}

    def run(log, schema, preds, evals):
        staged = eng.stage_log(log)
        st = staged.replay(0)
        staged.release()
        out = {}
        try:
            for name, p in preds.items():
                prog = build_program(schema, p)
                for ev in evals:
                    with eng.options(filter_eval=ev):
                        out["%s, filter_eval=%d" % (name, ev)] = timed_calls(st, prog)
        finally:
            st.release()
        return out

    # (i) 8,760 hourly partitions from 2020-01-01 on
    t0 = dt.datetime(2020, 1, 1)

    def hour(k):
        h = (t0 + dt.timedelta(hours=k % 8760)).strftime("%Y-%m-%d %H:00:00")
        return {"hour": h, "hourstr": h}

    types_i = {"hour": "timestamp", "hourstr": "string"}
    log_i = write_table(os.path.join(args.workdir, "like_hourly_%d" % args.files), types_i, args.files, hour)
    ts = lambda s: ("lit", "timestamp", timestamp_micros(s))  # noqa: E731
    res_i = run(log_i, types_i, {
        "hourstr LIKE '2020-03-0%'": [("like", C("hourstr"), S("2020-03-0%"))],
        "hourstr LIKE '2020-03-0_ %'": [("like", C("hourstr"), S("2020-03-0_ %"))],
        "hour >= '2020-03-01' AND hour < '2020-03-10'": [(">=", C("hour"), ts("2020-03-01")), ("<", C("hour"), ts("2020-03-10"))],
    }, (0, 1, 2))

    # (ii) a unique 40-byte value per file
    def unique(k):
        # one value in 16 ends in "xy" (the others in "zy"), so the patterns select a sixteenth
        return {"u": "k%09d-%07x-payload-of-bytes-%02d%sy" % (k, (k * 2654435761) & 0xfffffff, k % 97, "zx"[k % 16 == 0])}

    types_ii = {"u": "string"}
    log_ii = write_table(os.path.join(args.workdir, "like_unique_%d" % args.files), types_ii, args.files, unique)
    res_ii = run(log_ii, types_ii, {
        "u LIKE '%_x%y'": [("like", C("u"), S("%_x%y"))],
        "u CONTAINS 'bytes-42x'": [("contains", C("u"), S("bytes-42x"))],
        "u STARTSWITH 'k00001234'": [("startswith", C("u"), S("k00001234"))],
        "u = <one value>": [("=", C("u"), S(unique(1234)["u"]))],
    }, (1, 2))

    print(json.dumps({"files": args.files, "reps": args.reps, "warmup": args.warmup,
                      "statistic": "host clock around dr_filter, ms per call", "hourly": res_i, "unique": res_ii}))


if __name__ == "__main__":
    main()
