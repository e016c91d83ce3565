"""Times the replay of config 3 from two checkpoints written from the same actions, both with
use_dictionary=False and SNAPPY: every leaf PLAIN (the baseline, on this build), and add.path /
remove.path as DELTA_BYTE_ARRAY with the integer leaves as DELTA_BINARY_PACKED. Prints one JSON line
(also written to $OUT_DIR/delta_pages_timing.json when OUT_DIR is set) with, per file: the checkpoint's
bytes, its decompressed page bytes, the first replay of the staged segment (host clock; for the delta
file it holds the sizing pass and its read-back), the step (median host clock of --reps replays after
that) and the per-kernel device times (dr_set_timing, median over --reps timed replays) of the SNAPPY
kernels, the delta kernels, k_pq_data / k_pq_data_dl and k_ckpt_assemble. The two states' counters and
record sums are compared before anything is reported.

  python scripts/delta_pages_timing.py [--scale 1.0] [--reps 10] [--workdir DIR]
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

DELTA = {"add.path": "DELTA_BYTE_ARRAY", "remove.path": "DELTA_BYTE_ARRAY", "add.size": "DELTA_BINARY_PACKED",
         "add.modificationTime": "DELTA_BINARY_PACKED", "remove.deletionTimestamp": "DELTA_BINARY_PACKED",
         "remove.size": "DELTA_BINARY_PACKED"}
KERNELS = ("k_snap", "k_page_copy", "k_ba_", "k_dl_", "k_pq_d", "k_ckpt_assemble")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--workdir", default=os.environ.get("DR_BENCH_DIR", os.path.join(tempfile.gettempdir(), "dr_bench")))
    args = ap.parse_args()

    from delta_amd.delta_log import Engine
    from delta_amd.testing import synth as S

    eng = Engine.get(0)
    out = {"workload": "config 3, scale %g" % args.scale, "reps": args.reps,
           "statistic": "median; first_replay_s / step_s: host clock (s); kernels: device time (ms)", "files": {}}
    sums = {}
    for name, enc in (("plain", None), ("delta", DELTA)):
        d = os.path.join(args.workdir, "dp_%s_s%g" % (name, args.scale))
        marker = os.path.join(d, "expected.json")
        if not os.path.exists(marker):
            exp = S.build_table(d, S.config_spec(3, args.scale), seed=3, keep_ids=False, use_dictionary=False,
                                column_encoding=enc)
            with open(marker, "w") as f:
                json.dump({"cutoff": int(exp.min_file_retention_timestamp), "num_files": int(exp.num_files)}, f)
        exp = json.load(open(marker))
        lp = os.path.join(d, "_delta_log")
        ck = sum(os.path.getsize(os.path.join(lp, f)) for f in os.listdir(lp) if ".checkpoint" in f)
        print("[delta_pages_timing] %s: checkpoint %d bytes" % (name, ck), file=sys.stderr, flush=True)
        staged = eng.stage_log(lp)
        t = time.perf_counter()
        st = staged.replay(exp["cutoff"])
        first = time.perf_counter() - t
        assert st.counts["num_files"] == exp["num_files"]
        sums[name] = (dict(st.counts), st.record_sums())
        st.release()
        steps = []
        for _ in range(args.reps):
            t = time.perf_counter()
            st = staged.replay(exp["cutoff"])
            steps.append(time.perf_counter() - t)
            st.release()
        eng.set_timing(True)
        runs = []
        for _ in range(args.reps):
            st = staged.replay(exp["cutoff"])
            runs.append({k: v for k, v in eng.last_timings().items() if k.startswith(KERNELS)})
            st.release()
        eng.set_timing(False)
        plan = staged.plan()
        staged.release()
        out["files"][name] = {
            "checkpoint_bytes": ck, "pages_decompressed_bytes": plan["pages_decompressed_bytes"],
            "delta_pages": plan["delta_pages"], "delta_arena_bytes": plan["delta_arena_bytes"],
            "first_replay_s": round(first, 6), "step_s": round(statistics.median(steps), 6),
            "step_min_max_s": [round(min(steps), 6), round(max(steps), 6)],
            "kernels_ms": {k: round(statistics.median(r.get(k, 0.0) for r in runs), 4) for k in sorted(set().union(*runs))}}
    assert sums["plain"] == sums["delta"], "the two checkpoints replay to different states"
    line = json.dumps(out)
    print(line)
    if os.environ.get("OUT_DIR"):
        os.makedirs(os.environ["OUT_DIR"], exist_ok=True)
        with open(os.path.join(os.environ["OUT_DIR"], "delta_pages_timing.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
