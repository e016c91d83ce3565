"""LZ4 checkpoint pages against their ZSTD and SNAPPY twins: config 3 (default scale 0.05), built three times from one
seed (compression "lz4" -- Parquet codec 7, LZ4_RAW --, "zstd" and "snappy"), each replayed ten times with kernel timing
on after two untimed warm-up replays, in one process. Prints one JSON line: per codec the decompression kernels' ms per
replay (median and spread over the ten) and, for k_lz4 and k_zstd, the decompressed GB/s (out_bytes / time)."""
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.prof_zstd import measure  # noqa: E402


def main():
    from delta_amd.delta_log import Engine
    from delta_amd.testing import synth as S
    scale = float(sys.argv[1]) if len(sys.argv) > 1 else 0.05
    engine = Engine.get(0)
    out = {"config": 3, "scale": scale}
    with tempfile.TemporaryDirectory() as d:
        for codec, prefixes in (("lz4", ("k_lz4",)), ("zstd", ("k_zstd",)), ("snappy", ("k_snap_", "k_page_copy"))):
            t = os.path.join(d, codec)
            exp = S.build_table(t, S.config_spec(3, scale), seed=3, compression=codec)
            ms, plan = measure(engine, os.path.join(t, "_delta_log"), exp.min_file_retention_timestamp, prefixes)
            med = statistics.median(ms)
            out[codec] = {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}
            if codec != "snappy":
                out[codec].update(pages=plan[codec + "_pages"], in_bytes=plan[codec + "_in_bytes"],
                                  out_bytes=plan[codec + "_out_bytes"], copy_bytes=plan["copy_bytes"],
                                  out_gb_per_s=round(plan[codec + "_out_bytes"] / (med * 1e-3) / 1e9, 3) if med else None)
            else:
                out[codec].update(in_bytes=plan["snappy_in_bytes"], out_bytes=plan["snappy_out_bytes"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
