# Full GPU test suite, then the default bench line with everything --full measures (CPU baseline
# included), outputs under $OUT_DIR (default bench_out/)
set -o pipefail
O=${OUT_DIR:-bench_out}
mkdir -p $O
bash scripts/gpu_tests.sh || exit 1
timeout -k 10 900 python bench.py --full > $O/bench.json 2> $O/bench.err || { tail -30 $O/bench.err; exit 1; }
tail -3 $O/bench.err
cat $O/bench.json
