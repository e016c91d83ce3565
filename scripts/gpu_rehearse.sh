# smoke(), then a 2-rank bench rehearsal on the one GPU (gloo exchange, the N>1 code path), outputs
# under $OUT_DIR (default bench_out/)
set -e
O=${OUT_DIR:-bench_out}/reh
mkdir -p $O
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1
DR_BENCH_BACKEND=gloo timeout -k 10 600 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29533 bench.py --gpus 2 --steps 3 --warmup 1 --scale 0.25 --full > $O/n2.json 2> $O/n2.err
tail -1 $O/smoke.log
tail -1 $O/n2.json | cut -c1-600
