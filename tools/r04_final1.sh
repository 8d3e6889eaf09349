#!/bin/bash
# snapshot writer + K7 timing + full GPU suite + driver-like bench
set -o pipefail
mkdir -p bench_out
timeout -k 10 300 python -m pytest tests/test_gpu_api.py -x -q -m gpu -k "snapshot or skipped_and_missing or preview or jpeg" > bench_out/f1_snap.log 2>&1 || { tail -n 30 bench_out/f1_snap.log; exit 1; }
tail -n 3 bench_out/f1_snap.log
timeout -k 10 200 python tools/k7_time.py --out bench_out/k7_time.json > bench_out/f1_k7.log 2>&1 || { tail -n 20 bench_out/f1_k7.log; exit 1; }
cat bench_out/f1_k7.log
timeout -k 10 900 python -m pytest tests -x -q -m gpu > bench_out/f1_gpu.log 2>&1 || { tail -n 40 bench_out/f1_gpu.log; exit 1; }
tail -n 3 bench_out/f1_gpu.log
timeout -k 10 600 python bench.py --full --gpus 1 --steps 20 --warmup 5 > bench_out/f1_bench.json 2> bench_out/f1_bench.err || { tail -n 20 bench_out/f1_bench.err; exit 1; }
cat bench_out/f1_bench.json
