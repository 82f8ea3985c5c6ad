#!/bin/bash
# the wide (fp64 MFMA) path: its parity tests, then the cfg5 bench line   bash tools/gpu_wide.sh [out dir]
set -o pipefail
OUT=${1:-bench_out/wide}
mkdir -p "$OUT"
timeout -k 10 300 python -u -m pytest tests/test_gpu_parity.py -x -q -k "wide or n64 or 64 or dense_n16 or safe" --timeout 120 --timeout-method thread > "$OUT/tests.log" 2>&1 || { tail -30 "$OUT/tests.log"; exit 1; }
tail -1 "$OUT/tests.log"
timeout -k 10 300 python -u bench.py --full --N 64 --K 1024 --T 400 --R 6250 --steps 10 --warmup 2 --topology dense --no-cpu-baseline > "$OUT/cfg5.log" 2>&1 || { tail -20 "$OUT/cfg5.log"; exit 1; }
grep -o '"ms_per_step": [0-9.]*\|"kernel_ms": [0-9.]*\|"loglik_last": [-0-9.]*' "$OUT/cfg5.log"
