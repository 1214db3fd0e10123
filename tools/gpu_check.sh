set -o pipefail
# GPU tests, smoke() and the full benchmark (CPU baseline included); logs under $OUT_DIR (default build/logs)
out=${OUT_DIR:-build/logs}
mkdir -p "$out"
timeout -k 10 500 python -u -m pytest tests -m gpu -v --timeout 200 --timeout-method thread > "$out/t_gpu.log" 2>&1 || { grep -E "Error|FAILED|assert" "$out/t_gpu.log" | head -30; exit 1; }
tail -1 "$out/t_gpu.log"
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" > "$out/smoke.log" 2>&1 || { tail -20 "$out/smoke.log"; exit 1; }
tail -2 "$out/smoke.log"
timeout -k 10 600 python -u bench.py --full > "$out/bench.log" 2>&1 || { tail -20 "$out/bench.log"; exit 1; }
tail -1 "$out/bench.log"
