# rank walk: its parity tests, then the C2 bench with its checks (--full) and a kernel trace of the plain run
# run on a machine with an MI355X; logs go to $OUT (default check_out/ in the repository root)
cd "$(dirname "$0")/.." && OUT=${OUT:-check_out} && mkdir -p "$OUT" && \
timeout -k 10 300 python -u -m pytest tests/test_rank_gpu.py -x -v --timeout 120 --timeout-method thread > "$OUT/rank_tests.log" 2>&1 && \
timeout -k 10 300 python -u bench.py --full --no-other --no-cpu > "$OUT/bench_rank.log" 2>&1 && \
export TMPDIR=/tmp && \
timeout -k 10 300 rocprofv3 --kernel-trace --stats -T -f csv -d "$OUT/kt_rank" -o kt -- python3 bench.py --steps 5 > "$OUT/kt_rank.log" 2>&1
