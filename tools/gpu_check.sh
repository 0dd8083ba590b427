# the round-end checks: GPU suite, smoke, the whole bench line (--full), a kernel trace of the ordered path
# run from anywhere on a machine with an MI355X; logs go to $OUT (default check_out/ in the repository root)
cd "$(dirname "$0")/.." && OUT=${OUT:-check_out} && mkdir -p "$OUT" && \
timeout -k 10 1000 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread > "$OUT/gputest.log" 2>&1 && \
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.log" 2>&1 && \
timeout -k 10 600 python -u bench.py --full > "$OUT/bench.log" 2>&1 && \
export TMPDIR=/tmp && \
timeout -k 10 300 rocprofv3 --kernel-trace --stats -T -f csv -d "$OUT/kt_ord" -o kt -- python3 bench.py --path ordered --steps 5 > "$OUT/kt_ord.log" 2>&1
