# Round-end rehearsal on one MI355X: GPU test suite, smoke(), bench.py --full (GPT-J + SD + the N=1
# secondaries), each step bounded.   usage: bash tools/gpu_round_end.sh LOG_DIR
set -o pipefail
export TMPDIR=/tmp
OUT=$(realpath -m "${1:?usage: bash tools/gpu_round_end.sh LOG_DIR}")
cd "$(dirname "$0")/.."
mkdir -p "$OUT"
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > "$OUT/re_tests.log" 2>&1 || { tail -30 "$OUT/re_tests.log"; exit 1; }
tail -1 "$OUT/re_tests.log"
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" > "$OUT/re_smoke.log" 2>&1 || { tail -20 "$OUT/re_smoke.log"; exit 1; }
tail -1 "$OUT/re_smoke.log"
timeout -k 10 600 python -u bench.py --full > "$OUT/re_bench.log" 2>&1 || { tail -20 "$OUT/re_bench.log"; exit 1; }
grep "^\[bench\]" "$OUT/re_bench.log"
grep "^{" "$OUT/re_bench.log"
