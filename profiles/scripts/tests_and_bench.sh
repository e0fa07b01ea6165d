# end-of-session check on one MI355X: smoke, the whole GPU suite, the full bench line;  bash profiles/scripts/tests_and_bench.sh OUTDIR
OUT=${1:?usage: tests_and_bench.sh OUTDIR}; mkdir -p "$OUT"
python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" 2>&1 | tail -2
timeout 1800 python -m pytest tests -q -m gpu > "$OUT/pytest_gpu.txt" 2>&1; grep "passed\|failed\|^FAILED" "$OUT/pytest_gpu.txt" | tail -8
python bench.py --full > "$OUT/bench.json" 2> "$OUT/bench.err"; tail -c 300 "$OUT/bench.json"
