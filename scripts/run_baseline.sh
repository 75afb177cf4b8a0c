cd $GRAFT_REPO_ROOT
O=${1:-baseline_out}
mkdir -p "$O"
timeout 1500 python -m pytest tests -m gpu -x -q 2>&1 | tail -15 > "$O/pytest.log"
python bench.py --full --steps 20 --warmup 5 > "$O/bench.json.log" 2> "$O/bench.err"
build/lab_gemm 20 > "$O/lab_gemm.log" 2>&1
tail -5 "$O/pytest.log"; cat "$O/bench.json.log" | cut -c1-1500; tail -3 "$O/lab_gemm.log"
