set -u
cd "${GRAFT_REPO_ROOT:-/root/repo}"; mkdir -p gpurun_out
timeout -k 10 600 python -u -m pytest tests/test_gpu_parity.py tests/test_capi.py -m gpu -x -q --timeout 120 --timeout-method thread -p no:cacheprovider > gpurun_out/pytest_parity.log 2>&1
rc=$?; tail -3 gpurun_out/pytest_parity.log; [ $rc -eq 0 ] || exit $rc
OUT=${GGS_OUT_DIR:-out}; mkdir -p "$OUT"   # logs of this run
timeout -k 10 300 python bench.py --full --steps 30 --warmup 5 --no-cpu-baseline > "$OUT/bench.log" 2>&1 || exit $?
python3 -c "import json; d=json.loads(open('$OUT/bench.log').read().strip().splitlines()[-1]); print(d['value'], d['value_one_stream'], d['value_with_readback'], d['host_api_renders_per_s'])"
