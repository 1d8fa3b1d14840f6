# forward parity tests + a full bench line without the CPU baseline / training legs; outputs under DIR (default bench_out/TAG)
#   bash tools/quick_check.sh TAG [DIR]
TAG=${1:-quick}
O=${2:-bench_out/$TAG}
mkdir -p $O
timeout 900 python -m pytest tests/test_forward_gpu.py tests/test_ops_gpu.py -q -x -k "not stream_kernel" > $O/fwd_tests.log 2>&1; echo "tests rc=$?"; tail -n 3 $O/fwd_tests.log
timeout 500 python bench.py --full --no-cpu-baseline --no-train > $O/bench_quick.json 2> $O/bench_quick.err; echo "bench rc=$?"
python - "$O" <<'PY'
import json, sys
d = json.loads(open(f"{sys.argv[1]}/bench_quick.json").read().strip().splitlines()[-1])
print("maps/s", round(d["value"], 1), "ms/step", round(d["ms_per_step"], 4), "rel_l1", d.get("rel_l1"), "f16", d.get("f16", {}).get("value"), d.get("f16", {}).get("rel_l1"))
print("latency", d.get("latency"), d["config"].get("lane_choice_ms_per_step"))
print("roofline frac", d["roofline"]["frac"], "dw in_graph", d["dw3x3"].get("in_graph"), d["dw3x3"].get("frac_of_measured_copy_in_graph"))
print("kernel_ms_per_step", d.get("kernel_ms_per_step"))
PY
