#!/bin/bash
# The driver's multi-GPU bench command with ONE rank over RCCL (nccl backend,
# native communicator, every round form, the parity phase, and with --full
# config 5): what bench.py --gpus N --full runs on an 8-GPU node, minus the
# cross-GPU traffic.
set -o pipefail
cd "$(dirname "$0")/.."
OUT="${FA_OUT_DIR:-bench_out}"
mkdir -p "$OUT"
FA_BENCH_STACK_DUMP_S=200 timeout -k 10 400 python3 -m torch.distributed.run --nnodes 1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29517 bench.py --gpus 1 --multi-rehearsal --full --steps 20 --warmup 5 > "$OUT/multi_rehearsal.json" 2> "$OUT/multi_rehearsal.err" || exit $?
python3 - "$OUT/multi_rehearsal.json" <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(d["value"], d["selected_mode"], d["config"]["parallelism"])
for k, v in d["modes"].items():
    print(" ", k, v.get("ms_per_step"), v.get("bit_exact"), v.get("error", ""))
print(json.dumps(d.get("cfg5_feddct_c100_n24_sharded"))[:800])
print("native_comm_error", d.get("native_comm_error"))
PY
