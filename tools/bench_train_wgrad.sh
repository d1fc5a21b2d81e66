#!/bin/bash
# The weight-gradient kernel's A/B on whole training steps: tools/bench_train.py at batch 32 and 128 with LDN_WGRAD=0 (the gather +
# PyTorch GEMM path) and LDN_WGRAD=1 (ldn_wgrad_rows), three runs each, alternating, on ONE box in ONE session; then a rocprofv3 --kernel-trace
# --stats summary of one timed step per setting.  Run from the repository root on an MI355X:  bash tools/bench_train_wgrad.sh [outdir]
#   -> <outdir>/train_step_wgrad.jsonl          every line of every run, then one median line per (batch, workload)
#   -> <outdir>/train_wgrad_kernel_stats.txt    per setting: the kernels of `--batch 32 --warmup 1 --steps 1` (the calibration forwards included)
# Every GPU step runs under its own time limit and the script stops at the first one that fails.
set -eo pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${1:-$R/profiles}
mkdir -p "$OUT"
JL=$OUT/train_step_wgrad.jsonl
: > "$JL"
for batch in 32 128; do
  for run in 1 2 3; do
    for on in 0 1; do
      LDN_WGRAD=$on timeout -k 10 420 python "$R/tools/bench_train.py" --batch $batch --no-reference | tee -a "$JL"
    done
  done
done
python - "$JL" <<'PY'
import json, statistics, sys
lines = [json.loads(l) for l in open(sys.argv[1]) if l.startswith("{")]
out = open(sys.argv[1], "a")
for key in sorted({(d["batch"], d["workload"]) for d in lines}):
    pick = lambda on, f: [d["hip_row_kernels"][f] for d in lines if (d["batch"], d["workload"]) == key and d["wgrad_kernel"] == on]
    print(json.dumps({"summary": "medians of the runs above", "batch": key[0], "workload": key[1],
                      "median_ms_per_step_wgrad_off": round(statistics.median(pick(False, "ms_per_step")), 2),
                      "median_ms_per_step_wgrad_on": round(statistics.median(pick(True, "ms_per_step")), 2),
                      "peak_MiB_one_step_wgrad_off": max(pick(False, "peak_MiB_one_step")), "peak_MiB_one_step_wgrad_on": max(pick(True, "peak_MiB_one_step"))}), file=out)
PY
STATS=$OUT/train_wgrad_kernel_stats.txt
: > "$STATS"
for on in 0 1; do
  D=$(mktemp -d)
  (cd "$D" && LDN_WGRAD=$on timeout -k 10 600 rocprofv3 --kernel-trace --stats -d "$D" -o r -- python "$R/tools/bench_train.py" --batch 32 --warmup 1 --steps 1 --no-reference > "$D/log.txt" 2>&1)
  echo "== LDN_WGRAD=$on: tools/bench_train.py --batch 32 --warmup 1 --steps 1 --no-reference (layer, spatial, channel; per workload 1 warm-up + 1 timed + 1 peak-memory step, and the maskers' calibration forwards)" >> "$STATS"
  python "$R/tools/rocpd_stats.py" "$(find "$D" -name '*.db' | head -1)" 25 >> "$STATS"
  rm -rf "$D"
done
