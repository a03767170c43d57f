#!/bin/bash
# Per-launch durations of one forward (one batch in flight) with the matrix-core convolutions in the int8 form
# (BNN_AMD_MFMA_F4=0) and in the FP4 form (=all), two traces each, taken alternately in one visit:
#   bash tools/f4_trace.sh   then   python tools/f4_trace_table.py   (prints the table of profiles/mfma_f4_kernel_roofline.md)
# Every trace runs under a time limit of its own and the script stops at the first one that fails.
R="$(cd "$(dirname "$0")/.." && pwd)"
OUT="${F4_TRACE_DIR:-$R/build/f4trace}"; rm -rf "$OUT"; mkdir -p "$OUT"   # (build/ is git-ignored)
cd /tmp; export TMPDIR=/tmp
run() {  # tag, switch
  BNN_AMD_MFMA_F4="$2" timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/$1" -o t -- \
    python "$R/bench.py" --steps 20 --warmup 5 --spinup 200 --sustain 0 --streams 1 --no-extras --no-cpu-baseline --no-roofline \
    > "$OUT/$1.log" 2>&1
}
run zero1 0 && run all1 all && run zero2 0 && run all2 all || { echo "f4_trace: a trace failed (see $OUT/*.log)"; exit 1; }
find "$OUT" -name "*kernel_trace.csv" -size +8M -delete
find "$OUT" -name "*.csv" ! -name "*kernel_trace.csv" ! -name "*kernel_stats.csv" -delete
ls "$OUT"
