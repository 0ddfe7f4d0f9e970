#!/bin/bash
# The paired split-2 trip of the matcher's DB pass without the periodic exchange of bounds (profiles/match_hot_trip.json), in parts so
# that each fits one GPU visit. PARENT_LIB: a build of the parent commit's library (TODHIP_LIB_PATH); without it only this library runs.
#   trip      tools/k4x_trip_counts.py on the paired forms (no GPU)
#   step0     PARENT_LIB alone, split 2 at 32 000 x 1M: the default against TODHIP_K4X_SHARE=1000000 (the exchange never runs after the
#             first trip, its code and the copies at the back edge stay), three alternating turns; then SQ_INSTS_VALU of the second
#             under rocprofv3 --pmc, a run of its own (the default's comes with `profile`)
#   forms     split 2 at 32 000 x 1M, this library against PARENT_LIB, alternating, three turns; then split 3 and whole blocks
#   sizes     1, 2, 4, 8, 16 frames, adaptive block form, alternating
#   profile   rocprofv3 on tools/k4x_one.py at 32 x 1000 queries, split 2: kernel trace, then each counter set in a run of its own
#   bench     python bench.py, five runs each, alternating; then --dump-outputs of both, compared array for array
#   full      python bench.py --full --extras chained --no-cpu-baseline, FULL_RUNS (2) runs each, alternating
#   chained   the pass on the chained block's DB with split 2 forced (tools/k4x_on_chained_db.py): the dense case
# Output: $OUT/hot_* (OUT, default bench_out).
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT:-$PWD/bench_out}; mkdir -p "$OUT"
export TMPDIR=/tmp
libs="child"; [ -n "$PARENT_LIB" ] && libs="parent child"
with_lib() {
  case $1 in
    parent) ( export TODHIP_LIB_PATH="$PARENT_LIB"; "${@:2}" ) ;;
    *) ( unset TODHIP_LIB_PATH; "${@:2}" ) ;;
  esac
}
stop() { echo "stopped: $1 ended with status $2"; exit 1; }
one() { env "$@" timeout -k 10 200 python tools/k4x_one.py mfma 2>&1 | tail -1; return "${PIPESTATUS[0]}"; }
SHORT='import json, sys
d = json.loads(sys.stdin.read()); c = d.get("chained") or {}
print(json.dumps({"value": d["value"], "ms_per_step": d["ms_per_step"], "launch_ms": d["roofline"]["launch_ms"], "stage_ms_per_step": d["config"].get("stage_ms_per_step"),
                  "chained": {k: c[k] for k in ("frames_per_s", "matcher_launch_ms", "ms_per_step") if k in c}}))'
PMC='import csv, glob, os, sys
out, tags = sys.argv[1], sys.argv[2:]
for tag in tags:
    for f in sorted(glob.glob(os.path.join(out, tag, "**", "*counter_collection.csv"), recursive=True), key=os.path.getmtime)[-1:]:
        acc, n = {}, {}
        for row in csv.DictReader(open(f)):
            if "hamming_topk" not in row["Kernel_Name"]: continue
            key = (row["Kernel_Name"][:60], row["Counter_Name"])
            acc[key] = acc.get(key, 0.0) + float(row["Counter_Value"]); n.setdefault(key, set()).add(row["Dispatch_Id"])
        for key in sorted(acc): print("%s %s %-20s %.6g per launch (%d launches)" % (tag, key[0], key[1], acc[key] / len(n[key]), len(n[key])))
    for f in sorted(glob.glob(os.path.join(out, tag, "**", "*kernel_stats.csv"), recursive=True), key=os.path.getmtime)[-1:]:
        for row in csv.DictReader(open(f)):
            if "hamming_topk" in row["Name"]: print("%s %-70s calls %s avg %s ns pct %s" % (tag, row["Name"][:70], row["Calls"], row["AverageNs"], row["Percentage"]))'
for part in "$@"; do
  case $part in
  trip)
    python tools/k4x_trip_counts.py 2,6,2 5,6,2 2,4,2 | tee "$OUT/hot_trip.txt"; [ "${PIPESTATUS[0]}" = 0 ] || exit 1 ;;
  step0)
    [ -n "$PARENT_LIB" ] || stop "step0: PARENT_LIB is not set" 1
    for round in 1 2 3; do for share in 16 1000000; do
      echo -n "parent split 2 share $share: "; with_lib parent one B=32 TODHIP_K4X_HALF=2 TODHIP_K4X_SHARE=$share; s=$?; [ "$s" = 0 ] || stop "step0 $share" "$s"
    done; done | tee "$OUT/hot_step0.txt"; [ "${PIPESTATUS[0]}" = 0 ] || exit 1
    with_lib parent env B=32 TODHIP_K4X_HALF=2 TODHIP_K4X_SHARE=1000000 timeout -k 10 280 rocprofv3 --pmc SQ_INSTS_VALU --output-format csv -d "$OUT/hot_parent_noshare_pmc" -- python3 tools/k4x_one.py mfma > "$OUT/hot_parent_noshare_pmc.log" 2>&1 || stop "step0 pmc" $?
    python3 -c "$PMC" "$OUT" hot_parent_noshare_pmc | tee -a "$OUT/hot_step0.txt" ;;
  forms)
    for round in 1 2 3; do for which in $libs; do
      echo -n "split 2 $which: "; with_lib $which one B=32 TODHIP_K4X_HALF=2; s=$?; [ "$s" = 0 ] || stop "forms 2 $which" "$s"
    done; done | tee "$OUT/hot_forms.txt"; [ "${PIPESTATUS[0]}" = 0 ] || exit 1
    for half in 3 0; do for round in 1 2; do for which in $libs; do
      echo -n "split $half $which: "; with_lib $which one B=32 TODHIP_K4X_HALF=$half; s=$?; [ "$s" = 0 ] || stop "forms $half $which" "$s"
    done; done; done | tee -a "$OUT/hot_forms.txt"; [ "${PIPESTATUS[0]}" = 0 ] || exit 1 ;;
  sizes)
    for B in 1 2 4 8 16; do for round in 1 2; do for which in $libs; do
      echo -n "frames $B $which: "; with_lib $which one B=$B; s=$?; [ "$s" = 0 ] || stop "sizes $B $which" "$s"
    done; done; done | tee "$OUT/hot_sizes.txt"; [ "${PIPESTATUS[0]}" = 0 ] || exit 1 ;;
  profile)
    tags=""
    for which in $libs; do
      with_lib $which env B=32 TODHIP_K4X_HALF=2 timeout -k 10 280 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/hot_${which}_trace" -- python3 tools/k4x_one.py mfma > "$OUT/hot_${which}_trace.log" 2>&1 || stop "trace $which" $?
      with_lib $which env B=32 TODHIP_K4X_HALF=2 timeout -k 10 280 rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_VMEM_RD --output-format csv -d "$OUT/hot_${which}_pmc1" -- python3 tools/k4x_one.py mfma > "$OUT/hot_${which}_pmc1.log" 2>&1 || stop "pmc1 $which" $?
      with_lib $which env B=32 TODHIP_K4X_HALF=2 timeout -k 10 280 rocprofv3 --pmc SQ_BUSY_CYCLES --output-format csv -d "$OUT/hot_${which}_pmc2" -- python3 tools/k4x_one.py mfma > "$OUT/hot_${which}_pmc2.log" 2>&1 || stop "pmc2 $which" $?
      tags="$tags hot_${which}_trace hot_${which}_pmc1 hot_${which}_pmc2"
    done
    python3 -c "$PMC" "$OUT" $tags | tee "$OUT/hot_profile.txt" ;;
  bench)
    for round in 1 2 3 4 5; do for which in $libs; do
      echo -n "bench $which: "; with_lib $which timeout -k 10 300 python bench.py 2>&1 | grep '^{' | tail -1 | python3 -c "$SHORT"; s=${PIPESTATUS[0]}; [ "$s" = 0 ] || stop "bench $which" "$s"
    done; done | tee "$OUT/hot_bench.txt"; [ "${PIPESTATUS[0]}" = 0 ] || exit 1
    for which in $libs; do
      with_lib $which timeout -k 10 300 python bench.py --steps 20 --warmup 3 --dump-outputs "$OUT/hot_dump_$which" > "$OUT/hot_dump_$which.log" 2>&1 || stop "dump $which" $?
    done
    [ -n "$PARENT_LIB" ] && python3 - "$OUT" <<'PY' | tee "$OUT/hot_dump.txt"
import glob, os, sys
import numpy as np
out = sys.argv[1]
names = sorted(os.path.basename(f) for f in glob.glob(os.path.join(out, "hot_dump_parent", "*.npy")))
diff = [n for n in names if not np.array_equal(np.load(os.path.join(out, "hot_dump_parent", n)), np.load(os.path.join(out, "hot_dump_child", n)))]
print("%d arrays, different: %s" % (len(names), diff))
PY
    ;;
  full)
    for round in $(seq 1 "${FULL_RUNS:-2}"); do for which in $libs; do
      echo -n "full $which: "; with_lib $which timeout -k 10 500 python bench.py --full --extras chained --no-cpu-baseline 2>&1 | grep '^{' | tail -1 | python3 -c "$SHORT"; s=${PIPESTATUS[0]}; [ "$s" = 0 ] || stop "full $which" "$s"
    done; done | tee "$OUT/hot_full.txt"; [ "${PIPESTATUS[0]}" = 0 ] || exit 1 ;;
  chained)
    for which in $libs; do
      echo -n "chained DB, split 2 $which: "; with_lib $which env ONLY_CHAINED=1 TODHIP_K4X_HALF=2 timeout -k 10 280 python tools/k4x_on_chained_db.py 2>&1 | grep '^chained_db' | tail -1; s=${PIPESTATUS[0]}; [ "$s" = 0 ] || stop "chained $which" "$s"
    done | tee "$OUT/hot_chained.txt"; [ "${PIPESTATUS[0]}" = 0 ] || exit 1 ;;
  *) echo "unknown part $part"; exit 1 ;;
  esac
done
