#!/bin/bash
# ORB's vector work beside the matcher (profiles/orb_diet.json), in parts so that each fits one GPU visit:
#   attribution  python bench.py with --stages match | orb,match | match,verify | the default, three alternating turns, this library:
#                roofline.launch_ms and value of each; ORB's share of the DB pass's loss = median(orb,match) - median(match)
#   pmc          rocprofv3 --pmc SQ_INSTS_VALU, a run of its own, on tools/time_orb_batch.py at 32 frames: vector instructions per launch
#   trace        the kernel trace of one batch alone, as tools/profile_orb.sh takes it (the synthetic image, then the chained block's views)
#   batch        tools/time_orb_batch.py at 32 frames, five alternating turns
#   bench        python bench.py, five runs each, alternating; then --dump-outputs of both, compared array for array
#   full         python bench.py --full --extras chained --no-cpu-baseline, one run each
# PARENT_LIB: a build of the parent commit's library (TODHIP_LIB_PATH); without it only this library runs. Output: $OUT/diet_* (OUT, default bench_out).
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT:-$PWD/bench_out}; mkdir -p "$OUT"
export TMPDIR=/tmp
libs="child"; [ -n "$PARENT_LIB" ] && libs="parent child"
with_lib() {
  case $1 in
    parent) TODHIP_LIB_PATH="$PARENT_LIB" "${@:2}" ;;
    *) env -u TODHIP_LIB_PATH "${@:2}" ;;
  esac
}
stop() { echo "stopped: $1 ended with status $2"; exit 1; }
SHORT='import json, sys
d = json.loads(sys.stdin.read()); c = d.get("chained") or {}
print(json.dumps({"value": d["value"], "ms_per_step": d["ms_per_step"], "launch_ms": d["roofline"]["launch_ms"], "stage_ms_per_step": d["config"].get("stage_ms_per_step"),
                  "chained": {k: c[k] for k in ("frames_per_s", "matcher_launch_ms", "ms_per_step", "stage_ms_per_step") if k in c}}))'
for part in "$@"; do
  case $part in
  attribution)
    for round in 1 2 3; do for stages in match orb,match match,verify orb,match,verify; do
      echo -n "stages $stages: "; env -u TODHIP_LIB_PATH timeout -k 10 300 python bench.py --stages $stages 2>&1 | grep '^{' | tail -1 | python3 -c "$SHORT"; s=${PIPESTATUS[0]}; [ "$s" = 0 ] || stop "attribution $stages" "$s"
    done; done | tee "$OUT/diet_attribution.txt"; [ "${PIPESTATUS[0]}" = 0 ] || exit 1 ;;
  pmc)
    for which in $libs; do
      with_lib $which env B=32 timeout -k 10 280 rocprofv3 --pmc SQ_INSTS_VALU --output-format csv -d "$OUT/diet_${which}_pmc" -- python3 tools/time_orb_batch.py > "$OUT/diet_${which}_pmc.log" 2>&1 || stop "pmc $which" $?
    done
    python3 - "$OUT" $libs <<'PY' | tee "$OUT/diet_pmc.txt"
import csv, glob, os, sys
out, libs = sys.argv[1], sys.argv[2:]
for which in libs:
    for f in sorted(glob.glob(os.path.join(out, "diet_%s_pmc" % which, "**", "*counter_collection.csv"), recursive=True), key=os.path.getmtime)[-1:]:
        acc, n = {}, {}
        for row in csv.DictReader(open(f)):
            name = row["Kernel_Name"].replace("(anonymous namespace)::", "").split("(")[0]
            if "at::" in name or "rocclr" in name: continue
            acc[name] = acc.get(name, 0.0) + float(row["Counter_Value"]); n.setdefault(name, set()).add(row["Dispatch_Id"])
        for name in sorted(acc):                                # 23 batches: resize_kernel is launched twice in each
            print("%s %-28s SQ_INSTS_VALU %.6g per launch, %.6g per batch (%d launches)" % (which, name[:28], acc[name] / len(n[name]), acc[name] / 23, len(n[name])))
        print("%s batch total %.6g" % (which, sum(acc.values()) / 23))
PY
    ;;
  trace)
    for which in $libs; do
      echo "== $which"
      for S in "" 1; do
        tag=orb_synth; [ -n "$S" ] && tag=orb_scenes
        rm -rf "$OUT/diet_${which}_trace_$tag"
        with_lib $which env B=32 SCENES=$S timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/diet_${which}_trace_$tag" -- python3 tools/time_orb_batch.py > "$OUT/diet_${which}_trace_$tag.log" 2>&1 || stop "trace $which $tag" $?
        tail -1 "$OUT/diet_${which}_trace_$tag.log"
        find "$OUT/diet_${which}_trace_$tag" -name "*kernel_stats.csv" | head -1 | xargs -I{} cp {} "$OUT/diet_${which}_${tag}_kernel_stats.csv"
        python3 - "$OUT/diet_${which}_${tag}_kernel_stats.csv" <<'PY'
import csv, sys
tot = 0
for row in csv.DictReader(open(sys.argv[1])):
    n = row["Name"].replace("(anonymous namespace)::", "").split("(")[0]
    if "at::" in n or "rocclr" in n: continue
    per = float(row["TotalDurationNs"]) / 23 / 1e3                                 # 3 + 20 batches per run
    tot += per
    print("  %-28s calls %4s avg %8.1f us   per batch %8.1f us" % (n[:28], row["Calls"], float(row["AverageNs"]) / 1e3, per))
print("  sum per batch %.1f us" % tot)
PY
      done
    done 2>&1 | tee "$OUT/diet_trace.txt"; [ "${PIPESTATUS[0]}" = 0 ] || exit 1 ;;
  batch)
    for round in 1 2 3 4 5; do for which in $libs; do
      echo -n "batch $which: "; with_lib $which env B=32 timeout -k 10 200 python tools/time_orb_batch.py 2>&1 | tail -1; s=${PIPESTATUS[0]}; [ "$s" = 0 ] || stop "batch $which" "$s"
    done; done | tee "$OUT/diet_batch.txt"; [ "${PIPESTATUS[0]}" = 0 ] || exit 1 ;;
  bench)
    for round in 1 2 3 4 5; do for which in $libs; do
      echo -n "bench $which: "; with_lib $which timeout -k 10 300 python bench.py 2>&1 | grep '^{' | tail -1 | python3 -c "$SHORT"; s=${PIPESTATUS[0]}; [ "$s" = 0 ] || stop "bench $which" "$s"
    done; done | tee "$OUT/diet_bench.txt"; [ "${PIPESTATUS[0]}" = 0 ] || exit 1
    for which in $libs; do
      with_lib $which timeout -k 10 300 python bench.py --steps 20 --warmup 3 --dump-outputs "$OUT/diet_dump_$which" > "$OUT/diet_dump_$which.log" 2>&1 || stop "dump $which" $?
    done
    [ -n "$PARENT_LIB" ] && python3 - "$OUT" <<'PY' | tee "$OUT/diet_dump.txt"
import glob, os, sys
import numpy as np
out = sys.argv[1]
names = sorted(os.path.basename(f) for f in glob.glob(os.path.join(out, "diet_dump_parent", "*.npy")))
diff = [n for n in names if not np.array_equal(np.load(os.path.join(out, "diet_dump_parent", n)), np.load(os.path.join(out, "diet_dump_child", n)))]
print("%d arrays, different: %s" % (len(names), diff))
PY
    ;;
  full)
    for which in $libs; do
      echo -n "full $which: "; with_lib $which timeout -k 10 500 python bench.py --full --extras chained --no-cpu-baseline 2>&1 | grep '^{' | tail -1 | tee "$OUT/diet_full_$which.json" | python3 -c "$SHORT"; s=${PIPESTATUS[0]}; [ "$s" = 0 ] || stop "full $which" "$s"
    done | tee -a "$OUT/diet_full.txt"; [ "${PIPESTATUS[0]}" = 0 ] || exit 1 ;;
  *) echo "unknown part $part"; exit 1 ;;
  esac
done
