#!/bin/bash
# The split forms of the matcher's DB pass with their tails loaded on demand (hamming_topk_fp4rows, profiles/match_tails.json), against
# a build of the parent commit's library, in parts so that each fits one GPU visit:
#   forms     split 2, split 3, whole blocks forced at 32 000 x 1M, three alternating turns each
#   sizes     1, 2, 4, 8, 16 frames, adaptive block form, two alternating turns each
#   profile   rocprofv3 on tools/k4x_one.py at 32 x 1000 queries, split 2: kernel trace, then each counter set in a run of its own
#   bench     python bench.py, five runs each, alternating; then --dump-outputs of both, compared array for array
#   full      python bench.py --full --extras chained --no-cpu-baseline, one run each
# PARENT_LIB: a build of the parent commit's library (TODHIP_LIB_PATH); without it only this library runs. Output: $OUT/tails_* (OUT, default bench_out).
# A part that fails ends the script: nothing more is started on the GPU behind it.
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT:-$PWD/bench_out}; mkdir -p "$OUT"
export TMPDIR=/tmp
libs="child"; [ -n "$PARENT_LIB" ] && libs="parent child"
with_lib() { if [ "$1" = parent ]; then TODHIP_LIB_PATH="$PARENT_LIB" "${@:2}"; else env -u TODHIP_LIB_PATH "${@:2}"; fi; }
stop() { echo "stopped: $1 ended with status $2"; exit 1; }
# a bench.py result line, shortened to what this record keeps
SHORT='import json, sys
d = json.loads(sys.stdin.read()); c = d.get("chained") or {}
print(json.dumps({"value": d["value"], "ms_per_step": d["ms_per_step"], "launch_ms": d["roofline"]["launch_ms"], "frames_per_s": d["repeats"]["frames_per_s"],
                  "chained": {k: c[k] for k in ("frames_per_s", "matcher_launch_ms", "ms_per_step") if k in c}}))'
one() { with_lib "$1" env "${@:2}" timeout -k 10 200 python tools/k4x_one.py mfma > "$OUT/tails_one.tmp" 2>&1 || return $?; tail -1 "$OUT/tails_one.tmp"; }
for part in "$@"; do
  case $part in
  forms)
    for half in 2 3 0; do for round in 1 2 3; do for which in $libs; do
      echo -n "split $half $which: " >> "$OUT/tails_forms.txt"; one $which B=32 TODHIP_K4X_HALF=$half >> "$OUT/tails_forms.txt" || stop "forms $half $which" $?
    done; done; done; cat "$OUT/tails_forms.txt" ;;
  sizes)
    for B in 1 2 4 8 16; do for round in 1 2; do for which in $libs; do
      echo -n "frames $B $which: " >> "$OUT/tails_sizes.txt"; one $which B=$B >> "$OUT/tails_sizes.txt" || stop "sizes $B $which" $?
    done; done; done; cat "$OUT/tails_sizes.txt" ;;
  profile)
    for which in $libs; do
      with_lib $which env B=32 TODHIP_K4X_HALF=2 timeout -k 10 280 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/tails_${which}_trace" -- python3 tools/k4x_one.py mfma > "$OUT/tails_${which}_trace.log" 2>&1 || stop "trace $which" $?
      with_lib $which env B=32 TODHIP_K4X_HALF=2 timeout -k 10 280 rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_VMEM_RD SQ_INSTS_MFMA --output-format csv -d "$OUT/tails_${which}_pmc1" -- python3 tools/k4x_one.py mfma > "$OUT/tails_${which}_pmc1.log" 2>&1 || stop "pmc1 $which" $?
      with_lib $which env B=32 TODHIP_K4X_HALF=2 timeout -k 10 280 rocprofv3 --pmc SQ_BUSY_CYCLES --output-format csv -d "$OUT/tails_${which}_pmc2" -- python3 tools/k4x_one.py mfma > "$OUT/tails_${which}_pmc2.log" 2>&1 || stop "pmc2 $which" $?
    done
    python3 - "$OUT" $libs <<'PY' | tee "$OUT/tails_profile.txt"
import csv, glob, os, sys
out, libs = sys.argv[1], sys.argv[2:]
newest = lambda files: sorted(files, key=os.path.getmtime)[-1:]
for which in libs:
    for f in newest(glob.glob(os.path.join(out, "tails_%s_trace" % which, "**", "*kernel_stats.csv"), recursive=True)):
        for row in csv.DictReader(open(f)):
            if "hamming_topk" in row["Name"]: print("%s %-70s calls %s avg %s ns pct %s" % (which, row["Name"][:70], row["Calls"], row["AverageNs"], row["Percentage"]))
    for d in ("pmc1", "pmc2"):
        for f in newest(glob.glob(os.path.join(out, "tails_%s_%s" % (which, d), "**", "*counter_collection.csv"), recursive=True)):
            acc, n = {}, {}
            for row in csv.DictReader(open(f)):
                if "hamming_topk" not in row["Kernel_Name"]: continue
                key = (row["Kernel_Name"][:60], row["Counter_Name"])
                acc[key] = acc.get(key, 0.0) + float(row["Counter_Value"]); n.setdefault(key, set()).add(row["Dispatch_Id"])
            for key in sorted(acc): print("%s %s %-28s %.6g per launch (%d launches)" % (which, key[0], key[1], acc[key] / len(n[key]), len(n[key])))
PY
    ;;
  bench)
    for round in 1 2 3 4 5; do for which in $libs; do
      with_lib $which timeout -k 10 300 python bench.py > "$OUT/tails_bench.tmp" 2>&1 || stop "bench $which" $?
      echo -n "bench $which: " >> "$OUT/tails_bench.txt"; grep '^{' "$OUT/tails_bench.tmp" | tail -1 | python3 -c "$SHORT" >> "$OUT/tails_bench.txt" || stop "bench line $which" $?
    done; done; cat "$OUT/tails_bench.txt"
    for which in $libs; do
      with_lib $which timeout -k 10 300 python bench.py --steps 20 --warmup 3 --dump-outputs "$OUT/tails_dump_$which" > "$OUT/tails_dump_$which.log" 2>&1 || stop "dump $which" $?
    done
    [ -n "$PARENT_LIB" ] && python3 - "$OUT" <<'PY' | tee "$OUT/tails_dump.txt"
import glob, os, sys
import numpy as np
out = sys.argv[1]
names = sorted(os.path.basename(f) for f in glob.glob(os.path.join(out, "tails_dump_parent", "*.npy")))
diff = [n for n in names if not np.array_equal(np.load(os.path.join(out, "tails_dump_parent", n)), np.load(os.path.join(out, "tails_dump_child", n)))]
print("%d arrays, different: %s" % (len(names), diff))
PY
    ;;
  full)
    for which in $libs; do
      with_lib $which timeout -k 10 500 python bench.py --full --extras chained --no-cpu-baseline > "$OUT/tails_full.tmp" 2>&1 || stop "full $which" $?
      grep '^{' "$OUT/tails_full.tmp" | tail -1 > "$OUT/tails_full_$which.json"
      echo -n "full $which: " >> "$OUT/tails_full.txt"; python3 -c "$SHORT" < "$OUT/tails_full_$which.json" >> "$OUT/tails_full.txt" || stop "full line $which" $?
    done; cat "$OUT/tails_full.txt" ;;
  *) echo "unknown part $part"; exit 1 ;;
  esac
done
