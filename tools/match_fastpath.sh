#!/bin/bash
# The split-block fast path of the matcher's DB pass (hamming_topk_fp4rows, profiles/match_fastpath.json), in parts so that each fits
# one GPU visit:
#   model     tools/mfma_valu_overlap (built beforehand: see its first lines): the fast path's ingredients, ns per block and SIMD
#   profile   rocprofv3 on tools/k4x_one.py at 32 x 1000 queries, split 2: kernel trace, then each counter set in a run of its own
#   forms     split 2, split 3, whole blocks at 32 000 x 1M, this library against PARENT_LIB, alternating
#   sizes     1, 2, 4, 8, 16 frames, adaptive block form, alternating
#   bench     python bench.py, five runs each, alternating; then --dump-outputs of both, compared array for array
#   full      python bench.py --full --extras chained --no-cpu-baseline, one run each
# PARENT_LIB: a build of the parent commit's library (TODHIP_LIB_PATH); without it only this library runs. Output: $OUT/fastpath_* (OUT, default bench_out).
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
for part in "$@"; do
  case $part in
  model)
    timeout -k 10 120 tools/mfma_valu_overlap 2>&1 | tee "$OUT/fastpath_model.txt"; s=${PIPESTATUS[0]}; [ "$s" = 0 ] || stop model "$s" ;;
  profile)
    for which in $libs; do
      with_lib $which env B=32 TODHIP_K4X_HALF=2 timeout -k 10 280 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/fastpath_${which}_trace" -- python3 tools/k4x_one.py mfma > "$OUT/fastpath_${which}_trace.log" 2>&1 || stop "trace $which" $?
      with_lib $which env B=32 TODHIP_K4X_HALF=2 timeout -k 10 280 rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_MFMA --output-format csv -d "$OUT/fastpath_${which}_pmc1" -- python3 tools/k4x_one.py mfma > "$OUT/fastpath_${which}_pmc1.log" 2>&1 || stop "pmc1 $which" $?
      with_lib $which env B=32 TODHIP_K4X_HALF=2 timeout -k 10 280 rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES --output-format csv -d "$OUT/fastpath_${which}_pmc2" -- python3 tools/k4x_one.py mfma > "$OUT/fastpath_${which}_pmc2.log" 2>&1 || stop "pmc2 $which" $?
    done
    python3 - "$OUT" $libs <<'PY' | tee "$OUT/fastpath_profile.txt"
import csv, glob, os, sys
out, libs = sys.argv[1], sys.argv[2:]
newest = lambda files: sorted(files, key=os.path.getmtime)[-1:]
for which in libs:
    for f in newest(glob.glob(os.path.join(out, "fastpath_%s_trace" % which, "**", "*kernel_stats.csv"), recursive=True)):
        for row in csv.DictReader(open(f)):
            if "hamming_topk" in row["Name"]: print("%s %-70s calls %s avg %s ns pct %s" % (which, row["Name"][:70], row["Calls"], row["AverageNs"], row["Percentage"]))
    for d in ("pmc1", "pmc2"):
        for f in newest(glob.glob(os.path.join(out, "fastpath_%s_%s" % (which, d), "**", "*counter_collection.csv"), recursive=True)):
            acc, n = {}, {}
            for row in csv.DictReader(open(f)):
                if "hamming_topk" not in row["Kernel_Name"]: continue
                key = (row["Kernel_Name"][:60], row["Counter_Name"])
                acc[key] = acc.get(key, 0.0) + float(row["Counter_Value"]); n.setdefault(key, set()).add(row["Dispatch_Id"])
            for key in sorted(acc): print("%s %s %-28s %.6g per launch (%d launches)" % (which, key[0], key[1], acc[key] / len(n[key]), len(n[key])))
PY
    ;;
  clock)
    # the shader clock under each loop: GRBM_GUI_ACTIVE (summed over the 8 XCDs) over the dispatch's own duration, in a run of its own
    timeout -k 10 200 rocprofv3 --pmc GRBM_GUI_ACTIVE --output-format csv -d "$OUT/fastpath_model_clock" -- tools/mfma_valu_overlap > "$OUT/fastpath_model_clock.log" 2>&1 || stop "clock model" $?
    env -u TODHIP_LIB_PATH B=32 TODHIP_K4X_HALF=2 timeout -k 10 280 rocprofv3 --pmc GRBM_GUI_ACTIVE --output-format csv -d "$OUT/fastpath_child_clock" -- python3 tools/k4x_one.py mfma > "$OUT/fastpath_child_clock.log" 2>&1 || stop "clock product" $?
    python3 - "$OUT" <<'PY' | tee "$OUT/fastpath_clock.txt"
import csv, glob, os, sys
out = sys.argv[1]
newest = lambda files: sorted(files, key=os.path.getmtime)[-1:]
for d, blocks in (("fastpath_model_clock", 2.0 * 2048 * 6), ("fastpath_child_clock", 31.25e6 / 1024)):
    for f in newest(glob.glob(os.path.join(out, d, "**", "*counter_collection.csv"), recursive=True)):
        rows, order = {}, []
        for row in csv.DictReader(open(f)):
            name = row["Kernel_Name"]
            if not (name.startswith("void kp<") or "hamming_topk" in name): continue
            if name not in rows: rows[name] = []; order.append(name)
            rows[name].append((float(row["Counter_Value"]) / 8.0, float(row["End_Timestamp"]) - float(row["Start_Timestamp"])))
        for name in order:
            r = sorted(rows[name][1:] or rows[name], key=lambda x: x[1])[0]            # the fastest dispatch behind the first
            print("%-62s %.4f ms  %.3f GHz  %5.1f ns = %5.1f cycles per block and SIMD" % (name[:62], r[1] * 1e-6, r[0] / r[1], r[1] / blocks, r[0] / blocks))
PY
    ;;
  forms)
    for half in 2 3 0; do for round in 1 2 3; do for which in $libs; do
      echo -n "split $half $which: "; with_lib $which env B=32 TODHIP_K4X_HALF=$half timeout -k 10 200 python tools/k4x_one.py mfma 2>&1 | tail -1; s=${PIPESTATUS[0]}; [ "$s" = 0 ] || stop "forms $half $which" "$s"
    done; done; done | tee "$OUT/fastpath_forms.txt"; [ "${PIPESTATUS[0]}" = 0 ] || exit 1 ;;
  sizes)
    for B in 1 2 4 8 16; do for round in 1 2; do for which in $libs; do
      echo -n "frames $B $which: "; with_lib $which env B=$B timeout -k 10 200 python tools/k4x_one.py mfma 2>&1 | tail -1; s=${PIPESTATUS[0]}; [ "$s" = 0 ] || stop "sizes $B $which" "$s"
    done; done; done | tee "$OUT/fastpath_sizes.txt"; [ "${PIPESTATUS[0]}" = 0 ] || exit 1 ;;
  bench)
    for round in 1 2 3 4 5; do for which in $libs; do
      echo -n "bench $which: "; with_lib $which timeout -k 10 300 python bench.py 2>&1 | grep '^{' | tail -1 | python3 -c "$SHORT"; s=${PIPESTATUS[0]}; [ "$s" = 0 ] || stop "bench $which" "$s"
    done; done | tee "$OUT/fastpath_bench.txt"; [ "${PIPESTATUS[0]}" = 0 ] || exit 1
    for which in $libs; do
      with_lib $which timeout -k 10 300 python bench.py --steps 20 --warmup 3 --dump-outputs "$OUT/fastpath_dump_$which" > "$OUT/fastpath_dump_$which.log" 2>&1 || stop "dump $which" $?
    done
    [ -n "$PARENT_LIB" ] && python3 - "$OUT" <<'PY' | tee "$OUT/fastpath_dump.txt"
import glob, os, sys
import numpy as np
out = sys.argv[1]
names = sorted(os.path.basename(f) for f in glob.glob(os.path.join(out, "fastpath_dump_parent", "*.npy")))
diff = [n for n in names if not np.array_equal(np.load(os.path.join(out, "fastpath_dump_parent", n)), np.load(os.path.join(out, "fastpath_dump_child", n)))]
print("%d arrays, different: %s" % (len(names), diff))
PY
    ;;
  full)
    for which in $libs; do
      echo -n "full $which: "; with_lib $which timeout -k 10 500 python bench.py --full --extras chained --no-cpu-baseline 2>&1 | grep '^{' | tail -1 | tee "$OUT/fastpath_full_$which.json" | python3 -c "$SHORT"; s=${PIPESTATUS[0]}; [ "$s" = 0 ] || stop "full $which" "$s"
    done | tee "$OUT/fastpath_full.txt"; [ "${PIPESTATUS[0]}" = 0 ] || exit 1 ;;
  *) echo "unknown part $part"; exit 1 ;;
  esac
done
