#!/bin/bash
# Two split blocks per accumulator in the matcher's DB pass (profiles/match_pairs.json), in parts so that each fits one GPU visit:
#   model     tools/mfma_valu_overlap pairs (built beforehand: see its first lines): today's split-2 block (p0) against the paired
#             lines p1 .. p3, three alternating turns, then the exactness of the packing on the device
#   clock     the same lines under rocprofv3 --pmc GRBM_GUI_ACTIVE, a run of its own: cycles per block and SIMD
#   forms     split 2 at 32 000 x 1M: this library, this library with TODHIP_K4X_PAIRS=0 and PARENT_LIB, alternating, three turns;
#             then split 3 and whole blocks (the parent's code), this library against PARENT_LIB
#   sizes     1, 2, 4, 8, 16 frames, adaptive block form, alternating
#   prio      split 2 at 32 000 x 1M with and without the static priority (NOPRIO_LIB: a build with -DTOD_K4X_STATIC_PRIO=0), alternating
#   profile   rocprofv3 on tools/k4x_one.py at 32 x 1000 queries, split 2: kernel trace, then each counter set in a run of its own
#   bench     python bench.py, five runs each, alternating; then --dump-outputs of both, compared array for array
#   full      python bench.py --full --extras chained --no-cpu-baseline, one run each
# PARENT_LIB: a build of the parent commit's library (TODHIP_LIB_PATH); without it only this library runs. Output: $OUT/pairs_* (OUT, default bench_out).
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT:-$PWD/bench_out}; mkdir -p "$OUT"
export TMPDIR=/tmp
libs="child"; [ -n "$PARENT_LIB" ] && libs="parent child"
with_lib() {
  case $1 in
    parent) TODHIP_LIB_PATH="$PARENT_LIB" "${@:2}" ;;
    noprio) TODHIP_LIB_PATH="$NOPRIO_LIB" "${@:2}" ;;
    pairs0) env -u TODHIP_LIB_PATH TODHIP_K4X_PAIRS=0 "${@:2}" ;;
    *) env -u TODHIP_LIB_PATH "${@:2}" ;;
  esac
}
stop() { echo "stopped: $1 ended with status $2"; exit 1; }
# a bench.py result line, shortened to what this record keeps
SHORT='import json, sys
d = json.loads(sys.stdin.read()); c = d.get("chained") or {}
print(json.dumps({"value": d["value"], "ms_per_step": d["ms_per_step"], "launch_ms": d["roofline"]["launch_ms"], "stage_ms_per_step": d["config"].get("stage_ms_per_step"),
                  "chained": {k: c[k] for k in ("frames_per_s", "matcher_launch_ms", "ms_per_step") if k in c}}))'
for part in "$@"; do
  case $part in
  model)
    timeout -k 10 120 tools/mfma_valu_overlap pairs 3 2>&1 | tee "$OUT/pairs_model.txt"; s=${PIPESTATUS[0]}; [ "$s" = 0 ] || stop model "$s" ;;
  clock)
    timeout -k 10 200 rocprofv3 --pmc GRBM_GUI_ACTIVE --output-format csv -d "$OUT/pairs_model_clock" -- tools/mfma_valu_overlap pairs 3 > "$OUT/pairs_model_clock.log" 2>&1 || stop "clock model" $?
    python3 - "$OUT" <<'PY' | tee "$OUT/pairs_clock.txt"
import csv, glob, os, re, sys
out = sys.argv[1]
blocks = 2.0 * 2048 * 6                                                        # per SIMD and launch: two waves, 2048 steps of six blocks
for f in sorted(glob.glob(os.path.join(out, "pairs_model_clock", "**", "*counter_collection.csv"), recursive=True), key=os.path.getmtime)[-1:]:
    rows, order = {}, []
    for row in csv.DictReader(open(f)):
        name = row["Kernel_Name"]
        if not name.startswith("void kq<"): continue
        if name not in rows: rows[name] = []; order.append(name)
        rows[name].append((float(row["Counter_Value"]) / 8.0, float(row["End_Timestamp"]) - float(row["Start_Timestamp"])))
    for name in order:
        timed = [r for i, r in enumerate(rows[name][-21:]) if i % 7]           # three turns of 1 + 6 launches behind the warm-up: the timed ones
        turns = [sorted(timed[6 * t:6 * t + 6], key=lambda x: x[1])[0] for t in range(len(timed) // 6)]
        print("%-6s " % re.match(r"void (kq<\d>)", name).group(1) + "  ".join("%.4f ms %.3f GHz %5.1f cycles" % (r[1] * 1e-6, r[0] / r[1], r[0] / blocks) for r in turns))
PY
    ;;
  forms)
    for round in 1 2 3; do for which in $libs pairs0; do
      echo -n "split 2 $which: "; with_lib $which env B=32 TODHIP_K4X_HALF=2 timeout -k 10 200 python tools/k4x_one.py mfma 2>&1 | tail -1; s=${PIPESTATUS[0]}; [ "$s" = 0 ] || stop "forms 2 $which" "$s"
    done; done | tee "$OUT/pairs_forms.txt"; [ "${PIPESTATUS[0]}" = 0 ] || exit 1
    for half in 3 0; do for round in 1 2; do for which in $libs; do
      echo -n "split $half $which: "; with_lib $which env B=32 TODHIP_K4X_HALF=$half timeout -k 10 200 python tools/k4x_one.py mfma 2>&1 | tail -1; s=${PIPESTATUS[0]}; [ "$s" = 0 ] || stop "forms $half $which" "$s"
    done; done; done | tee -a "$OUT/pairs_forms.txt"; [ "${PIPESTATUS[0]}" = 0 ] || exit 1 ;;
  sizes)
    for B in 1 2 4 8 16; do for round in 1 2; do for which in $libs; do
      echo -n "frames $B $which: "; with_lib $which env B=$B timeout -k 10 200 python tools/k4x_one.py mfma 2>&1 | tail -1; s=${PIPESTATUS[0]}; [ "$s" = 0 ] || stop "sizes $B $which" "$s"
    done; done; done | tee "$OUT/pairs_sizes.txt"; [ "${PIPESTATUS[0]}" = 0 ] || exit 1 ;;
  prio)
    [ -n "$NOPRIO_LIB" ] || stop "prio: NOPRIO_LIB is not set" 1
    for round in 1 2 3; do for which in child noprio; do
      echo -n "split 2 $which: "; with_lib $which env B=32 TODHIP_K4X_HALF=2 timeout -k 10 200 python tools/k4x_one.py mfma 2>&1 | tail -1; s=${PIPESTATUS[0]}; [ "$s" = 0 ] || stop "prio $which" "$s"
    done; done | tee "$OUT/pairs_prio.txt"; [ "${PIPESTATUS[0]}" = 0 ] || exit 1 ;;
  profile)
    for which in $libs; do
      with_lib $which env B=32 TODHIP_K4X_HALF=2 timeout -k 10 280 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/pairs_${which}_trace" -- python3 tools/k4x_one.py mfma > "$OUT/pairs_${which}_trace.log" 2>&1 || stop "trace $which" $?
      with_lib $which env B=32 TODHIP_K4X_HALF=2 timeout -k 10 280 rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_MFMA --output-format csv -d "$OUT/pairs_${which}_pmc1" -- python3 tools/k4x_one.py mfma > "$OUT/pairs_${which}_pmc1.log" 2>&1 || stop "pmc1 $which" $?
      with_lib $which env B=32 TODHIP_K4X_HALF=2 timeout -k 10 280 rocprofv3 --pmc SQ_BUSY_CYCLES GRBM_GUI_ACTIVE --output-format csv -d "$OUT/pairs_${which}_pmc2" -- python3 tools/k4x_one.py mfma > "$OUT/pairs_${which}_pmc2.log" 2>&1 || stop "pmc2 $which" $?
    done
    python3 - "$OUT" $libs <<'PY' | tee "$OUT/pairs_profile.txt"
import csv, glob, os, sys
out, libs = sys.argv[1], sys.argv[2:]
newest = lambda files: sorted(files, key=os.path.getmtime)[-1:]
for which in libs:
    for f in newest(glob.glob(os.path.join(out, "pairs_%s_trace" % which, "**", "*kernel_stats.csv"), recursive=True)):
        for row in csv.DictReader(open(f)):
            if "hamming_topk" in row["Name"]: print("%s %-70s calls %s avg %s ns pct %s" % (which, row["Name"][:70], row["Calls"], row["AverageNs"], row["Percentage"]))
    for d in ("pmc1", "pmc2"):
        for f in newest(glob.glob(os.path.join(out, "pairs_%s_%s" % (which, d), "**", "*counter_collection.csv"), recursive=True)):
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
      echo -n "bench $which: "; with_lib $which timeout -k 10 300 python bench.py 2>&1 | grep '^{' | tail -1 | python3 -c "$SHORT"; s=${PIPESTATUS[0]}; [ "$s" = 0 ] || stop "bench $which" "$s"
    done; done | tee "$OUT/pairs_bench.txt"; [ "${PIPESTATUS[0]}" = 0 ] || exit 1
    for which in $libs; do
      with_lib $which timeout -k 10 300 python bench.py --steps 20 --warmup 3 --dump-outputs "$OUT/pairs_dump_$which" > "$OUT/pairs_dump_$which.log" 2>&1 || stop "dump $which" $?
    done
    [ -n "$PARENT_LIB" ] && python3 - "$OUT" <<'PY' | tee "$OUT/pairs_dump.txt"
import glob, os, sys
import numpy as np
out = sys.argv[1]
names = sorted(os.path.basename(f) for f in glob.glob(os.path.join(out, "pairs_dump_parent", "*.npy")))
diff = [n for n in names if not np.array_equal(np.load(os.path.join(out, "pairs_dump_parent", n)), np.load(os.path.join(out, "pairs_dump_child", n)))]
print("%d arrays, different: %s" % (len(names), diff))
PY
    ;;
  full)
    for which in $libs; do
      echo -n "full $which: "; with_lib $which timeout -k 10 500 python bench.py --full --extras chained --no-cpu-baseline 2>&1 | grep '^{' | tail -1 | tee "$OUT/pairs_full_$which.json" | python3 -c "$SHORT"; s=${PIPESTATUS[0]}; [ "$s" = 0 ] || stop "full $which" "$s"
    done | tee -a "$OUT/pairs_full.txt"; [ "${PIPESTATUS[0]}" = 0 ] || exit 1 ;;
  *) echo "unknown part $part"; exit 1 ;;
  esac
done
