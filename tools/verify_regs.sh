#!/bin/bash
# Does the hypothesis gate (eval_kernel<false>) cost the DB pass a wave slot because it cannot start beside two of its waves?
# (profiles/verify_regs.json), in parts so that each fits one GPU visit:
#   asm          no GPU: verify.hip and match.hip as gfx950 assembly (the Makefile's flags) in $OUT/vregs_verify.s and vregs_match.s,
#                where the trace part finds the code objects' registers and scratch
#   attribution  python bench.py with --stages match | orb,match | match,verify | the default, three alternating turns, on PARENT_LIB
#                (without it: this library): the verifier's share of roofline.launch_ms = median(match,verify) - median(match)
#   trace        rocprofv3 --kernel-trace of the default bench.py command (the program after --), per library, summarised by
#                tools/verify_regs_trace.py: launches per batch, workgroups, workgroup size, duration beside the matcher, registers,
#                LDS and scratch of every verifier kernel, and the wave-slot estimate of those that do not fit beside two waves of the pass
#   ceiling      the headline with PARENT_LIB (without it: this library) and CAPPED_LIB alternating, five runs each, then the verifier
#                batch alone and beside the matcher (tools/time_verify_batch.py at 32 frames), five turns. CAPPED_LIB was step 0's
#                diagnostics build of the parent: eval_kernel<false, ...> alone under __attribute__((amdgpu_num_vgpr(56))) (the compiler
#                doubles the figure on gfx950's unified file: 112 registers, 52 and 148 bytes of scratch), everything else the parent's
#   batch        tools/time_verify_batch.py at 32 frames, parent and child, five alternating turns
#   bench        python bench.py, five runs each, alternating; then --dump-outputs of both, compared array for array
#   full         python bench.py --full --extras chained --no-cpu-baseline, two runs each
# PARENT_LIB: a build of the parent commit's library (TODHIP_LIB_PATH); without it only this library runs. Output: $OUT/vregs_*
# (OUT, default bench_out). Every GPU step runs under a time limit of its own and the first one that fails ends the script.
# The script writes only text and csv files; profiles/verify_regs.json was put together from them by hand.
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT:-$PWD/bench_out}; mkdir -p "$OUT"
export TMPDIR=/tmp
libs="child"; [ -n "$PARENT_LIB" ] && libs="parent child"
with_lib() {
  case $1 in
    parent) if [ -n "$PARENT_LIB" ]; then TODHIP_LIB_PATH="$PARENT_LIB" "${@:2}"; else env -u TODHIP_LIB_PATH "${@:2}"; fi ;;
    capped) TODHIP_LIB_PATH="$CAPPED_LIB" "${@:2}" ;;
    *) env -u TODHIP_LIB_PATH "${@:2}" ;;
  esac
}
stop() { echo "stopped: $1 ended with status $2"; exit 1; }
SHORT='import json, sys
d = json.loads(sys.stdin.read()); c = d.get("chained") or {}
print(json.dumps({"value": d["value"], "ms_per_step": d["ms_per_step"], "launch_ms": d["roofline"]["launch_ms"], "stage_ms_per_step": d["config"].get("stage_ms_per_step"),
                  "chained": {k: c[k] for k in ("frames_per_s", "matcher_launch_ms", "ms_per_step", "stage_ms_per_step") if k in c}}))'
bench_turns() {   # bench_turns <file> <lib> <lib>: the headline five times each, alternating
  for round in 1 2 3 4 5; do for which in "${@:2}"; do
    echo -n "bench $which: "; with_lib $which timeout -k 10 300 python bench.py 2>&1 | grep '^{' | tail -1 | python3 -c "$SHORT"; s=${PIPESTATUS[0]}; [ "$s" = 0 ] || stop "bench $which" "$s"
  done; done | tee -a "$1"; [ "${PIPESTATUS[0]}" = 0 ] || exit 1
}
batch_turns() {   # batch_turns <file> <lib> <lib>: the verifier batch alone and beside the matcher, five alternating turns
  for round in 1 2 3 4 5; do for which in "${@:2}"; do
    with_lib $which env B=32 timeout -k 10 200 python tools/time_verify_batch.py 2>&1 | tail -2 | sed "s/^/batch $which: /"; s=${PIPESTATUS[0]}; [ "$s" = 0 ] || stop "batch $which" "$s"
  done; done | tee "$1"; [ "${PIPESTATUS[0]}" = 0 ] || exit 1
}
for part in "$@"; do
  case $part in
  asm)
    for f in verify match; do
      /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -S --cuda-device-only -o "$OUT/vregs_$f.s" tod_amd/csrc/$f.hip || exit 1
    done ;;
  attribution)
    for round in 1 2 3; do for stages in match orb,match match,verify orb,match,verify; do
      echo -n "stages $stages: "; with_lib parent timeout -k 10 300 python bench.py --stages $stages 2>&1 | grep '^{' | tail -1 | python3 -c "$SHORT"; s=${PIPESTATUS[0]}; [ "$s" = 0 ] || stop "attribution $stages" "$s"
    done; done | tee "$OUT/vregs_attribution.txt"; [ "${PIPESTATUS[0]}" = 0 ] || exit 1 ;;
  trace)
    for which in ${TRACE_LIBS:-$libs}; do
      echo "== $which"
      rm -rf "$OUT/vregs_${which}_trace"
      with_lib $which timeout -k 10 400 rocprofv3 --kernel-trace --output-format csv -d "$OUT/vregs_${which}_trace" -- python3 bench.py > "$OUT/vregs_${which}_trace.log" 2>&1 || stop "trace $which" $?
      grep '^{' "$OUT/vregs_${which}_trace.log" | tail -1 | python3 -c "$SHORT"
      f=$(find "$OUT/vregs_${which}_trace" -name "*kernel_trace.csv" | head -1)
      gzip -c "$f" > "$OUT/vregs_${which}_kernel_trace.csv.gz"; rm -rf "$OUT/vregs_${which}_trace"
      python3 tools/verify_regs_trace.py "$OUT/vregs_${which}_kernel_trace.csv.gz" $(ls "$OUT"/vregs_verify.s "$OUT"/vregs_match.s 2>/dev/null) || stop "trace summary $which" $?
    done 2>&1 | tee "$OUT/vregs_trace.txt"; [ "${PIPESTATUS[0]}" = 0 ] || exit 1 ;;
  ceiling)
    [ -f "$CAPPED_LIB" ] || { echo "CAPPED_LIB names no library"; exit 1; }
    bench_turns "$OUT/vregs_ceiling_bench.txt" parent capped
    batch_turns "$OUT/vregs_ceiling_batch.txt" parent capped ;;
  batch) batch_turns "$OUT/vregs_batch.txt" $libs ;;
  bench)
    bench_turns "$OUT/vregs_bench.txt" $libs
    for which in $libs; do
      with_lib $which timeout -k 10 300 python bench.py --steps 20 --warmup 3 --dump-outputs "$OUT/vregs_dump_$which" > "$OUT/vregs_dump_$which.log" 2>&1 || stop "dump $which" $?
    done
    [ -n "$PARENT_LIB" ] && python3 - "$OUT" <<'PY' | tee "$OUT/vregs_dump.txt"
import glob, os, sys
import numpy as np
out = sys.argv[1]
names = sorted(os.path.basename(f) for f in glob.glob(os.path.join(out, "vregs_dump_parent", "*.npy")))
diff = [n for n in names if not np.array_equal(np.load(os.path.join(out, "vregs_dump_parent", n)), np.load(os.path.join(out, "vregs_dump_child", n)))]
print("%d arrays, different: %s" % (len(names), diff))
PY
    ;;
  full)
    for round in 1 2; do for which in $libs; do
      echo -n "full $which: "; with_lib $which timeout -k 10 500 python bench.py --full --extras chained --no-cpu-baseline 2>&1 | grep '^{' | tail -1 | tee "$OUT/vregs_full_${which}_$round.json" | python3 -c "$SHORT"; s=${PIPESTATUS[0]}; [ "$s" = 0 ] || stop "full $which" "$s"
    done; done | tee -a "$OUT/vregs_full.txt"; [ "${PIPESTATUS[0]}" = 0 ] || exit 1 ;;
  *) echo "unknown part $part"; exit 1 ;;
  esac
done
