#!/bin/bash
# fast_nms_kernel's suppression over the survivor list, its DPP append and packed score (profiles/orb_nms.json): the parts of
# tools/orb_diet.sh under OUT/orb_nms, and step 0's attribution on the PARENT's library:
#   attribution  python bench.py with --stages match | orb,match | match,verify | the default, three alternating turns, on PARENT_LIB
#                (without it: this library): ORB's share of the DB pass's loss = median(orb,match) - median(match) of roofline.launch_ms
#   pmc | trace | batch | bench | full   as tools/orb_diet.sh has them, parent and child alternating
#   summary      tools/orb_nms_summary.py: everything found under OUT/orb_nms as one JSON document on stdout
# PARENT_LIB: a build of the parent commit's library (TODHIP_LIB_PATH). Every GPU step runs under its own time limit and the first
# failure ends the script.
cd "$(dirname "$0")/.." || exit 1
export OUT=${OUT:-$PWD/bench_out}/orb_nms; mkdir -p "$OUT"
export TMPDIR=/tmp
SHORT='import json, sys
d = json.loads(sys.stdin.read())
print(json.dumps({"value": d["value"], "ms_per_step": d["ms_per_step"], "launch_ms": d["roofline"]["launch_ms"], "stage_ms_per_step": d["config"].get("stage_ms_per_step")}))'
for part in "$@"; do
  case $part in
  attribution)
    for round in 1 2 3; do for stages in match orb,match match,verify orb,match,verify; do
      echo -n "stages $stages: "
      if [ -n "$PARENT_LIB" ]; then TODHIP_LIB_PATH="$PARENT_LIB" timeout -k 10 300 python bench.py --stages $stages 2>&1 | grep '^{' | tail -1 | python3 -c "$SHORT"
      else env -u TODHIP_LIB_PATH timeout -k 10 300 python bench.py --stages $stages 2>&1 | grep '^{' | tail -1 | python3 -c "$SHORT"; fi
      s=${PIPESTATUS[0]}; [ "$s" = 0 ] || { echo "stopped: attribution $stages ended with status $s"; exit 1; }
    done; done | tee "$OUT/diet_attribution.txt"; [ "${PIPESTATUS[0]}" = 0 ] || exit 1 ;;
  summary) python3 tools/orb_nms_summary.py "$OUT" ;;
  *) tools/orb_diet.sh "$part" || exit 1 ;;
  esac
done
