#!/bin/bash
# runs the default bench.py N times, each under its own timeout, and shows where a run that did not finish stopped
cd "$GRAFT_REPO_ROOT"
export OUT=${OUT:-bench_out}; mkdir -p "$OUT"
N=${1:-8}
for i in $(seq 1 $N); do
  timeout -k 5 ${2:-200} python bench.py --full ${3:-} > $OUT/soak_$i.json 2> $OUT/soak_$i.err
  rc=$?
  echo "run $i rc=$rc: $(grep 'bench.py \[' $OUT/soak_$i.err | tail -1)"
  if [ $rc -ne 0 ]; then echo "  --- stopped here; stderr tail:"; tail -5 $OUT/soak_$i.err; break; fi
done
