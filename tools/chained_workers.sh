cd "$GRAFT_REPO_ROOT"
export OUT=${OUT:-bench_out}; mkdir -p "$OUT"
for w in ${1:-4 6 8}; do
  timeout -k 10 300 python bench.py --full --extras chained --stages match --no-cpu-baseline --verify-workers $w --steps ${2:-60} --repeats 3 > $OUT/vw$w.json 2> $OUT/vw$w.err
  python3 -c "
import json
d=json.load(open('$OUT/vw$w.json'))
c=d['chained']
print('workers $w: chained', c['frames_per_s']['values'], c['stage_ms_per_step'], c['frames_with_the_rendering_pose'])
"
done
