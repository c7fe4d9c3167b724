# environment A/B on one box (separate processes, alternating): bench.py Gatys + fast_st legs
# with VAR=a vs VAR=b, after the given tests.   bash tools/gpu_envab.sh <tag> VAR a b "<tests>"
# (outputs under $STX_OUT, default bench_out/)
export STX_AB=1  # (the host path reads its A/B switches only under STX_AB=1: N.knob)
cd "$(dirname "$0")/.."; OUT=${STX_OUT:-bench_out}; mkdir -p $OUT
tag=$1; var=$2; va=$3; vb=$4; T=${5:-}
if [ -n "$T" ]; then
  timeout -k 10 400 python -u -m pytest $T -x -q -rf --timeout 120 --timeout-method thread > $OUT/${tag}_t.log 2>&1
  rc=$?; echo "T rc=$rc"; tail -1 $OUT/${tag}_t.log; grep -E "^(FAILED|ERROR)|^E  " $OUT/${tag}_t.log | head -10
  [ $rc -eq 0 ] || exit $rc
fi
for i in 1 2; do
  for v in $va $vb; do
    env $var=$v timeout -k 10 200 python bench.py --full --steps 50 --warmup 5 --skip-cpu --skip-infer --lbfgs-steps 0 --gatys-run-iters 0 --fast-b64-steps 0 > $OUT/${tag}_$v$i.json 2>$OUT/${tag}_$v$i.err || { tail -3 $OUT/${tag}_$v$i.err; exit 1; }
    python -c "import json;d=json.load(open('$OUT/${tag}_$v$i.json'));print('$var=$v #$i', 'gatys_ms', d['ms_per_step'], 'fast_ms', d['fast_st']['ms_per_step'])"
  done
done
