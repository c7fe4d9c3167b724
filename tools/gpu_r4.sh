# Round-4 evidence on one MI355X: the -m gpu suite, smoke, the calibrated FETCH/WRITE
# passes (tools/pmc_r3.sh), the bench line (with the CPU baseline), and rocprofv3
# --kernel-trace --stats of the bench's Gatys-Adam legs, its L-BFGS leg and its fast_st
# leg.  Outputs $OUT/<tag>_*; tools/save_round.py <tag> copies them to profiles/.
#   bash tools/gpu_r4.sh r4          ($OUT = $STX_OUT, default bench_out/)
set -o pipefail
export TMPDIR=/tmp
cd "$(dirname "$0")/.."; OUT=${STX_OUT:-bench_out}; mkdir -p $OUT
tag=${1:-r4}
if [ -z "${SKIP_TESTS:-}" ]; then
  echo "== tests"
  timeout -k 10 600 python -u -m pytest tests/ -m gpu -x -q -rf --timeout 120 --timeout-method thread > $OUT/${tag}_t.log 2>&1
  rc=$?; echo "TESTS rc=$rc"; tail -2 $OUT/${tag}_t.log; grep -E "^(FAILED|ERROR)|^E  " $OUT/${tag}_t.log | head -20
  [ $rc -eq 0 ] || exit $rc
  echo "== smoke"
  timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/${tag}_smoke.log 2>&1 || { tail -20 $OUT/${tag}_smoke.log; exit 1; }
  tail -1 $OUT/${tag}_smoke.log
fi
if [ -z "${SKIP_PMC:-}" ]; then
  echo "== pmc"
  timeout -k 10 600 bash tools/pmc_r3.sh ${tag} > $OUT/${tag}_pmc.log 2>&1 || { tail -10 $OUT/${tag}_pmc.log; exit 1; }
  cp profiles/${tag}_pmc.json $OUT/${tag}_pmc.json
fi
echo "== bench"
timeout -k 10 500 python bench.py --full ${BENCH_ARGS:-} > $OUT/${tag}_bench.json 2> $OUT/${tag}_bench.err || { tail -20 $OUT/${tag}_bench.err; exit 1; }
cat $OUT/${tag}_bench.json
echo "== rocprof gatys"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${tag}_prof -o run \
  -- python3 bench.py --full --steps 50 --warmup 5 --skip-cpu --skip-fast --skip-infer --lbfgs-steps 0 > $OUT/${tag}_prof.log 2>&1 || { tail -20 $OUT/${tag}_prof.log; exit 1; }
echo "== rocprof lbfgs"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${tag}_profl -o run \
  -- python3 bench.py --full --steps 1 --warmup 1 --gatys-run-iters 0 --skip-cpu --skip-fast --skip-infer > $OUT/${tag}_profl.log 2>&1 || { tail -20 $OUT/${tag}_profl.log; exit 1; }
echo "== rocprof fast_st"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${tag}_proff -o run \
  -- python3 bench.py --fast-only --steps 30 --warmup 2 > $OUT/${tag}_proff.log 2>&1 || { tail -20 $OUT/${tag}_proff.log; exit 1; }
echo "== done"
