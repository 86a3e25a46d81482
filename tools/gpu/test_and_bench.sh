# GPU box: the whole -m gpu suite (verbose, per-test timeout), then one bench line
# (logs under $OUT_DIR, default ./out).
set -o pipefail
cd $GRAFT_REPO_ROOT
O=${OUT_DIR:-out}; mkdir -p $O
timeout -k 10 900 python -u -m pytest tests -m gpu -v -p no:cacheprovider -rf --timeout 180 --timeout-method thread ${TESTS} > $O/pytest_gpu.log 2>&1
rc=$?
echo "pytest rc=$rc"
tail -30 $O/pytest_gpu.log
if [ $rc -eq 0 ] || [ $rc -eq 1 ]; then
  timeout -k 10 600 python bench.py --full --steps 10 --warmup 3 --no_cpu_baseline > $O/bench.log 2>&1
  brc=$?
  echo "bench rc=$brc"; tail -1 $O/bench.log
fi
exit $rc
