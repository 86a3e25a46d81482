set -o pipefail
cd $GRAFT_REPO_ROOT
O=${OUT_DIR:-out}; mkdir -p $O
timeout -k 10 600 python bench.py --full --task go2_parkour --num_envs 8192 --steps 5 --warmup 2 --no_cpu_baseline > $O/bench_parkour.log 2>&1
rc=$?
echo "parkour rc=$rc"; tail -3 $O/bench_parkour.log
exit $rc
