# final collection of round 5 (GPU box): gpu suite, profiles of three workloads, the bench lines, the scaling emulation.  usage: _run_final.sh OUTDIR
OUT=${1:?usage: _run_final.sh OUTDIR}
mkdir -p $OUT
(timeout 2300 python -m pytest tests -m gpu -q 2>&1 | tail -8) > $OUT/gpu_suite.log
tools/collect_profiles.sh r05 phage-100k > $OUT/prof_100k.log 2>&1
tools/collect_profiles.sh r05 phage-1k > $OUT/prof_1k.log 2>&1
tools/collect_profiles.sh r05 imgvr-10k > $OUT/prof_imgvr.log 2>&1
timeout 1200 python bench.py --full > $OUT/bench_default.json 2> $OUT/bench_default.err
timeout 600 python bench.py --workload phage-1k --full --no-cli-wall --steps 20 --warmup 3 > $OUT/bench_1k.json 2>/dev/null
timeout 600 python bench.py --workload imgvr-10k --full --no-cli-wall --no-cpu-baseline --steps 10 --warmup 2 > $OUT/bench_imgvr.json 2>/dev/null
(SCAN=sliced timeout 600 python tools/strong_scaling_sim.py 2>&1 | tail -6) > $OUT/sim_sliced.log
(SCAN=sliced RANK_SIM=5 timeout 600 python tools/strong_scaling_sim.py 2>&1 | tail -6) > $OUT/sim_sliced_rank5.log
cat $OUT/gpu_suite.log; tail -2 $OUT/bench_default.err
