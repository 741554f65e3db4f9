# Full GPU evidence pass of a round: parity tests, smoke, rocprof kernel stats, HBM PMC passes -> traffic json, then the
# bench line (which reads that traffic json), labelling / post-processing benches.
# usage (via gpurun): [SKIP_PMC=1] bash scripts/gpu_full.sh TAG
OUT=${EDET_OUT:-out}; mkdir -p $OUT
T=${1:-full}
STEPS_IN_PMC_RUN=6       # bench.py --full --steps 1 --warmup 1 in graph mode: 3 warm-up incl. capture, 1 profiled eager, 1 replay, 1 eager roofline step
export TMPDIR=/tmp
(timeout 1200 python -m pytest tests -m gpu -q --durations=5 2>&1 | cut -c1-3000 | tail -120) > $OUT/${T}_pytest_gpu.log
(timeout 300 python __graft_entry__.py smoke 2>&1 | tail -4) > $OUT/${T}_smoke.log
(timeout 600 rocprofv3 --kernel-trace --stats -d $OUT/prof_${T} -o ${T} --output-format csv -- python bench.py --full --steps 3 --warmup 1 --no_cpu_baseline --no_other_configs 2>&1 | tail -3) > $OUT/${T}_prof.log
find $OUT/prof_${T} -name "*kernel_trace.csv" -delete
run() {
  timeout 600 rocprofv3 --kernel-trace --pmc $2 -d $OUT/${T}_$1 -o $1 --output-format csv -- python bench.py --full --steps 1 --warmup 1 --no_cpu_baseline --no_other_configs > $OUT/${T}_$1.log 2>&1
  python scripts/pmc_agg.py $OUT/${T}_$1 > $OUT/${T}_pmc_$1.txt 2>&1
  rm -rf $OUT/${T}_$1
}
if [ -z "$SKIP_PMC" ]; then
run fetch "FETCH_SIZE"
run write "WRITE_SIZE"
python scripts/pmc_traffic.py $OUT/${T}_pmc_fetch.txt $OUT/${T}_pmc_write.txt $STEPS_IN_PMC_RUN profiles/${T}_traffic.json && cp profiles/${T}_traffic.json $OUT/
fi
(timeout 900 python bench.py --full --steps 20 --warmup 5 --dump_launches $OUT/${T}_launches.txt 2>&1 | tail -3) > $OUT/${T}_bench_b128.log
(timeout 120 python scripts/bench_labeling.py 2>&1 | tail -1) > $OUT/${T}_labeling.json
(timeout 200 python scripts/bench_postprocess.py 2>&1 | tail -12) > $OUT/${T}_postprocess_bench_b128.jsonl
tail -6 $OUT/${T}_pytest_gpu.log | cut -c1-300; cat $OUT/${T}_smoke.log; cut -c1-1200 $OUT/${T}_bench_b128.log; head -5 $OUT/${T}_pmc_fetch.txt; cat $OUT/${T}_labeling.json
