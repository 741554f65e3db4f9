# Evidence pass on the FINAL tree when the GPU budget does not hold the full one (scripts/gpu_final.sh, ~15 min): the same
# rocprof statistics / PMC passes / bench lines, the kernel timeline of a replayed step, and the parity tests of the files
# that the changes since the last full pass touch (LITE_TESTS / LITE_K).  usage (via gpurun): bash scripts/gpu_final_lite.sh TAG
OUT=${EDET_OUT:-out}; mkdir -p $OUT
T=${1:-final}
STEPS_IN_PMC_RUN=6
export TMPDIR=/tmp
(timeout 300 python __graft_entry__.py smoke 2>&1 | tail -4) > $OUT/${T}_smoke.log
(timeout 600 rocprofv3 --kernel-trace --stats -d $OUT/prof_${T} -o ${T} --output-format csv -- python bench.py --full --steps 3 --warmup 1 --no_cpu_baseline --no_other_configs 2>&1 | tail -3) > $OUT/${T}_prof.log
find $OUT/prof_${T} -name "*kernel_trace.csv" -delete
cp $OUT/prof_${T}/${T}_kernel_stats.csv profiles/${T}_kernel_stats_b128.csv && echo ${T}_kernel_stats_b128.csv > profiles/CURRENT
(timeout 900 python -m pytest ${LITE_TESTS:-tests/test_gpu_bench_shapes.py tests/test_gpu_network.py} -m gpu -q --durations=5 2>&1 | cut -c1-3000 | tail -40) > $OUT/${T}_pytest_gpu.log
(timeout 600 python -m pytest tests/test_gpu_kernels.py -m gpu -q -k "${LITE_K:-fuse or batchnorm or test_dw_ or squeeze}" 2>&1 | cut -c1-3000 | tail -12) >> $OUT/${T}_pytest_gpu.log
run() {
  timeout 600 rocprofv3 --kernel-trace --pmc $2 -d $OUT/${T}_$1 -o $1 --output-format csv -- python bench.py --full --steps 1 --warmup 1 --no_cpu_baseline --no_other_configs > $OUT/${T}_$1.log 2>&1
  python scripts/pmc_agg.py $OUT/${T}_$1 > $OUT/${T}_pmc_$1.txt 2>&1
  rm -rf $OUT/${T}_$1
}
run fetch "FETCH_SIZE"
run write "WRITE_SIZE"
python scripts/pmc_traffic.py $OUT/${T}_pmc_fetch.txt $OUT/${T}_pmc_write.txt $STEPS_IN_PMC_RUN profiles/${T}_traffic.json && cp profiles/${T}_traffic.json $OUT/
(timeout 900 python bench.py --full --steps 20 --warmup 5 --dump_launches $OUT/${T}_launches.txt 2>&1 | tail -3) > $OUT/${T}_bench_b128.log
bash scripts/gpu_trace.sh ${T} > $OUT/${T}_trace.log 2>&1
python scripts/timeline_gaps.py $OUT/${T}_trace.csv.gz 6 > $OUT/${T}_timeline.txt 2>&1
(timeout 600 rocprofv3 --kernel-trace --stats -d $OUT/prof_${T}_v2s -o v2s --output-format csv -- python scripts/bench_v2s.py --steps 10 --dump_launches $OUT/${T}_launches_v2s_224_b256.txt 2>&1 | grep "^{" | tail -1) > $OUT/${T}_bench_v2s.json
(timeout 900 rocprofv3 --kernel-trace --stats -d $OUT/prof_${T}_d7x -o d7x --output-format csv -- python bench.py --full --model efficientdet-d7x --image_size 1536 --batch 8 --steps 3 --warmup 1 --no_cpu_baseline --no_other_configs --dump_launches $OUT/${T}_launches_d7x_1536_b8.txt 2>&1 | grep "^{" | tail -1) > $OUT/${T}_bench_d7x.json
find $OUT/prof_${T}_v2s $OUT/prof_${T}_d7x -name "*kernel_trace.csv" -delete
tail -14 $OUT/${T}_pytest_gpu.log | cut -c1-300; cat $OUT/${T}_smoke.log; cut -c1-1200 $OUT/${T}_bench_b128.log; cat $OUT/${T}_timeline.txt | head -8; cut -c1-250 $OUT/${T}_bench_v2s.json; cut -c1-250 $OUT/${T}_bench_d7x.json
