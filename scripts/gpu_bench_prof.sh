# bench (+ per-launch table) and rocprof kernel stats only (no pytest).  usage: gpu_bench_prof.sh TAG
OUT=${EDET_OUT:-out}; mkdir -p $OUT
T=${1:-bp}
export TMPDIR=/tmp
(timeout 600 python bench.py --full --steps 5 --warmup 2 --no_cpu_baseline --no_other_configs --dump_launches $OUT/${T}_launches.txt 2>&1 | tail -3) > $OUT/${T}_bench_b128.log
(timeout 600 rocprofv3 --kernel-trace --stats -d $OUT/prof_${T} -o ${T} --output-format csv -- python bench.py --full --steps 3 --warmup 1 --no_cpu_baseline --no_other_configs 2>&1 | tail -3) > $OUT/${T}_prof.log
rm -f $OUT/prof_${T}/*kernel_trace.csv
cut -c1-700 $OUT/${T}_bench_b128.log
