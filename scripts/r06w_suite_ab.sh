#!/bin/bash
# full -m gpu suite on the current tree, then a same-box A/B of the fused MBConv head in the headline step
cd "$GRAFT_REPO_ROOT"
OUT=${EDET_OUT:-out}; mkdir -p $OUT
T=${1:-r06w}
python -m pytest tests/ -x -q -m gpu > $OUT/${T}_pytest_gpu.log 2>&1
tail -5 $OUT/${T}_pytest_gpu.log
for f in 0 1; do
  EDET_MBCONV_FUSED=$f python bench.py --full --steps 20 --warmup 3 --no_cpu_baseline --no_other_configs --dump_launches $OUT/${T}_launches_f$f.txt > $OUT/${T}_bench_f$f.log 2>&1
  grep -o '"ms_per_step": [0-9.]*' $OUT/${T}_bench_f$f.log
done
grep -E "mbconv" $OUT/${T}_launches_f1.txt
