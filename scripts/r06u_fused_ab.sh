#!/bin/bash
# same-box A/B of the fused MBConv head in the headline step, plus the network tests that exercise it
cd "$GRAFT_REPO_ROOT"
OUT=${EDET_OUT:-out}; mkdir -p $OUT
python -m pytest tests/test_gpu_network.py -x -q -m gpu -k "bf16 or bit_reproducible or reference_graph" > $OUT/r06u_pytest.log 2>&1
tail -5 $OUT/r06u_pytest.log
for f in 0 1; do
  EDET_MBCONV_FUSED=$f python bench.py --full --steps 10 --warmup 3 --no_cpu_baseline --no_other_configs --dump_launches $OUT/r06u_launches_f$f.txt > $OUT/r06u_bench_f$f.log 2>&1
  grep -o '"ms_per_step": [0-9.]*' $OUT/r06u_bench_f$f.log
  grep -E "mbconv|320x320x16->96|160x160x24->144|320x320x96 k3s2|160x160x144 k" $OUT/r06u_launches_f$f.txt
done
