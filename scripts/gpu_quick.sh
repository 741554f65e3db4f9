# quick GPU check: selected parity tests + bench with per-launch table.  usage: gpu_quick.sh TAG "pytest -k expr"
OUT=${EDET_OUT:-out}; mkdir -p $OUT
T=${1:-q}
K=${2:-pw_fwd}
(timeout 900 python -m pytest tests -m gpu -x -q -k "$K" 2>&1 | tail -15) > $OUT/${T}_pytest.log
(timeout 600 python bench.py --full --steps 5 --warmup 2 --no_cpu_baseline --no_other_configs --dump_launches $OUT/${T}_launches.txt 2>&1 | tail -3) > $OUT/${T}_bench.log
tail -6 $OUT/${T}_pytest.log; cut -c1-330 $OUT/${T}_bench.log
