#!/bin/bash
# full -m gpu suite + the default bench line
cd "$GRAFT_REPO_ROOT"
OUT=${EDET_OUT:-out}; mkdir -p $OUT
T=${1:-r06x}
python -m pytest tests/ -x -q -m gpu > $OUT/${T}_pytest_gpu.log 2>&1
tail -4 $OUT/${T}_pytest_gpu.log
( time python bench.py --full ) > $OUT/${T}_bench_default.log 2>&1
tail -c 3000 $OUT/${T}_bench_default.log
