#!/bin/bash
# The three phases of scripts/bench_v2_train.py, each in a process of its own under a time limit, chained: a phase that
# fails or runs out of time ends the run.  Output: one JSON line per phase, also appended to ${EDET_OUT:-out}/bench_v2_train.jsonl
set -euo pipefail
cd "$(dirname "$0")/.."
OUT="${EDET_OUT:-out}"
mkdir -p "$OUT"
timeout -k 10 240 python scripts/bench_v2_train.py opt "$@" | tee -a "$OUT/bench_v2_train.jsonl" &&
timeout -k 10 300 python scripts/bench_v2_train.py step "$@" | tee -a "$OUT/bench_v2_train.jsonl" &&
timeout -k 10 300 python scripts/bench_v2_train.py fwdbwd "$@" | tee -a "$OUT/bench_v2_train.jsonl"
