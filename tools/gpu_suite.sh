#!/bin/bash
# the whole GPU suite, then the bench line with every leg beside the step (--full) (no core files: a crashing torch process writes tens of GB)
set -u
TAG=${TAG:-r06}   # the round the outputs are named after (profiles/$TAG/ once copied there)
OUT=${OUT:-results}   # where the test log and the bench line are written
ulimit -c 0
mkdir -p "$OUT"
timeout -k 10 1100 python -m pytest tests -x -q -m gpu "$@" > "$OUT/${TAG}_gpu_tests.log" 2>&1; echo "suite rc=$?"; tail -5 "$OUT/${TAG}_gpu_tests.log"
timeout -k 10 600 python bench.py --full > "$OUT/${TAG}_bench.json" 2> "$OUT/${TAG}_bench.err"; echo "bench rc=$?"; tail -c 3000 "$OUT/${TAG}_bench.json"
