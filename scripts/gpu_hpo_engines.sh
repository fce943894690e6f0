#!/bin/bash
# Inline-HPO engines per GPU (the `hpo` record of the `bench.py --full` line): 3 / 4 / 5 / 6.
# Logs and the summary go to $OUT (default build/hpo_engines).
set -o pipefail
cd $GRAFT_REPO_ROOT
OUT=${OUT:-build/hpo_engines}
mkdir -p $OUT
: > $OUT/hpo_engines.txt
for e in 3 4 5 6; do
  timeout -k 10 300 python bench.py --full --steps 50 --warmup 10 --hpo-engines-per-gpu $e > $OUT/hpoe.log 2>&1 || { tail -n 20 $OUT/hpoe.log; exit 1; }
  echo "engines $e $(tail -n 1 $OUT/hpoe.log | python -c 'import json,sys; h=json.loads(sys.stdin.read())["hpo"]; print(h["trials_per_hour"], h["wall_s"], h["mean_trial_s"], h["trials_done"])')" | tee -a $OUT/hpo_engines.txt
done
