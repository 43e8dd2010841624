#!/bin/bash
# tools/profile_round.sh <tag> — the round's measurement batch (GPU box, from the repo root): rocprofv3 stats + FETCH/WRITE
# passes of the roofline workloads, one bench line per workload, the full bench line, the GPU test log with durations; all under
# $WAA_OUT_DIR (default out/).
set -u
TAG=$1
OUT=${WAA_OUT_DIR:-out}; export WAA_OUT_DIR=$OUT
mkdir -p $OUT
for w in c2 t1 c3 c4 c5 c1a os2 hrtf echo; do
  bash tools/pmc_pass.sh $w ${TAG}_$w > /dev/null 2>&1
done
for w in c2k c4 echo fb fbq fm osc iir2 iir8 os2 os4 hrtf; do
  python bench.py --workload $w --steps 5 --warmup 2 --sustain 0 --no-cpu-baseline --no-extra > $OUT/${TAG}_bench_$w.json 2>/dev/null
done
python bench.py --full --detail $OUT/${TAG}_bench_detail.json > $OUT/${TAG}_bench_default.json 2> $OUT/${TAG}_bench_default.err
python -m pytest tests -m gpu -q --durations=15 > $OUT/${TAG}_gputests_durations.log 2>&1
tail -3 $OUT/${TAG}_gputests_durations.log
ls $OUT | grep $TAG | wc -l
