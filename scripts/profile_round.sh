#!/bin/bash
# Regenerates the judged profile artefacts on the GPU box: usage scripts/profile_round.sh TAG [OUT]   (writes OUT/<files>_TAG, OUT
# defaults to prof_out; copy them into profiles/ afterwards).  AY_GIT_HEAD=<short sha> is recorded in the traffic json files next to the kernel-source hash.
set -e
export TMPDIR=/tmp
TAG=$1
OUT=${2:-prof_out}
R=${ROUND:-r03}
INF="--no_cpu_baseline --no_other_dtype --no_train_leg --no_fp32_leg --no_pipelined_leg --dtype ${AY_PROFILE_DTYPE:-bf16}"
mkdir -p $OUT
rm -rf $OUT/prof_kt $OUT/prof_fetch $OUT/prof_write
# ---- inference (the timed dtype of bench.py's default line: bf16; AY_PROFILE_DTYPE=fp16 profiles the other one)
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_kt -- python3 bench.py --steps 5 --warmup 2 $INF > $OUT/bench_kt_$TAG.log 2>&1
cp $OUT/prof_kt/*/*_kernel_stats.csv $OUT/${R}_bench_b64_kernel_stats_$TAG.csv
python scripts/layer_times.py $OUT/prof_kt > $OUT/${R}_bench_b64_layer_times_$TAG.txt
echo "inference kernel trace done"
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/prof_fetch -- python3 bench.py --steps 1 --warmup 1 $INF > /dev/null 2>&1
rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/prof_write -- python3 bench.py --steps 1 --warmup 1 $INF > /dev/null 2>&1
python scripts/hbm_traffic.py $OUT/prof_fetch $OUT/prof_write --json $OUT/traffic_$TAG.json > $OUT/${R}_hbm_traffic_$TAG.txt
tail -3 $OUT/${R}_hbm_traffic_$TAG.txt
rm -rf $OUT/prof_kt $OUT/prof_fetch $OUT/prof_write
# ---- the fp32 parity path (B=8): a leg of the --full line
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_kt -- python3 bench.py --full --steps 2 --warmup 1 --no_cpu_baseline --no_other_dtype --no_train_leg --no_pipelined_leg > $OUT/bench_kt_fp32_$TAG.log 2>&1
cp $OUT/prof_kt/*/*_kernel_stats.csv $OUT/${R}_bench_fp32leg_kernel_stats_$TAG.csv
rm -rf $OUT/prof_kt
echo "fp32 leg kernel trace done"
# ---- training (configs[2]: B=32, 1024^2)
TRN="--mode train --train_size 1024 --no_cpu_baseline"
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_kt -- python3 bench.py $TRN --steps 5 --warmup 2 > $OUT/bench_kt_train_$TAG.log 2>&1
cp $OUT/prof_kt/*/*_kernel_stats.csv $OUT/${R}_train_b32_s1024_kernel_stats_$TAG.csv
rm -rf $OUT/prof_kt
echo "training kernel trace done"
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/prof_fetch -- python3 bench.py $TRN --steps 1 --warmup 1 > /dev/null 2>&1
rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/prof_write -- python3 bench.py $TRN --steps 1 --warmup 1 > /dev/null 2>&1
python scripts/hbm_traffic_train.py $OUT/prof_fetch $OUT/prof_write --json $OUT/traffic_train_$TAG.json > $OUT/${R}_hbm_traffic_train_$TAG.txt
tail -3 $OUT/${R}_hbm_traffic_train_$TAG.txt
rm -rf $OUT/prof_fetch $OUT/prof_write
