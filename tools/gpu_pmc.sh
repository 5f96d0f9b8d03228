#!/bin/bash
# HBM traffic counters for the bench step, one counter group per pass (gfx950 TCC slot limits).
TAG=${1:-pmc}
R=$PWD
OUT=$R/gpurun_out/$TAG
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/fetch -o run -- python $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > $OUT/fetch.log 2>&1 || exit 1
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/write -o run -- python $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > $OUT/write.log 2>&1 || exit 1
echo PMC_OK
