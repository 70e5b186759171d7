#!/bin/bash
# Runs on a GPU machine: the whole parity suite, smoke, the default bench line (live PMC traffic + CPU baseline),
# an fp32 bench line, and a rocprofv3 kernel trace of the default command.  Everything is logged under $OUT (default bench_out/).
export TMPDIR=/tmp
OUT=${OUT:-bench_out}; mkdir -p $OUT/prof
cd "$GRAFT_REPO_ROOT" 2>/dev/null || true
REPO="$PWD"
rocm-smi --showproductname 2>/dev/null | head -5 > $OUT/device.txt
timeout 1500 python -m pytest tests -m gpu -q --tb=short -p no:cacheprovider > $OUT/pytest_gpu.log 2>&1
echo "pytest exit: $?" >> $OUT/pytest_gpu.log
tail -6 $OUT/pytest_gpu.log
timeout 300 python __graft_entry__.py smoke 2>&1 | grep -v amdgpu.ids > $OUT/smoke.log; echo "smoke exit $?" >> $OUT/smoke.log; tail -3 $OUT/smoke.log
timeout 900 python bench.py --full 2>&1 | grep -v amdgpu.ids > $OUT/bench_bf16.log; tail -1 $OUT/bench_bf16.log | cut -c1-1500
timeout 600 python bench.py --full --precision fp32 --no-cpu-baseline --no-pmc --steps 40 2>&1 | grep -v amdgpu.ids > $OUT/bench_fp32.log; tail -1 $OUT/bench_fp32.log | cut -c1-600
timeout 600 python bench.py --full --hidden 128 --no-cpu-baseline --no-pmc --steps 60 2>&1 | grep -v amdgpu.ids > $OUT/bench_h128.log; tail -1 $OUT/bench_h128.log | cut -c1-600
(cd /tmp && rm -rf /tmp/prof && timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof -o bench -- python "$REPO/bench.py" --full --steps 60 --pretrain 300 --eval-rays 0 --no-cpu-baseline --no-pmc > "$REPO/$OUT/prof.log" 2>&1)
find /tmp/prof -name "*kernel_stats.csv" -exec cp {} $OUT/prof/r02_bench_default_kernel_stats.csv \;
python scripts/trace_gaps.py /tmp/prof > $OUT/prof/r02_step_timeline.txt 2>&1; cat $OUT/prof/r02_step_timeline.txt | head -24
python scripts/trace_gaps.py /tmp/prof hashgrid_fwd 100 > $OUT/prof/r02_step_timeline_2p21.txt 2>&1; cat $OUT/prof/r02_step_timeline_2p21.txt | head -30
head -16 $OUT/prof/r02_bench_default_kernel_stats.csv | cut -c1-200
