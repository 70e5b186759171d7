export TMPDIR=/tmp; OUT=${OUT:-bench_out}; mkdir -p $OUT
timeout 900 python bench.py --full --no-cpu-baseline 2>&1 | grep -v amdgpu.ids > $OUT/bench_q.log; tail -1 $OUT/bench_q.log | cut -c1-1800
