#!/bin/bash
# round 6: the sort passes' counts published before the ranking (MGS_OS_EARLY=1) against after it (0): correctness + stage times + trace
T=${TAG:-r6_k}; mkdir -p results; C=$PWD/vk_gaussian_splatting_amd/csrc; rm -f results/${T}_ab.log
( MGS_OS_EARLY=1 timeout 900 python -m pytest tests/test_gpu_parity.py -m gpu -x -q -k "sort or keys" 2>&1 | tail -3 ) | tee results/${T}_tests.log
for rep in 1 2 3; do for v in 0 1; do
  export MGS_OS_EARLY=$v
  python tools/stage_times.py --graph --tag garden_early$v 2>&1 | grep -v amdgpu >> results/${T}_ab.log
  if [ $rep != 3 ]; then
    python tools/stage_times.py --splats 1030000 --graph --tag train_early$v 2>&1 | grep -v amdgpu >> results/${T}_ab.log
    python tools/stage_times.py --strip 34 38 --graph --tag strip_early$v 2>&1 | grep -v amdgpu >> results/${T}_ab.log
    python tools/stage_times.py --instances 8 --frames 16 --graph --tag x8_early$v 2>&1 | grep -v amdgpu >> results/${T}_ab.log
  fi
done; done
for v in 0 1; do
  MGS_OS_EARLY=$v python bench.py --full --no-cpu-baseline --no-extras 2>/dev/null | grep '^{' | python -c "import sys,json; d=json.loads(sys.stdin.read()); print('bench_if3_early$v', round(d['value'],1), 'single', round(d['value_single_frame'],1), {k: round(v*1000,1) for k,v in d['stage_ms_single_stream'].items()}, d.get('parity',{}).get('psnr_db_min'), 'err', d['error_flags'])" >> results/${T}_ab.log
  MGS_OS_EARLY=$v MGS_LIB=$C/libmgs_trace.so MGS_GRAPH=0 MGS_OS_TRACE_FILE=/tmp/o.bin timeout 300 python tools/os_trace.py 0 2>&1 | grep -v amdgpu > results/${T}_os_trace_early$v.log
done
cat results/${T}_ab.log; grep -A8 "pass 1: \|pass 2: " results/${T}_os_trace_early0.log results/${T}_os_trace_early1.log | grep -v "^--$"
