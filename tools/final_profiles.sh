#!/bin/bash
# everything behind profiles/${TAG}_*: run on an MI355X, results land in results/ (copy to profiles/ afterwards)
export TAG=${TAG:-r6_z}; R=$(cd "$(dirname "$0")/.." && pwd); cd $R; mkdir -p results
python bench.py --full 2>/dev/null | grep '^{' | tail -1 > results/${TAG}_bench_if3.json
python bench.py --full --inflight 1 2>/dev/null | grep '^{' | tail -1 > results/${TAG}_bench_if1.json
bash tools/collect_profiles.sh > results/${TAG}_collect.log 2>&1
cp results/pmc_sq_all.json results/${TAG}_pmc_sq_all_kernels.json
cd $R; bash tools/bench_matrix.sh > results/${TAG}_bench_matrix.log 2>&1
cd $R; bash tools/pmc_alpha_sum.sh > results/${TAG}_pmc_alpha_sum.log 2>&1
cd $R; for g in 2 4 8; do python tools/strip_throughput.py 1920 1080 $g 3 > results/${TAG}_strip_throughput_1920x1080_g${g}_k3.log 2>&1; done
python tools/strip_throughput.py 3840 2160 8 3 > results/${TAG}_strip_throughput_3840x2160_g8_k3.log 2>&1
TAG=$TAG bash tools/strip_kernels.sh 1920 1080 34 38 > results/${TAG}_strip_kernels.log 2>&1
ls -la results | tail -30
