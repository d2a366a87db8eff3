#!/bin/bash
# same-box A/B of the r05 GEMM route: the shape rule with the 256x192 tile (default) against the rule without it (VG_GEMM_P8=4), twice each, interleaved
R=${GRAFT_REPO_ROOT:-/root/repo}
cd $R
for i in 1 2; do
  for v in 1 4; do
    VG_GEMM_P8=$v python bench.py --full --no-cpu-baseline --no-quality --steps 5 2>/dev/null | python -c "
import sys, json
r = json.loads(sys.stdin.read().strip().splitlines()[-1])
st = r['stages']
print('VG_GEMM_P8=$v  C2 %.2f ms  video %.2f ms  stages hiera %.2f towers %.2f prefill %.2f decode %.2f' % (r['ms_per_step'], r['video_branch']['ms_per_step'], st['hiera_fpn']['ms'], st['towers']['ms'], st['prefill']['ms'], st['decode']['ms']))"
  done
done
