#!/bin/bash
# same-box A/B of the Hiera start point: first (default: beside towers + prefill) vs prefill (enqueued when the decode loop starts)
R=${GRAFT_REPO_ROOT:-/root/repo}
cd $R
for i in 1 2; do
  for v in first prefill; do
    VG_HIERA_START=$v python bench.py --full --no-cpu-baseline --no-quality --no-roofline --steps 5 2>/dev/null | python -c "
import sys, json; r=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('VG_HIERA_START=$v  C2 %.2f ms  video %.2f ms  graph %s' % (r['ms_per_step'], r['video_branch']['ms_per_step'], r['video_branch'].get('propagation_graph')))"
  done
done
