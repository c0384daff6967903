#!/bin/bash
# same box: round-2 bench (library + python of commit 08b158f) against the working tree, alternating
# needs scratch/old_r02/repo: a git worktree of 08b158f with its own build (git-ignored, not in a checkout)
cd $GRAFT_REPO_ROOT
[ -f scratch/old_r02/repo/bench.py ] || { echo "needs round 2's tree, built: git worktree add scratch/old_r02/repo 08b158f, then its own build()"; exit 1; }
for tag in old new old new; do
  if [ $tag = old ]; then f=scratch/old_r02/repo/bench.py; else f=bench.py; fi
  extra=""; [ $tag = new ] && extra="--full --no-stages"
  python $f --no-cpu-baseline $extra > gpurun_out/abb_$tag.log 2>/dev/null
  python - <<PY
import json
for l in open("gpurun_out/abb_$tag.log"):
    if l.startswith("{"):
        d=json.loads(l); lc=d.get("launch_classes") or {}
        print("$tag", round(d["ms_per_step"]*1e3,2), "us/step; kernel", round(d["kernels"]["gicp_align_kernel"]["ms"]*1e3,2), "; steady", (lc.get("steady") or {}).get("mean_us"), "; searching", (lc.get("searching") or {}).get("mean_us"), "; until_converged", (d.get("until_converged") or {}).get("ms_per_alignment"))
PY
done
