#!/bin/bash
# Quick iteration on the stride-2 3-D split kernel: its tests + the bench line's per-kernel timings.
R=${GRAFT_REPO_ROOT:-$(pwd)}
cd $R
OUT=${OUT:-/tmp/s2_iter}; mkdir -p $OUT
python -m pytest tests -m gpu -q -x --timeout 900 -s -k "stride2 or deconv3d or hourglass" 2>&1 | grep -v "MIOpen\|^MODE\|^using\|^add" | tail -${2:-14}
python bench.py --steps 5 --warmup 2 --full --no-cpu-baseline --no-eval-b1 2>/dev/null | grep "^{" > $OUT/${1:-s2}_bench.json
python - <<PY
import json
d=json.loads(open("$OUT/${1:-s2}_bench.json").read())
print(d["value"], d["ms_per_step"])
for k,v in d["kernels"].items():
    if " s2 " in k or "deconv" in k: print(k, v)
PY
