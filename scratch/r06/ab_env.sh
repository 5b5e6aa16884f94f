#!/bin/bash
# same-box A/B of one environment switch on the default bench: bash scratch/r06/ab_env.sh VAR [pairs]   (VAR=0 against VAR=1)
V=$1; R=${2:-3}
echo "# columns: setting, images/s, ms per step, conv family TFLOP/s, conv family ms per step"
for r in $(seq $R); do for X in 0 1; do
env $V=$X python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-other-configs 2>/dev/null | tail -1 | python -c "
import json,sys
l=json.loads(sys.stdin.read()); r=l['roofline']
print('$V=$X', l['value'], l['ms_per_step'], r['achieved'], r['conv_ms_per_step'])"
done; done
