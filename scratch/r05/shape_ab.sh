#!/bin/bash
line() { python3 -c "import json,sys; d=json.loads(sys.stdin.read()); print('$1', d['value'], d['ms_per_step'], d['roofline']['achieved'], d['roofline'].get('conv_ms_per_step'))"; }
for i in 1 2; do
for m in 1 2 3 4 0; do
timeout 600 python bench.py --full --no-cpu-baseline --no-other-configs --wide-tiles $m 2>/dev/null | tail -1 | line "tiles$m"
done
done
