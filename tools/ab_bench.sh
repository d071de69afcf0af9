#!/bin/bash
# usage: ab_bench.sh tag libpath [opts]
# (writes $OUT/ab_TAG.json and .err; OUT defaults to bench_out/)
tag=$1; lib=$2; opts=$3; out=${OUT:-bench_out}; mkdir -p $out
MBPE_LIB=$lib MBPE_BENCH_OPTS=$opts python bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-full-run > $out/ab_$tag.json 2> $out/ab_$tag.err
python - <<PY
import json
d=json.loads(open('$out/ab_$tag.json').read().strip().splitlines()[-1])
r=d['roofline']
print('$tag', 'value %.0f'%d['value'], 'passes', d['timed_region']['stream_passes']/3, 'fused ms avg %.3f'%r['avg_launch_ms'], 'frac %.3f'%r['frac'], 'pc %.3f'%d['roofline_pair_count']['frac'])
PY
