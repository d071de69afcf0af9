#!/bin/bash
# Round-3 profiles.  Run on the GPU box from the repo root:  bash profiles/collect_r03.sh
# (build/libmbpe_diag.so must exist: tools/mkvar.sh diag -DMBPE_DIAG)
# Writes the condensed summaries to gpurun_out/r03/ (copied into profiles/ afterwards).
# rocprofv3: counters in their own runs (never together with traces), program directly after "--".
R=${GRAFT_REPO_ROOT:-$(pwd)}
O=$R/gpurun_out/r03
rm -rf $O; mkdir -p $O
cd /tmp && export TMPDIR=/tmp
S=$R/profiles/summarize.py

# 1. the driver's command: kernel trace + stats
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $O/kt -o kt -- python3 $R/bench.py --full --gpus 1 --steps 20 --warmup 5 > $O/r03_bench_under_profiler.json 2> $O/kt.err || { tail -5 $O/kt.err; exit 1; }
python3 $S stats $(find $O/kt -name '*kernel_stats.csv' | head -1) > $O/r03_kernel_stats.csv
python3 $S trace $(find $O/kt -name '*kernel_trace.csv' | head -1) > $O/r03_kernel_trace.csv
python3 $S trace20 $(find $O/kt -name '*kernel_trace.csv' | head -1) > $O/r03_kernel_trace_timed_region.csv
rm -rf $O/kt
echo "step 1 done"

# 2. config 3 (bible stand-in)
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $O/kb -o kb -- python3 $R/bench.py --full --config bible --steps 20 --warmup 5 > $O/r03_bible_bench_under_profiler.json 2> $O/kb.err || { tail -5 $O/kb.err; exit 1; }
python3 $S trace $(find $O/kb -name '*kernel_trace.csv' | head -1) > $O/r03_bible_kernel_trace.csv
rm -rf $O/kb
echo "step 2 done"

# 3. HBM traffic, one counter per run (FETCH_SIZE takes 3 TCC slots, WRITE_SIZE 2)
for c in FETCH_SIZE WRITE_SIZE; do
  timeout -k 10 600 rocprofv3 --pmc $c --output-format csv -d $O/p_$c -o p -- python3 $R/bench.py --full --steps 20 --warmup 5 --no-full-run --no-cpu-baseline > $O/p_$c.log 2>&1 || { tail -5 $O/p_$c.log; exit 1; }
  python3 $S pmc $(find $O/p_$c -name '*counter_collection.csv' | head -1) > $O/r03_pmc_$c.csv
  rm -rf $O/p_$c
done
echo "step 3 done"

# 4. SQ counters (instruction mix and LDS bank conflicts of the pair-count scan and the fused pass)
i=0
: > $O/r03_pmc_sq.csv
for set in "SQ_BUSY_CYCLES SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU" "SQ_INSTS_LDS SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_ACTIVE_INST_VALU" "SQ_WAVE_CYCLES SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_WAIT_ANY"; do
  i=$((i+1))
  timeout -k 10 600 rocprofv3 --pmc $set --kernel-trace --output-format csv -d $O/s_$i -o p -- python3 $R/bench.py --full --steps 20 --warmup 5 --no-full-run --no-cpu-baseline > $O/s_$i.log 2>&1 || { tail -5 $O/s_$i.log; continue; }
  python3 $S sq $(find $O/s_$i -name '*counter_collection.csv' | head -1) >> $O/r03_pmc_sq.csv
  if [ $i = 1 ]; then cp $(find $O/s_1 -name '*counter_collection.csv' | head -1) $O/set1_counters.csv; cp $(find $O/s_1 -name '*kernel_trace.csv' | head -1) $O/set1_trace.csv; fi
  rm -rf $O/s_$i
done
python3 $R/profiles/make_traffic_json.py $O r03 > $O/r03_pmc_traffic.json
echo "step 4 done"

# 5. the two floors of a fused pass: copy-only build of the kernel (timing-only instantiations, -DMBPE_DIAG) and
#    the shipped kernel's vector instructions per tile; the duration of a full-size pass comes from step 1's trace
cd $R
MBPE_LIB=$R/build/libmbpe_diag.so timeout -k 10 300 python3 tools/fused_diag.py > $O/fused_diag.log 2>&1 || tail -5 $O/fused_diag.log
python3 profiles/make_floor_json.py --diag-log $O/fused_diag.log --counters $O/set1_counters.csv --trace $O/set1_trace.csv > $O/r03_fused_floor.json
rm -f $O/set1_counters.csv $O/set1_trace.csv
cat $O/r03_fused_floor.json
echo "step 5 done"

# 6. pair-count scan through the C-ABI (clock ramp; random and text) and the bytes a multi-GPU run would exchange
timeout -k 10 300 python3 tools/pc_time.py > $O/r03_pc_time.log 2>&1
timeout -k 10 300 python3 tools/exchange_bytes.py > $O/r03_exchange_bytes.json 2> $O/xb.err || tail -3 $O/xb.err
ls -la $O
