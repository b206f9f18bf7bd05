#!/bin/bash
# SQ counters of the tick launch (full ticks only): where do the wavefronts of a tick spend their cycles?
#   tools/debug/tick_sq_pmc.sh  -> gpurun_out/tick_sq_pmc.txt
# Also the L2-side counters: what does the launch ask of the L2?  Counters only -- no tracing beside them (the counter CSV names
# the kernels itself); one run per set, each under its own time limit, and nothing more is started once a run has failed.
# (an argument is a tag appended to the file's name: tick_sq_pmc_<tag>.txt; BEATRICE_HIP_LIB selects another build, as everywhere)
ROOT=${GRAFT_REPO_ROOT:-$(pwd)}
cd /tmp && export TMPDIR=/tmp
OUT=$ROOT/gpurun_out/tick_sq_pmc.txt
[ -n "$1" ] && OUT=${OUT%.txt}_$1.txt
mkdir -p "$(dirname $OUT)"
: > $OUT
for set in "SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_WAIT_INST_LDS SQ_VALU_MFMA_BUSY_CYCLES SQ_WAVES" \
           "SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_ACTIVE_INST_VMEM SQ_ACTIVE_INST_SCA SQ_INSTS_VALU SQ_INSTS_MFMA SQ_INSTS_LDS SQ_INSTS_VMEM" \
           "SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INSTS_SALU SQ_INST_CYCLES_VMEM SQ_IFETCH SQ_WAIT_IFETCH SQ_INSTS_SMEM SQ_INSTS_BRANCH" \
           "TCP_TCC_READ_REQ_sum TCC_REQ_sum TCC_HIT_sum"; do
  rm -rf /tmp/pmc
  timeout -k 10 240 rocprofv3 --pmc $set --output-format csv -d /tmp/pmc -o p -- python $ROOT/bench.py --full --steps 120 --warmup 10 --no-extras > /tmp/pmc_run.log 2>&1
  rc=$?
  if [ $rc -ne 0 ]; then echo "counter run failed (exit $rc): $set" | tee -a $OUT; tail -5 /tmp/pmc_run.log; exit $rc; fi
  python - "$(find /tmp/pmc -name '*counter_collection.csv' | head -1)" >> $OUT <<'PY'
import csv, sys, collections
d = collections.defaultdict(list)
for r in csv.DictReader(open(sys.argv[1])):
    if "table_kernel" in r["Kernel_Name"]:
        d[r["Counter_Name"]].append(float(r["Counter_Value"]))
for k, v in d.items():
    v = sorted(v); v = v[len(v) // 2:]          # full ticks
    print("%-28s %14.0f per full tick (%d launches)" % (k, sum(v) / len(v), len(v)))
PY
done
cat $OUT
