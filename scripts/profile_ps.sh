#!/bin/bash
# The persistent round's profile at C3, three runs of their own:
#   the phase stamps (the timing build, issue-point stamps with the product's one parameter copy:
#     make -C shadow-1_amd timing TIMING_FLAGS="-DSHD_TIMING_LIGHT -DSHD_TIMING_P0 -DSHD_TIMING_NOWAIT"),
#   the SQ counters per wave and round over the bench's timed region (two counter sets, no tracing),
#   the kernel trace of the timed region against the bench's own time per round.
#     scripts/profile_ps.sh <out dir> [<product library>] [<timing library>]
# PS_TIMING_ARGS goes to scripts/ps_timing.py.
set -o pipefail
export TMPDIR=/tmp
O=$1
LIB=${2:-shadow-1_amd/libshdgpu.so}
TIM=${3:-shadow-1_amd/libshdgpu_tim.so}
B="bench.py --gpus 1 --steps 20 --warmup 5 --no-cpu-baseline --lossy-edge-loss-max 0"
rm -rf $O; mkdir -p $O
SHDGPU_LIB=$TIM timeout -k 10 200 python3 -u scripts/ps_timing.py $PS_TIMING_ARGS > $O/stamps_c3.txt 2>&1 || { tail -5 $O/stamps_c3.txt; exit 3; }
i=0
for set in "SQ_WAVES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS" \
           "SQ_WAVES SQ_INSTS_SMEM SQ_INSTS_BRANCH SQ_BUSY_CYCLES SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_WAIT_INST_LDS SQ_ACTIVE_INST_VALU"; do
  i=$((i+1))
  SHDGPU_LIB=$LIB timeout -s KILL 200 rocprofv3 --pmc $set --output-format csv -d $O/pmc$i -o run -- \
      python3 $B > $O/pmc$i.json 2> $O/pmc$i.err || { tail -5 $O/pmc$i.err; exit 4; }
done
mv $O/pmc1.json $O/bench_pmc.json
python3 scripts/pmc_round.py $O/bench_pmc.json $O/pmc1 $O/pmc2 > $O/sq_counters.txt || exit 5
rm -rf $O/pmc1 $O/pmc2 $O/pmc2.json $O/pmc*.err
SHDGPU_LIB=$LIB timeout -k 10 200 rocprofv3 --kernel-trace --marker-trace --output-format csv -d $O/tr -o run -- \
    python3 $B > $O/bench_rocprof.json 2> $O/tr.err || { tail -5 $O/tr.err; exit 6; }
python3 scripts/rocprof_timed.py $O/tr $O/bench_rocprof.json --out $O/timed_region.json > /dev/null || exit 7
rm -rf $O/tr $O/tr.err
cat $O/stamps_c3.txt $O/sq_counters.txt $O/timed_region.json
