#!/bin/bash
# One visit: whole suite + smoke, then parent/candidate alternations
# (traced, then plain), then the candidate's PMC passes.  Every GPU step has
# its own time limit; the script stops at the first step that fails.
set -uo pipefail
OUT=${1:-out/uniform_hint}  # where the records go
mkdir -p "$OUT"
PARENT=$PWD/tools/ablib/parent/libmirsha.so
step() {  # step <name> <seconds> <cmd...>
  local name=$1 secs=$2; shift 2
  local t0=$SECONDS
  timeout -k 10 "$secs" "$@"
  local rc=$?
  echo "[$name] rc=$rc $((SECONDS - t0))s"
  if [ $rc -ne 0 ]; then echo "stopping at $name"; exit $rc; fi
}
step suite 400 bash -c "python -m pytest -q -m gpu tests > $OUT/suite.log 2>&1; rc=\$?; tail -4 $OUT/suite.log; exit \$rc"
step smoke 120 bash -c "python -c 'import __graft_entry__ as g; g.smoke()' > $OUT/smoke.log 2>&1; rc=\$?; tail -2 $OUT/smoke.log; exit \$rc"
FAST="--gpus 1 --steps 20 --warmup 5 --cpu-seconds 0 --no-pcie --no-config3-leg --no-overlap-extra"
for i in 1 2 3; do
  step trace_parent_$i 150 bash -c "MIRSHA_AB_LIB=$PARENT rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace_parent_$i -o run -- python3 bench.py $FAST > $OUT/traced_parent_$i.json 2> $OUT/traced_parent_$i.err"
  step trace_cand_$i 150 bash -c "rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace_cand_$i -o run -- python3 bench.py $FAST > $OUT/traced_cand_$i.json 2> $OUT/traced_cand_$i.err"
done
# the candidate's instruction count: one PMC pass of its own
step pmc_sq 150 bash -c "rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_ACTIVE_INST_VALU --kernel-include-regex sha256 --output-format csv -d $OUT/prof/pmc_sq -o run -- python3 bench.py $FAST > $OUT/pmc_sq.out 2>&1"
for i in 1 2 3; do
  step plain_parent_$i 200 bash -c "MIRSHA_AB_LIB=$PARENT python3 bench.py --gpus 1 --steps 20 --warmup 5 > $OUT/plain_parent_$i.json 2> $OUT/plain_parent_$i.err"
  step plain_cand_$i 200 bash -c "python3 bench.py --gpus 1 --steps 20 --warmup 5 > $OUT/plain_cand_$i.json 2> $OUT/plain_cand_$i.err"
done
# traffic of the new source key (profiles/summarize.py layout)
step pmc_write 150 bash -c "rocprofv3 --pmc WRITE_SIZE --kernel-include-regex sha256 --output-format csv -d $OUT/prof/pmc_write -o run -- python3 bench.py $FAST > $OUT/pmc_write.out 2>&1"
step pmc_size 150 bash -c "rocprofv3 --pmc TCC_EA0_RDREQ_32B_sum TCC_EA0_RDREQ_64B_sum TCC_EA0_RDREQ_128B_sum --kernel-include-regex sha256 --output-format csv -d $OUT/prof/pmc_size -o run -- python3 bench.py $FAST > $OUT/pmc_size.out 2>&1"
step pmc_fetch 150 bash -c "rocprofv3 --pmc FETCH_SIZE --kernel-include-regex sha256 --output-format csv -d $OUT/prof/pmc_fetch -o run -- python3 bench.py $FAST > $OUT/pmc_fetch.out 2>&1"
echo done
