#!/bin/bash
# Runs on the GPU box: counters-only rocprofv3 passes (--pmc alone, no tracing of any kind) of the bench command, for the
# wait / LDS counters of the group kernels.  usage: tools/profile_pmc_passes.sh TAG "GEN_OPTS" BATCH...
# Output under $PROFILE_OUT/pmc_<TAG>/b<BATCH>_p<n>/ (PROFILE_OUT: default out) (one directory per pass); profiles/r05_group16_b4096_pmc.csv holds the
# per-dispatch means of csim_tran_group_kernel.  Counters this GPU does not offer (rocprofv3 --list-avail) are left out.
# Each pass runs under its own time limit; after an abort, a fault or a time limit nothing more is started; a pass that
# merely fails is reported, the others still run, and the script ends with status 1.
# (tools/profile_bench.sh pairs its --pmc passes with --kernel-trace for tools/summarize_profile.py; here nothing is traced.)
set -u
FAILED=0
TAG=$1; GOPTS=$2; shift 2
OUT=${PROFILE_OUT:-out}/pmc_$TAG
mkdir -p "$OUT"
export TMPDIR=/tmp
step() {  # name, command...
  local name=$1; shift
  "$@" > "$OUT/$name.out" 2> "$OUT/$name.err"; local rc=$?
  echo "$name rc=$rc"
  case $rc in 124|134|137|139) echo "stopping after $name"; tail -5 "$OUT/$name.err"; exit $rc;; esac
  if grep -qi "illegal memory access" "$OUT/$name.err" "$OUT/$name.out"; then echo "GPU fault in $name"; exit 99; fi
  return $rc
}
timeout -k 10 120 rocprofv3 --list-avail > "$OUT/avail.txt" 2> "$OUT/avail.err" || { echo "rocprofv3 --list-avail failed"; exit 1; }
pick() { local o=""; for c in "$@"; do if grep -qw "$c" "$OUT/avail.txt"; then o="$o $c"; else echo "not offered: $c" >&2; fi; done; echo $o; }
P1=$(pick SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_VALU SQ_INSTS_VALU)
P2=$(pick SQ_WAIT_INST_LDS SQ_ACTIVE_INST_LDS SQ_INSTS_LDS SQ_INSTS_SALU SQ_ACTIVE_INST_ANY SQ_WAVES)
P3=$(pick SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_LDS_ADDR_CONFLICT SQ_LDS_UNALIGNED_STALL SQ_ACTIVE_INST_SCA)
for B in "$@"; do
  ARGS="--steps 3 --warmup 1 --tsteps 500 --no-cpu --large-batch 0 --mid-batch 0 --batch $B"
  [ -n "$GOPTS" ] && ARGS="$ARGS --gen-opts $GOPTS"
  echo "bench args: $ARGS" > "$OUT/command_b$B.txt"
  i=0
  for pass in "$P1" "$P2" "$P3"; do
    i=$((i+1))
    [ -z "$pass" ] && continue
    step b${B}_p$i timeout -k 10 300 rocprofv3 --pmc $pass --output-format csv -d "$OUT/b${B}_p$i" -- python3 bench.py $ARGS || { echo "pass b${B}_p$i failed"; FAILED=1; }
  done
done
exit $FAILED
