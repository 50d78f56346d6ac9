#!/bin/bash
# Budget of the fp32 torso backward (torso_bwd_sp_kernel) at the bench shape, the inputs of
# profiles/torso_bwd_budget.txt: tools/torso_bwd_sp_probe.py's times, removal variants and stamps,
# then two counter passes (8 SQ counters each; counters only, no tracing in the same run).
# Run on the GPU box from the repo root: tools/torso_bwd_budget.sh [out dir]
set -o pipefail
export TMPDIR=/tmp
out=${1:-logs/tbwd}
mkdir -p "$out"
timeout -k 10 240 python tools/torso_bwd_sp_probe.py > "$out/probe.json" 2> "$out/probe.log" \
  || { echo "probe failed"; tail -5 "$out/probe.log"; exit 1; }
cat "$out/probe.json"
i=0
for grp in "SQ_INSTS_VALU SQ_INSTS_MFMA SQ_INSTS_LDS SQ_INSTS_SALU SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_VMEM_RD" \
           "SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_WAIT_INST_LDS SQ_ACTIVE_INST_LDS SQ_ACTIVE_INST_VALU"; do
  i=$((i+1))
  rm -rf "$out/p$i"
  timeout -k 10 180 rocprofv3 --pmc $grp --output-format csv -d "$out/p$i" -- \
    python tools/torso_bwd_sp_probe.py --pmc-run > "$out/p$i.log" 2>&1 \
    || { echo "counter pass $i failed"; tail -5 "$out/p$i.log"; exit 1; }
done
python tools/torso_bwd_sp_probe.py --summarize "$out/p*/**/*counter_collection.csv" | tee "$out/counters.txt"
