"""fp32 (split) torso backward at the bench shape (2560 learning frames, 256 workgroups): the
budget probes behind profiles/torso_bwd_budget.txt.

  (default)          time of the production launch, of the PROBE instance with nothing removed and of
                     every removal variant (r2_torso_bwd_sp_debug bits; outputs are garbage), then the
                     per-stage / per-wave clock stamps of workgroup 0.  One JSON line.
  --pmc-run          three production launches and nothing else: the workload of a counter pass
                     (rocprofv3 --pmc ... -- python tools/torso_bwd_sp_probe.py --pmc-run)
  --summarize GLOB   per-frame counter table from the counter_collection.csv files of such passes
"""
import collections
import csv
import glob
import json
import os
import sys

N_FRAMES = 2560
# removal variants: name -> r2_torso_bwd_sp_debug bits (csrc/kernels/torso_sp.hip)
VARIANTS = [("probe_instance", 0x8000), ("no_w3_staging", 4), ("no_w2_staging", 1), ("no_s1_mfma", 8),
            ("no_dw2", 16), ("no_dact1_kloop", 32), ("no_dact1_stores", 2), ("no_frame_convert", 64),
            ("no_s3", 128), ("no_prefetch", 256)]


def summarize(pattern):
    per = collections.defaultdict(lambda: collections.defaultdict(float))
    for path in sorted(glob.glob(pattern, recursive=True)):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                if "torso_bwd_sp_kernel" in row["Kernel_Name"]:
                    per[row["Counter_Name"]][row.get("Dispatch_Id", "0")] += float(row["Counter_Value"])
    c = {k: sum(v.values()) / len(v) for k, v in per.items()}
    for k in sorted(c):
        print(f"   {k:<28s} {c[k]:>12.4g}   per frame {c[k] / N_FRAMES:>10.1f}")

    def ratio(name, a, b, pct=True):
        if a in c and c.get(b):
            print(f"   {name} = {c[a] / c[b] * (100 if pct else 1):.1f}{' %' if pct else ''}")
    ratio("wait% (SQ_WAIT_ANY / SQ_WAVE_CYCLES)", "SQ_WAIT_ANY", "SQ_WAVE_CYCLES")
    ratio("waitInst% (SQ_WAIT_INST_ANY / SQ_WAVE_CYCLES)", "SQ_WAIT_INST_ANY", "SQ_WAVE_CYCLES")
    ratio("LDS bank-conflict ratio (SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE)", "SQ_LDS_BANK_CONFLICT",
          "SQ_LDS_IDX_ACTIVE")
    # matrix pipes busy = SQ_VALU_MFMA_BUSY_CYCLES / (kernel seconds x clock x 1024 SIMDs)


if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
    summarize(sys.argv[2])
    sys.exit(0)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from pytorch_r2d2_amd.ops._lib import kernels, ptr, stream_handle  # noqa: E402

DEV = "cuda"
k = kernels()
g = torch.Generator(device=DEV).manual_seed(0)
n, cap = N_FRAMES, 100_000
frames = torch.randint(0, 256, (cap, 28224), dtype=torch.uint8, device=DEV, generator=g)
rows = torch.randint(0, cap, (n,), dtype=torch.int32, device=DEV, generator=g)


def bf(*shape, relu=False):
    x = torch.randn(*shape, device=DEV, generator=g)
    return (x.relu() if relu else x).bfloat16()


a1, a1l, a2, a2l = bf(n, 400, 32, relu=True), bf(n, 400, 32), bf(n, 81, 32, relu=True), bf(n, 81, 32)
dx, dxl, o3 = bf(n, 1568), bf(n, 1568), bf(n, 1568, relu=True)
w3, w3l, w2, w2l = bf(32, 288), bf(32, 288), bf(4, 32, 128), bf(4, 32, 128)
grid = torch.cuda.get_device_properties(0).multi_processor_count
slab = torch.zeros(grid * int(k.r2_torso_bwd_slab_floats()), device=DEV)
nsl = int(k.r2_torso_bwd_slab_floats())
dst = torch.arange(nsl, dtype=torch.int32, device=DEV)
scale = torch.ones(nsl, device=DEV)
grad = torch.zeros(nsl, device=DEV)
# grad = 0: the slabs stay for the optimizer launch, as in the benchmarked step (no reduce kernel)
run = lambda: k.r2_torso_bwd_sp(ptr(frames), ptr(rows), n, ptr(a1), ptr(a1l), ptr(a2), ptr(a2l), ptr(dx),
                                ptr(dxl), ptr(o3), ptr(w3), ptr(w3l), ptr(w2), ptr(w2l), ptr(slab), grid,
                                ptr(dst), ptr(scale), 0, stream_handle())
assert run() == 0
torch.cuda.synchronize()
if len(sys.argv) > 1 and sys.argv[1] == "--pmc-run":
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    sys.exit(0)

e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed(bits, reps=20):
    """us per launch pair (torso_bwd_sp_kernel + torso_dw3_sp_kernel), best of 3 batches of reps."""
    k.r2_torso_bwd_sp_debug(bits)
    run()
    torch.cuda.synchronize()
    best = 1e30
    for _ in range(3):
        e0.record()
        for _ in range(reps):
            run()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / reps * 1e3)
    k.r2_torso_bwd_sp_debug(0)
    return round(best, 1)


for _ in range(300):   # warm-up: the first timed batch of a fresh process has read up to 13 % high
    run()
res = {"us": {"full": timed(0)}}
for name, bits in VARIANTS:
    res["us"][name] = timed(bits)
res["us"]["full_again"] = timed(0)

# stamps [wave][frame][12]: 0 loop top, 1 S0 done, 2 S1 done (barrier passed), 3 S2 done, 4 dact1 K
# loop (with the frame conversion) done + next-frame load issued, 5 S3 done, 6 dW2 done, 7 the barrier
# after the K loop passed,
# 8 dact1 epilogue + activation prefetch issued, 9 S1 tap loop done, 10 S1 epilogue done, 11 the
# barrier before the K loop passed
tr = torch.zeros(8 * 16 * 12, dtype=torch.int64, device=DEV)
k.r2_torso_bwd_sp_trace(ptr(tr))
run()
torch.cuda.synchronize()
k.r2_torso_bwd_sp_trace(0)
t = tr.view(8, 16, 12).cpu()
mx = lambda fi, j: int(t[:, fi, j].max())
stages = []
for fi in range(1, 8):
    stages.append([mx(fi, 1) - mx(fi, 0), mx(fi, 2) - mx(fi, 1), mx(fi, 3) - mx(fi, 2), mx(fi, 5) - mx(fi, 3),
                   mx(fi + 1, 0) - mx(fi, 5)])
res["stage_cycles_S0_S1_S2_S3_loop"] = stages
res["median"] = [int(np.median([r[j] for r in stages])) for j in range(5)]
res["frame_cycles"] = [mx(fi + 1, 0) - mx(fi, 0) for fi in range(1, 8)]
F = 3   # the per-wave splits below are of frame 3 of workgroup 0
d = lambda w, a, b: int(t[w, F, a] - t[w, F, b])
# S1 per wave (waves 0-5): tap loop (1 -> 9), epilogue + db2 reduction (9 -> 10), barrier (10 -> 2)
res["S1_loop_epi_barrier_per_wave"] = [[d(w, 9, 1), d(w, 10, 9), d(w, 2, 10)] for w in range(6)]
# S2 per wave: W2 DMA issue + dW2 (2 -> 6), mask rows + vmcnt(0) + barrier (6 -> 11), K loop with
# the frame conversion + next-frame load issue (11 -> 4), barrier (4 -> 7), epilogue + prefetch
# issue (7 -> 8), barrier (8 -> 3)
res["S2_dW2_bar_kloop_bar_epi_bar_per_wave"] = [[d(w, 6, 2), d(w, 11, 6), d(w, 4, 11), d(w, 7, 4), d(w, 8, 7),
                                                 d(w, 3, 8)] for w in range(8)]
print(json.dumps(res))
