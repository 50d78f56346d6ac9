"""fp32 (split-precision) acting against bf16 acting: ms per env step of a BatchedActor and a
BatchedEvaluator with ``compute_dtype`` fp32 next to the same objects with bf16, on the same live
weights of one fp32 LearnerEngine, in ONE process, every object a captured graph, the four
alternating in windows of ``--steps`` replays (the method of tools/bench_eval.py; ``--repeats``
windows each, so the spread of the repeated windows is the yardstick for a difference).

    python tools/bench_infer_fp32.py --config atari57 --envs 64,256 --steps 3000 --repeats 7
Prints one JSON line; ``--out FILE`` also writes a table (profiles/actor_fp32_step_ab.txt)."""
import argparse
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from pytorch_r2d2_amd.actor_batched import BatchedActor, engine_weights  # noqa: E402
from pytorch_r2d2_amd.config import get_config  # noqa: E402
from pytorch_r2d2_amd.engine.learner_engine import LearnerEngine  # noqa: E402
from pytorch_r2d2_amd.engine.replay_hbm import HBMReplay  # noqa: E402
from pytorch_r2d2_amd.envs import make_device_env  # noqa: E402
from pytorch_r2d2_amd.evaluator import BatchedEvaluator, make_eval_env  # noqa: E402


def window(obj, steps, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(steps):
        obj.step()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="atari57")
    ap.add_argument("--envs", default="64,256")
    ap.add_argument("--steps", type=int, default=3000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--capacity", type=int, default=1 << 17)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = {"metric": "fp32_vs_bf16_ms_per_step", "config": args.config, "steps": args.steps,
           "repeats": args.repeats}
    lines = [f"# tools/bench_infer_fp32.py --config {args.config} --envs {args.envs} --steps {args.steps} "
             f"--repeats {args.repeats}",
             "# ms per env step of all E envs, windows of --steps graph replays; bf16 and fp32 actor, bf16 and",
             "# fp32 evaluator alternating in one process; median (min .. max) of the repeated windows",
             "# E    object      bf16 median (min .. max)         fp32 median (min .. max)          fp32 / bf16"]
    for E in [int(v) for v in args.envs.split(",")]:
        objs, keep = {}, []
        base = get_config(args.config, **{"actor.envs_per_actor": E})
        eng_rp = HBMReplay(base, dev, capacity=(args.capacity // E) * E, n_subrings=E)
        eng = LearnerEngine(base, eng_rp, dev)
        on, tg = engine_weights(eng)
        for dt in ("bf16", "fp32"):
            cfg = get_config(args.config, **{"actor.envs_per_actor": E, "actor.compute_dtype": dt,
                                             "eval.compute_dtype": dt})
            rp = eng_rp if dt == "bf16" else HBMReplay(cfg, dev, capacity=(args.capacity // E) * E,
                                                       n_subrings=E)
            actor = BatchedActor(cfg, rp, make_device_env(cfg, E, dev, seed=1), on, tg, seed=3)
            ev = BatchedEvaluator(cfg, make_eval_env(cfg, dev, E, seed=2), on, episodes_per_env=1, seed=3)
            for _ in range(args.warmup):
                actor.step()
                ev.step()
            actor.capture(warmup=1)
            ev.capture()
            objs[("actor", dt)], objs[("eval", dt)] = actor, ev
            keep += [rp, cfg]
        for o in objs.values():
            window(o, args.warmup, dev)
        t = {k: [] for k in objs}
        for _ in range(args.repeats):
            for k, o in objs.items():
                t[k].append(window(o, args.steps, dev))
        for name in ("actor", "eval"):
            b, f = t[(name, "bf16")], t[(name, "fp32")]
            mb, mf = statistics.median(b), statistics.median(f)
            out[f"E{E}_{name}"] = dict(bf16_ms=round(mb, 4), bf16_min=round(min(b), 4), bf16_max=round(max(b), 4),
                                       fp32_ms=round(mf, 4), fp32_min=round(min(f), 4), fp32_max=round(max(f), 4),
                                       fp32_over_bf16=round(mf / mb, 3))
            lines.append("%-5d %-10s  %.4f (%.4f .. %.4f)         %.4f (%.4f .. %.4f)          %.3f" %
                         (E, name, mb, min(b), max(b), mf, min(f), max(f), mf / mb))
        del objs, eng, eng_rp, keep
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
