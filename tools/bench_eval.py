"""Evaluator step against actor step: ms per env step of one BatchedEvaluator (one net, no replay
writes) and one BatchedActor (two nets, n-step / priorities / replay writes / tree repair) on the
same weights, in one process, the two alternating in windows of ``--steps`` graph replays
(the method of tools/bench_actor.py; ``--repeats`` windows each, so the spread of the repeated
actor windows is the yardstick for the difference).

    python tools/bench_eval.py --config atari57 --envs 64,256 --steps 300 --repeats 7
    python tools/bench_eval.py --set actor.compute_dtype=fp32 eval.compute_dtype=fp32   (fp32 acting)
Prints one JSON line; ``--out FILE`` also writes a table (profiles/eval_step_ab.txt)."""
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
from pytorch_r2d2_amd.envs.synthetic import VecSyntheticAtari  # noqa: E402
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
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--capacity", type=int, default=1 << 18)
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--set", nargs="*", default=[], metavar="KEY=VALUE",
                    help="config overrides, e.g. actor.compute_dtype=fp32 eval.compute_dtype=fp32")
    args = ap.parse_args()
    overrides = dict(kv.split("=", 1) for kv in args.set)
    dev = torch.device("cuda", 0)
    out = {"metric": "eval_vs_actor_ms_per_step", "config": args.config, "steps": args.steps,
           "repeats": args.repeats, "graph": not args.no_graph}
    lines = [f"# tools/bench_eval.py --config {args.config} --envs {args.envs} --steps {args.steps} "
             f"--repeats {args.repeats}{' --no-graph' if args.no_graph else ''}"
             f"{' --set ' + ' '.join(args.set) if args.set else ''}",
             "# ms per env step of all E envs, windows of --steps steps, actor and evaluator alternating",
             "# in one process; spread = max - min of the repeated windows",
             "# E     actor median (min .. max)        evaluator median (min .. max)     eval / actor"]
    for E in [int(v) for v in args.envs.split(",")]:
        cfg = get_config(args.config, **{**overrides, "actor.envs_per_actor": E})
        replay = HBMReplay(cfg, dev, capacity=(args.capacity // E) * E, n_subrings=E)
        eng = LearnerEngine(cfg, replay, dev)
        env = VecSyntheticAtari(E, dev, seed=1, episode_len=cfg.env.episode_len,
                                n_actions=cfg.model.n_actions,
                                n_stacks=cfg.env.channels_per_frame * cfg.env.n_stacks,
                                shape=(cfg.env.frame_h, cfg.env.frame_w))
        on, tg = engine_weights(eng)
        actor = BatchedActor(cfg, replay, env, on, tg, seed=3)
        ev = BatchedEvaluator(cfg, make_eval_env(cfg, dev, E, seed=2), on, episodes_per_env=1, seed=3)
        for _ in range(args.warmup):
            actor.step()
            ev.step()
        if not args.no_graph:
            actor.capture(warmup=1)
            ev.capture()
        for obj in (actor, ev):
            window(obj, args.warmup, dev)
        ta, te = [], []
        for _ in range(args.repeats):
            ta.append(window(actor, args.steps, dev))
            te.append(window(ev, args.steps, dev))
        ma, me = statistics.median(ta), statistics.median(te)
        out[f"E{E}"] = dict(actor_ms=round(ma, 4), actor_min=round(min(ta), 4), actor_max=round(max(ta), 4),
                            eval_ms=round(me, 4), eval_min=round(min(te), 4), eval_max=round(max(te), 4),
                            eval_over_actor=round(me / ma, 3),
                            eval_not_slower=bool(me <= ma + (max(ta) - min(ta))))
        lines.append("%-5d %.4f (%.4f .. %.4f)         %.4f (%.4f .. %.4f)          %.3f" %
                     (E, ma, min(ta), max(ta), me, min(te), max(te), me / ma))
        del actor, ev, eng, replay, env
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
