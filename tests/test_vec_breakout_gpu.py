"""The Breakout-like game's kernel (csrc/kernels/breakout.hip, VecBreakout) under the batched
actor (eager against captured), the evaluator (against a host count of the env's rewards) and the
drivers.  The kernel against its oracle, launch by launch, is in test_breakout_gpu.py.

Why a file of its own, named to be collected last: these tests create HIP streams (graph captures,
the concurrent driver's streams), and the runtime deals every stream of the process, a replayed
graph's branch streams included, onto a few hardware queues in turn.  Streams created by one test
therefore move the queues that a later test's graph branches get, and
test_hoist_gpu.py::test_hoisted_side_torso_takes_frames asserts that a side branch really overlaps
the main one.  Collected after every other GPU file, these tests change no other test's queues."""
import numpy as np
import pytest
import torch

from gpu_support import DEV, packed_weights
from gpu_support import stop_after_a_gpu_error  # noqa: F401
from pytorch_r2d2_amd.actor_batched import BatchedActor
from pytorch_r2d2_amd.config import get_config
from pytorch_r2d2_amd.engine.replay_hbm import HBMReplay
from pytorch_r2d2_amd.envs import VecBreakout, make_device_env
from pytorch_r2d2_amd.evaluator import BatchedEvaluator, make_eval_env
from pytorch_r2d2_amd.models import QNet
from pytorch_r2d2_amd.utils.metrics import read_jsonl
from test_breakout_ref_cpu import seven_start

pytestmark = pytest.mark.gpu


# ================================================================== under the actor and the evaluator
def _cfg(preset="reference", **over):
    kw = {"env.name": "breakout_device", "env.breakout_lives": 1, "env.breakout_max_steps": 30,
          "actor.envs_per_actor": 4}
    kw.update(over)
    return get_config(preset, **kw)


def _actor_run(cfg, graph, steps=40, E=4):
    rp = HBMReplay(cfg, torch.device(DEV, 0), capacity=E * 128, n_subrings=E)
    w = packed_weights(cfg, 0)[1]
    env = make_device_env(cfg, E, DEV, seed=3, randomize_start=False)
    assert type(env) is VecBreakout and env.fused
    actor = BatchedActor(cfg, rp, env, w, w, seed=1)
    state = env.state.cpu().numpy()       # the actor has reset the games: edit their start now
    seven_start(state)
    env.state.copy_(torch.from_numpy(state))
    if graph:
        assert actor.can_capture
        actor.capture(warmup=0)
        assert actor.graphs is not None
    for _ in range(steps):
        actor.step()
    torch.cuda.synchronize()
    out = {n: getattr(rp, n) for n in ("frames", "action", "reward", "done", "priority", "is_start", "hs_cs",
                                       "target_hs_cs", "n_valid")}
    out.update(ret_ring=actor.ret_ring, ret_cnt=actor.ret_cnt, ret_env=actor.ret_env, env_state=env.state,
               env_k=env.k, env_return=env.ep_return, env_frames=env.frames)
    return {n: t.detach().cpu() for n, t in out.items()}, list(actor.finished_returns)


def test_actor_on_breakout_eager_and_captured_agree():
    """BatchedActor on VecBreakout, E = 4, the reference preset's shapes, 40 steps: replay rows,
    starts, the returns ring and the env's state are bit-equal eager and as a replayed HIP graph,
    and a finished return is larger than 1, so the larger rewards reach the replay.

    From a fresh serve no policy scores more than 1 within 40 agent steps (the ball needs about 37
    to reach the paddle and then the lowest brick row), so the games start from an edited state
    (``seven_start``: the ball in play under a wall of its two upper rows); with one life and a cap
    of 30 every env then finishes an episode worth at least 7 whatever the actions
    (test_breakout_ref_cpu.py::test_seven_start_scores_seven_whatever_the_actions)."""
    cfg = _cfg()
    eager, rets = _actor_run(cfg, False)
    graph, rets_g = _actor_run(cfg, True)
    raw = lambda t: t.reshape(-1).view(torch.uint8)   # noqa: E731  (bits, so that NaN equals NaN)
    bad = [n for n in eager if not torch.equal(raw(eager[n]), raw(graph[n]))]
    assert not bad, bad
    assert int(eager["ret_cnt"].item()) >= 4 and rets == rets_g and max(rets) >= 7.0
    assert float(eager["reward"].max()) > 1.0, "a brick of the upper rows in the replay's rewards"
    assert int(eager["env_k"].min()) > 100 and eager["done"].any() and eager["is_start"].any()


def test_evaluator_on_breakout_counts_the_env_s_rewards():
    n, k = 4, 2
    cfg = _cfg("atari57", **{"env.breakout_max_steps": 60})
    w = packed_weights(cfg, 5)[1]
    ev = BatchedEvaluator(cfg, make_eval_env(cfg, DEV, n, seed=11), w, episodes_per_env=k, seed=11,
                          epsilon=[0.0, 0.3, 0.6, 1.0])
    assert type(ev.env) is VecBreakout and ev.can_capture and not ev.env.randomize_start
    assert ev.default_max_steps() == k * 60 + 1
    # eager, step by step: the host counts the rewards of every env's first k episodes
    count, length, ep = np.zeros((n, k), dtype=np.float32), np.zeros((n, k), dtype=np.int64), np.zeros(n, dtype=np.int64)
    for _ in range(200):
        ev.step()
        r, d = ev.env._reward.cpu().numpy(), ev.env._done.cpu().numpy()
        for e in range(n):
            if ep[e] < k:
                count[e, ep[e]] += r[e]
                length[e, ep[e]] += 1
                ep[e] += int(d[e])
        if (ep >= k).all():
            break
    res = ev.result()
    assert res["complete"] and res["episodes"] == n * k
    assert np.array_equal(res["returns"], count) and np.array_equal(res["lengths"], length)
    assert (count >= 0).all() and (length <= 60).all() and res["env_steps"] == length.sum()
    # run() as one graph per step on a fresh evaluator with the same seeds: the same evaluation
    gr = BatchedEvaluator(cfg, make_eval_env(cfg, DEV, n, seed=11), w, episodes_per_env=k, seed=11,
                          epsilon=[0.0, 0.3, 0.6, 1.0])
    gr.capture()
    out = gr.run(poll_every=16)
    assert gr.graph is not None and out["complete"]
    assert np.array_equal(out["returns"], res["returns"]) and np.array_equal(out["lengths"], res["lengths"])


# ================================================================== drivers
def _breakout_small(**over):
    kw = {"env.name": "breakout_device", "env.breakout_lives": 1, "env.breakout_max_steps": 30,
          "env.breakout_flicker": 64, "replay.burn_in": 4,
          "replay.learn": 6, "replay.overlap": 5, "replay.n_step": 3, "learner.batch_size": 8,
          "actor.envs_per_actor": 16, "eval.envs": 4, "eval.episodes_per_env": 2}
    kw.update(over)
    return get_config("pong", **kw)


def test_run_native_and_run_eval_on_breakout(tmp_path):
    """The drivers with env.name=breakout_device (one life, a cap of 30, flicker 64): run_native
    (serial, with an evaluation in it, and concurrent) ends with the engine's error word at 0 (it
    raises otherwise), run_eval and main.py --mode eval score a checkpoint."""
    import main
    from pytorch_r2d2_amd.runner import run_eval, run_native
    from pytorch_r2d2_amd.utils.checkpoint import save_reference_checkpoint
    cfg = _breakout_small()
    path = str(tmp_path / "m.jsonl")
    out = run_native(cfg, steps=6, eval_every=3, warmup_rows=16 * 40, capacity=16 * 128, log_every=3,
                     metrics_path=path)
    assert out["steps"] == 6 and np.isfinite(out["losses"]).all()
    assert out["returns"] and all(0 <= r <= 432 for r in out["returns"])
    assert [s for s, _ in out["eval_returns"]] == [3, 6] and all(0 <= r <= 432 for _, r in out["eval_returns"])
    recs = [r for r in read_jsonl(path) if r["kind"] == "eval"]
    assert all(r["complete"] and r["episodes"] == 8 for r in recs) and len(recs) == 2
    conc = run_native(cfg, steps=6, warmup_rows=16 * 40, capacity=16 * 128, log_every=3, concurrent=True)
    conc.pop("driver", None)
    assert conc["steps"] == 6 and conc["concurrent"] and np.isfinite(conc["losses"]).all()
    torch.manual_seed(3)
    net = QNet("cpu", cfg.model, cfg.env)
    ckpt = save_reference_checkpoint(net.state_dict(), 7, str(tmp_path / "save"))
    res = run_eval(cfg, ckpt)
    assert res["complete"] and res["episodes"] == 8 and res["returns"].shape == (4, 2)
    assert (res["lengths"] <= 30).all() and 0 <= res["min_return"] <= res["max_return"] <= 432
    sets = ["env.name=breakout_device", "env.breakout_lives=1", "env.breakout_max_steps=30",
            "env.breakout_flicker=64", "eval.envs=4"]
    cli = main.run(["--mode", "eval", "--config", "pong", "--checkpoint", ckpt, "--episodes", "2", "--set", *sets])
    assert np.array_equal(cli["returns"], res["returns"]) and np.array_equal(cli["lengths"], res["lengths"])
