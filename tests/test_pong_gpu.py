"""The Pong-like game's kernel (csrc/kernels/pong.hip) against its oracle (pytorch_r2d2_amd/
pong_ref.py), bit for bit after every agent step: state, counters, returns, outputs and every
frame byte; then the kernel under the batched actor (eager against captured), the evaluator
(against a host count of the env's rewards) and the drivers.

The launches go through the ctypes entry point on the test's own tensors.  Every buffer the kernel
writes sits between two runs of guard elements; the outputs start poisoned (NaN floats, 0xAB
bytes).  The scripted run, the proof that it covers every branch and that the comparison rejects
wrong games live in test_pong_ref_cpu.py."""
import ctypes

import numpy as np
import pytest
import torch

from gpu_support import DEV, NAN, Buf, packed_weights
from gpu_support import stop_after_a_gpu_error  # noqa: F401
from pytorch_r2d2_amd import pong_ref as pr
from pytorch_r2d2_amd.actor_batched import BatchedActor
from pytorch_r2d2_amd.config import get_config
from pytorch_r2d2_amd.engine.replay_hbm import HBMReplay
from pytorch_r2d2_amd.envs import VecPong, make_device_env
from pytorch_r2d2_amd.envs.pong_device import PongArgs
from pytorch_r2d2_amd.evaluator import BatchedEvaluator, make_eval_env
from pytorch_r2d2_amd.models import QNet
from pytorch_r2d2_amd.ops._lib import kernels, stream_handle
from pytorch_r2d2_amd.utils.metrics import read_jsonl
from test_pong_ref_cpu import RUN, SEED, STEPS, compare_run, scripted_case

pytestmark = pytest.mark.gpu

PLANE = 84 * 84


class Launch:
    """The kernel on guarded buffers that start as the oracle's arrays (state, counter, return)
    or poisoned (reward, done, finished, frames: the kernel writes every element of them)."""

    def __init__(self, ref):
        self.ref, E = ref, ref.E
        self.b = dict(state=Buf(ref.state, -1), k=Buf(ref.k, -1), ep_return=Buf(ref.ep_return, NAN),
                      reward=Buf.poisoned(E, torch.float32, NAN), done=Buf.poisoned(E, torch.uint8, 0xAB),
                      finished=Buf.poisoned(E, torch.float32, NAN),
                      frames=Buf.poisoned(E * ref.C * PLANE, torch.uint8, 0xAB))
        self.act = torch.zeros(E, dtype=torch.int64, device=DEV)

    def args(self, **over):
        ref, a = self.ref, PongArgs()
        for name, buf in self.b.items():
            setattr(a, name, buf.p)
        a.action = self.act.data_ptr()
        a.seed = ref.seed
        a.E, a.A, a.C, a.H, a.W = ref.E, 6, ref.C, 84, 84
        a.action_repeat, a.points, a.max_steps, a.lapse = ref.action_repeat, ref.points, ref.max_steps, ref.lapse
        for k, v in over.items():
            setattr(a, k, v)
        return a

    def __call__(self, act):
        self.act.copy_(torch.from_numpy(np.ascontiguousarray(act, dtype=np.int64)))
        a = self.args()
        assert kernels().r2_pong_env_step(ctypes.byref(a), stream_handle()) == 0
        torch.cuda.synchronize()
        for name, buf in self.b.items():
            buf.assert_guards(name)
        snap = self.ref.snapshot()
        return {n: self.b[n].bits().view(snap[n].dtype).reshape(snap[n].shape) for n in pr.CHECKED}

    def assert_untouched(self):
        torch.cuda.synchronize()
        for name, buf in self.b.items():
            buf.assert_untouched(name)


def test_pong_args_mirror_matches_the_library():
    assert ctypes.sizeof(PongArgs) == kernels().r2_pong_args_bytes()


def test_bitwise_run_against_the_oracle():
    """E = 3 (the smallest count at which per-env indexing can go wrong), first to 2, at most 100
    steps, the 600 scripted steps: both paddles hit, both sides score, games end on points in the
    middle of a repeat loop and at its end, and at the step cap."""
    actions, ev = scripted_case(3, STEPS, **RUN)
    assert min(ev[n] for n in ("hit_agent", "hit_opp", "point_agent", "point_opp", "wall", "done_mid_repeat",
                               "done_cap")) >= 1 and ev["done_points"] > ev["done_mid_repeat"]
    ref = compare_run(Launch, 3, actions, **RUN)
    assert ref.events == ev


@pytest.mark.parametrize("E,steps,kw", [(1, STEPS, RUN), (256, 8, dict(points=1, max_steps=5)),
                                         (3, 200, dict(RUN, action_repeat=4, n_stacks=2)),
                                         (2, 120, dict(points=1, max_steps=30, action_repeat=6, n_stacks=1))],
                         ids=["E1", "E256", "stacks2", "repeat6_stack1"])
def test_bitwise_run_other_shapes(E, steps, kw):
    """One env, more envs than one wave of workgroups has lanes (randomized starts, a step cap of 5
    so that every env resets within the 8 steps), two stacked planes of four frames, and one plane
    of six."""
    actions, _ = scripted_case(E, steps, **kw)
    ref = compare_run(Launch, E, actions, randomize_start=E == 256, **kw)
    assert ref.events["done_cap"] + ref.events["done_points"] >= 1


def test_launcher_refusals_write_nothing():
    ref = pr.PongRef(3, seed=SEED, **RUN)
    run = Launch(ref)
    k, s = kernels(), stream_handle()
    bad = dict(E0=dict(E=0), Eneg=dict(E=-3), A4=dict(A=4), A7=dict(A=7), stacks=dict(C=5), C0=dict(C=0),
               repeat=dict(action_repeat=3), repeat65=dict(action_repeat=65), H96=dict(H=96), W96=dict(W=96), swapped=dict(H=72, W=96),
               points0=dict(points=0), points43=dict(points=43), steps0=dict(max_steps=0), lapse=dict(lapse=257),
               frames=dict(frames=None), state=dict(state=None), action=dict(action=None))
    for name, over in bad.items():
        assert k.r2_pong_env_step(ctypes.byref(run.args(**over)), s) == -1, name
    assert k.r2_pong_env_step(None, s) == -1
    run.assert_untouched()
    # the same arguments without the fault are accepted
    ref.step([0, 0, 0])
    assert pr.check(run([0, 0, 0]), ref.snapshot()) == len(pr.CHECKED)


# ================================================================== under the actor and the evaluator
def _cfg(preset="reference", **over):
    kw = {"env.name": "pong_device", "env.pong_points": 1, "actor.envs_per_actor": 4}
    kw.update(over)
    return get_config(preset, **kw)


def _actor_run(cfg, graph, steps=40, E=4):
    rp = HBMReplay(cfg, torch.device(DEV, 0), capacity=E * 128, n_subrings=E)
    w = packed_weights(cfg, 0)[1]
    env = make_device_env(cfg, E, DEV, seed=3, randomize_start=False)
    assert type(env) is VecPong and env.fused
    actor = BatchedActor(cfg, rp, env, w, w, seed=1)
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


def test_actor_on_pong_eager_and_captured_agree():
    """BatchedActor on VecPong, E = 4, the reference preset's shapes, 40 steps: replay rows, starts,
    the returns ring and the env's state are bit-equal eager and as a replayed HIP graph."""
    cfg = _cfg()
    eager, rets = _actor_run(cfg, False)
    graph, rets_g = _actor_run(cfg, True)
    raw = lambda t: t.reshape(-1).view(torch.uint8)   # noqa: E731  (bits, so that NaN equals NaN)
    bad = [n for n in eager if not torch.equal(raw(eager[n]), raw(graph[n]))]
    assert not bad, bad
    assert int(eager["ret_cnt"].item()) >= 1 and rets == rets_g and set(rets) <= {-1.0, 1.0}
    assert int(eager["env_k"].min()) > 100 and eager["done"].any() and eager["is_start"].any()


def test_evaluator_on_pong_counts_the_env_s_rewards():
    n, k = 4, 2
    cfg = _cfg("atari57")
    w = packed_weights(cfg, 5)[1]
    ev = BatchedEvaluator(cfg, make_eval_env(cfg, DEV, n, seed=11), w, episodes_per_env=k, seed=11,
                          epsilon=[0.0, 0.3, 0.6, 1.0])
    assert type(ev.env) is VecPong and ev.can_capture and not ev.env.randomize_start
    assert ev.default_max_steps() == k * 5000 + 1
    # eager, step by step: the host counts the rewards of every env's first k episodes
    count, length, ep = np.zeros((n, k), dtype=np.float32), np.zeros((n, k), dtype=np.int64), np.zeros(n, dtype=np.int64)
    for _ in range(600):
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
    assert set(count.reshape(-1).tolist()) <= {-1.0, 1.0} and res["env_steps"] == length.sum()
    # run() as one graph per step on a fresh evaluator with the same seeds: the same evaluation
    gr = BatchedEvaluator(cfg, make_eval_env(cfg, DEV, n, seed=11), w, episodes_per_env=k, seed=11,
                          epsilon=[0.0, 0.3, 0.6, 1.0])
    gr.capture()
    out = gr.run(poll_every=16)
    assert gr.graph is not None and out["complete"]
    assert np.array_equal(out["returns"], res["returns"]) and np.array_equal(out["lengths"], res["lengths"])


# ================================================================== drivers
def _pong_small(**over):
    kw = {"env.name": "pong_device", "env.pong_points": 1, "env.pong_max_steps": 30, "replay.burn_in": 4,
          "replay.learn": 6, "replay.overlap": 5, "replay.n_step": 3, "learner.batch_size": 8,
          "actor.envs_per_actor": 16, "eval.envs": 4, "eval.episodes_per_env": 2}
    kw.update(over)
    return get_config("pong", **kw)


def test_run_native_and_run_eval_on_pong(tmp_path):
    """The drivers with env.name=pong_device: run_native (serial, with an evaluation in it, and
    concurrent) ends with the engine's error word at 0 (it raises otherwise), run_eval and
    main.py --mode eval score a checkpoint."""
    import main
    from pytorch_r2d2_amd.runner import run_eval, run_native
    from pytorch_r2d2_amd.utils.checkpoint import save_reference_checkpoint
    cfg = _pong_small()
    path = str(tmp_path / "m.jsonl")
    out = run_native(cfg, steps=6, eval_every=3, warmup_rows=16 * 40, capacity=16 * 128, log_every=3,
                     metrics_path=path)
    assert out["steps"] == 6 and np.isfinite(out["losses"]).all()
    assert out["returns"] and set(out["returns"]) <= {-1.0, 0.0, 1.0}
    assert [s for s, _ in out["eval_returns"]] == [3, 6] and all(-1 <= r <= 1 for _, r in out["eval_returns"])
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
    assert (res["lengths"] <= 30).all() and -1 <= res["min_return"] <= res["max_return"] <= 1
    sets = ["env.name=pong_device", "env.pong_points=1", "env.pong_max_steps=30", "eval.envs=4"]
    cli = main.run(["--mode", "eval", "--config", "pong", "--checkpoint", ckpt, "--episodes", "2", "--set", *sets])
    assert np.array_equal(cli["returns"], res["returns"]) and np.array_equal(cli["lengths"], res["lengths"])
