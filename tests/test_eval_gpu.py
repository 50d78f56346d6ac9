"""The batched evaluator on the GPU: the two launches of csrc/kernels/eval.hip against the oracle
(pytorch_r2d2_amd/eval_ref.py, bit for bit), its inference against float64 ``QNet``, whole
evaluations against a host count of the env's rewards, a training run with and without
evaluations in it, and the drivers (``run_native(eval_every=)``, ``run_eval``, ``main.py --mode
eval``).

The launches go through the ctypes entry points on the test's own tensors, in the order of
``BatchedEvaluator._body``: act, then post.  Every buffer a kernel writes sits between two runs of
guard elements and starts poisoned (NaN floats, -1 ints) unless the kernels read it before they
write it.  The scripted case and its builders live in test_eval_ref_cpu.py, which also shows on
the CPU that the oracle's check rejects wrong kernels.

With R2D2_EVAL_ORACLE_REPORT=<file> the measured inference errors are written there
(profiles/eval_oracle_errors.txt)."""
import ctypes

import numpy as np
import pytest
import torch

from gpu_support import (DEV, buf_from_host, engine_state, packed_weights, pong_small, qnet64,
                         report_fixture, train_with_evals, word)
from gpu_support import stop_after_a_gpu_error  # noqa: F401
from pytorch_r2d2_amd import eval_ref as er
from pytorch_r2d2_amd.config import get_config
from pytorch_r2d2_amd.envs.synthetic import VecSyntheticAtari
from pytorch_r2d2_amd.evaluator import BatchedEvaluator, EvalArgs, make_eval_env
from pytorch_r2d2_amd.models import QNet
from pytorch_r2d2_amd.ops._lib import kernels, stream_handle
from pytorch_r2d2_amd.utils.metrics import read_jsonl
from test_eval_ref_cpu import E, EPS, H, K, LOGS, N, SIZES, poison_init

pytestmark = pytest.mark.gpu

_REPORT, _report = report_fixture(
    "R2D2_EVAL_ORACLE_REPORT",
    "# BatchedEvaluator inference (one net of infer.PolicyInference) against float64 QNet\n"
    "# per output: largest error / (2 x the error of the bf16-rounded float64 QNet),\n"
    "#             and that error itself (1.0 = at the bound)\n")


# ================================================================== 1. / 2. the launches
class Launches:
    OUT = ("act", "h32", "c", "h_bf", "ret", "ep_len", "n_done", "len", "total_done", "counted_steps", "t")

    def __init__(self, A):
        self.A, self.lg = A, LOGS[A]
        self.init = poison_init()
        self.b = {k: buf_from_host(self.init[k]) for k in self.OUT}
        self.ticket = word(0)
        z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=DEV)   # noqa: E731
        self.i = dict(q=z(E, A), h_new=z(E, H), c_new=z(E, H), done=z(E, dt=torch.bool), finished=z(E),
                      eps=torch.from_numpy(EPS).to(DEV))
        self.S = 0

    def args(self, **over):
        a = EvalArgs()
        for name in self.OUT:
            setattr(a, name, self.b[name].p)
        a.q, a.eps, a.h_new, a.c_new = (self.i[k].data_ptr() for k in ("q", "eps", "h_new", "c_new"))
        a.env_done, a.env_finished = self.i["done"].data_ptr(), self.i["finished"].data_ptr()
        a.ticket = self.ticket.data_ptr()
        a.seed = self.lg.seed
        a.E, a.A, a.H, a.K = E, self.A, H, K
        for k, v in over.items():
            setattr(a, k, v)
        return a

    def step(self):
        lg, s, k = self.lg, self.S, kernels()
        for name, x in (("q", lg.q[s]), ("h_new", lg.h_new[s]), ("c_new", lg.c_new[s]),
                        ("done", lg.done[s]), ("finished", lg.finished[s])):
            self.i[name].copy_(torch.from_numpy(np.ascontiguousarray(x)))
        a = self.args()
        assert k.r2_eval_act(ctypes.byref(a), stream_handle()) == 0
        assert k.r2_eval_post(ctypes.byref(a), stream_handle()) == 0
        self.S += 1

    def got(self):
        torch.cuda.synchronize()
        for name, buf in self.b.items():
            buf.assert_guards(name)
        return {k: self.b[k].bits().view(self.init[k].dtype).reshape(self.init[k].shape) for k in self.OUT}

    def assert_untouched(self):
        torch.cuda.synchronize()
        for name, buf in self.b.items():
            buf.assert_untouched(name)
        assert int(self.ticket.item()) == 0


def test_eval_args_mirror_matches_the_library():
    assert ctypes.sizeof(EvalArgs) == kernels().r2_eval_args_bytes()


@pytest.mark.parametrize("A", SIZES)
def test_eval_launches_against_the_oracle(A):
    ref = er.EvalRef(LOGS[A], K)
    run = Launches(A)
    assert er.check(run.got(), ref.at(0), run.init) == len(er.EXACT)
    for _ in range(N):
        run.step()
        assert er.check(run.got(), ref.at(run.S), run.init) == len(er.EXACT)
        assert int(run.ticket.item()) == 0, "the last workgroup resets the ticket"
    got = run.got()
    assert int(got["t"][0]) == N == 12
    assert got["n_done"].tolist() == [2, 0, 1, 2, 1] and int(got["total_done"][0]) == 6


REFUSALS = dict(E0=dict(E=0), A0=dict(A=0), A65=dict(A=65), H0=dict(H=0), K0=dict(K=0), Kneg=dict(K=-1))
NULLS_ACT = ("q", "eps", "act", "t")
NULLS_POST = ("h_new", "c_new", "h32", "c", "h_bf", "env_done", "env_finished", "ret", "ep_len", "len",
              "n_done", "total_done", "counted_steps", "t", "ticket")


def test_eval_launches_refuse_bad_arguments():
    """Non-zero, nothing launched: every buffer keeps its poison."""
    run = Launches(6)
    k, s = kernels(), stream_handle()
    for over in REFUSALS.values():
        a = run.args(**over)
        assert k.r2_eval_act(ctypes.byref(a), s) != 0 and k.r2_eval_post(ctypes.byref(a), s) != 0
    for name in NULLS_ACT:
        assert k.r2_eval_act(ctypes.byref(run.args(**{name: None})), s) != 0, name
    for name in NULLS_POST:
        assert k.r2_eval_post(ctypes.byref(run.args(**{name: None})), s) != 0, name
    assert k.r2_eval_act(None, s) != 0 and k.r2_eval_post(None, s) != 0
    run.assert_untouched()
    # the same arguments without the fault are accepted
    assert k.r2_eval_act(ctypes.byref(run.args()), s) == 0


# ================================================================== 3. inference
def test_evaluator_inference_against_float64_qnet():
    """The evaluator's one-net inference on the Atari geometry, E = 5, six steps with carried state
    and a reset of every env after the third (episode_len 3).  The bound is the actor test's
    (test_actor_inference_against_float64_qnet): twice the error, per output, of float64 QNet with
    bf16-rounded operands against float64 QNet; the action (epsilon 0) is the first maximum of
    the evaluator's own Q and the float64 one wherever the float64 top-two gap exceeds the bound."""
    n = 5
    cfg = get_config("atari57")
    net, w = packed_weights(cfg, 0)
    env = VecSyntheticAtari(n, DEV, seed=4, episode_len=3, randomize_start=False)
    ev = BatchedEvaluator(cfg, env, w, episodes_per_env=2, seed=2)
    assert ev.infer.fused_torso
    worst = {}
    for step in range(6):
        frames = env.frames.cpu()
        h, c = ev.infer.h32["on"].cpu(), ev.infer.c["on"].cpu()
        if step in (0, 3):
            assert not h.any() and not c.any(), "reset"
        else:
            assert h.any()
        ev.step()
        torch.cuda.synchronize()
        exact = qnet64(net, frames, h, c, False)
        emu = qnet64(net, frames, h, c, True)
        got = (ev.infer.q["on"], ev.infer.h32_new["on"], ev.infer.c_new["on"])
        bound_q = None
        for nm, g, x, m in zip(("q", "h", "c"), got, exact, emu):
            bound = 2.0 * float((m - x).abs().max())
            err = float((g.cpu().double() - x).abs().max())
            worst[nm] = max(worst.get(nm, (0.0, 0.0)), (err / bound, bound / 2))
            print(f"step {step} {nm}: error {err:.3g}, bound {bound:.3g}")
            assert err <= bound, f"step {step} {nm}: error {err:.3g}, bound {bound:.3g}"
            bound_q = bound if nm == "q" else bound_q
        top = exact[0].topk(2, dim=1)
        clear = (top.values[:, 0] - top.values[:, 1]) > bound_q
        act = ev.act.cpu()
        assert torch.equal(act, ev.infer.q["on"].cpu().argmax(dim=1))
        assert torch.equal(act[clear], top.indices[:, 0][clear])
        assert torch.equal(ev.infer.h_bf_new["on"].cpu(), ev.infer.h32_new["on"].cpu().bfloat16())
    res = ev.result()
    assert res["complete"] and res["episodes"] == 2 * n and (res["lengths"] == 3).all()
    _REPORT.append("infer E 5, 6 steps      " + "  ".join("%s %.3f (%.2e)" % (k, *worst[k]) for k in sorted(worst)))


# ================================================================== 4. end to end
def _evaluator(cfg, n, k, seed=11, **kw):
    _, w = packed_weights(cfg, 5)
    env = make_eval_env(cfg, DEV, n, seed=seed)
    return BatchedEvaluator(cfg, env, w, episodes_per_env=k, seed=seed, **kw)


@pytest.mark.parametrize("preset", ["atari57", "dmlab30"])
def test_evaluation_end_to_end(preset):
    n, L, k = 4, 8, 2
    cfg = get_config(preset, **{"env.episode_len": L})
    ev = _evaluator(cfg, n, k)
    assert ev.can_capture and ev.env.episode_len == L and not ev.env.randomize_start
    # eager, step by step: the host counts the rewards
    count = np.zeros((n, k))
    for s in range(k * L):
        target = ev.env.target.cpu().numpy().copy()
        ev.step()
        count[:, s // L] += ev.act.cpu().numpy() == target
    res = ev.result()
    assert res["complete"] and res["episodes"] == n * k and res["env_steps"] == n * k * L
    assert np.array_equal(res["returns"], count.astype(np.float32))
    assert (res["lengths"] == L).all() and res["mean_length"] == L
    assert res["mean_return"] == count.mean() and res["max_return"] == count.max()
    # run() on a fresh evaluator with the same seeds: the same evaluation, no host reads but the
    # episode count
    ev2 = _evaluator(cfg, n, k)
    again = ev2.run()
    assert ev2.steps == k * L == 16 and again["complete"] and again["episodes"] == 8
    assert np.array_equal(again["returns"], res["returns"]) and np.array_equal(again["lengths"], res["lengths"])
    # one graph per step, same seeds
    gr = _evaluator(cfg, n, k)
    gr.capture()
    out = gr.run()
    assert gr.graph is not None and gr.steps == 16 and out["complete"]
    assert np.array_equal(out["returns"], res["returns"]) and np.array_equal(out["lengths"], res["lengths"])
    assert out["env_steps"] == res["env_steps"]
    # out of steps before the quota is full (same seeds again: the first episodes are the same)
    short = _evaluator(cfg, n, k)
    short.capture()
    part = short.run(max_steps=10)
    assert short.steps == 10 and not part["complete"] and part["episodes"] == n and part["env_steps"] == 10 * n
    assert np.array_equal(part["returns"][:, 0], res["returns"][:, 0]) and np.isnan(part["returns"][:, 1]).all()
    assert (part["lengths"][:, 0] == L).all() and (part["lengths"][:, 1] == -1).all()
    # a second run restarts the envs (new episodes) and refills the tables; other weights drop the graph
    assert short.run()["complete"] and short.steps == 16
    short.set_weights(packed_weights(cfg, 6)[1])
    assert short.graph is None and short.run()["complete"]


def test_epsilon_one_acts_at_random_and_zero_never_does():
    """Per-env epsilon: env 0 greedy (always its own first maximum), env 1 with epsilon 1."""
    cfg = get_config("atari57", **{"env.episode_len": 16})
    ev = _evaluator(cfg, 2, 1, epsilon=[0.0, 1.0])
    differs = 0
    for _ in range(16):
        ev.step()
        act, greedy = ev.act.cpu(), ev.infer.q["on"].cpu().argmax(dim=1)
        assert act[0] == greedy[0]
        differs += int(act[1] != greedy[1])
    assert differs > 0


# ================================================================== 5. training is untouched
def test_training_is_untouched_by_evaluations():
    """The engine of smoke() (batch 4, burn-in 4, learn 4, 4 sub-rings, fill_synthetic), 6 learner
    steps, once with an evaluation of the live weights after every step: master weights, optimizer
    moments, packed weights, priorities and the tree are bit-equal, and so are the replay's write
    count and the number of steps that kept their pre-sampled batch."""
    a, b = train_with_evals(False), train_with_evals(True)
    sa, sb = engine_state(a[0], a[1]), engine_state(b[0], b[1])
    sa.update(is_start=a[0].is_start, n_valid=a[0].n_valid)
    sb.update(is_start=b[0].is_start, n_valid=b[0].n_valid)
    bad = [k for k in sa if not torch.equal(sa[k], sb[k])]
    assert not bad, bad
    assert a[0].total_written == b[0].total_written
    assert a[1].hoist and a[1].hoisted_steps == b[1].hoisted_steps > 0
    assert len(b[2]) == 6 and np.isfinite(b[2]).all()


# ================================================================== 6. drivers
def test_run_native_evaluates_every_n_steps(tmp_path):
    from pytorch_r2d2_amd.runner import run_native
    cfg = pong_small()
    path = str(tmp_path / "m.jsonl")
    out = run_native(cfg, steps=4, eval_every=2, warmup_rows=16 * 40, capacity=16 * 128, log_every=2,
                     metrics_path=path)
    assert [s for s, _ in out["eval_returns"]] == [2, 4]
    assert all(np.isfinite(r) for _, r in out["eval_returns"])
    recs = [r for r in read_jsonl(path) if r["kind"] == "eval"]
    assert [r["step"] for r in recs] == [2, 4]
    assert all(r["episodes"] == r["envs"] * r["episodes_per_env"] == 8 and r["complete"] for r in recs)
    assert [r["mean_return"] for r in recs] == [r for _, r in out["eval_returns"]]
    # off: no evaluator, no record
    path0 = str(tmp_path / "m0.jsonl")
    out0 = run_native(cfg, steps=2, warmup_rows=16 * 40, capacity=16 * 128, log_every=2, metrics_path=path0)
    assert out0["eval_returns"] == [] and {r["kind"] for r in read_jsonl(path0)} == {"native"}


def test_run_eval_and_main_on_a_reference_checkpoint(tmp_path):
    import main
    from pytorch_r2d2_amd.runner import run_eval
    from pytorch_r2d2_amd.utils.checkpoint import save_full_checkpoint, save_reference_checkpoint
    cfg = pong_small()
    torch.manual_seed(3)
    net = QNet("cpu", cfg.model, cfg.env)
    ckpt = save_reference_checkpoint(net.state_dict(), 7, str(tmp_path / "save"))
    path = str(tmp_path / "e.jsonl")
    res = run_eval(cfg, ckpt, metrics_path=path)
    assert res["complete"] and res["episodes"] == 8 and res["returns"].shape == (4, 2)
    assert (res["lengths"] == 12).all() and 0 <= res["min_return"] <= res["mean_return"] <= res["max_return"] <= 12
    rec, = read_jsonl(path)
    assert rec["kind"] == "eval" and rec["episodes"] == 8 and rec["mean_return"] == res["mean_return"]
    # a full-state checkpoint of the same net gives the same evaluation
    full = save_full_checkpoint(str(tmp_path / "full_last.pt"), net.state_dict(), net.state_dict(), None, 7, cfg)
    assert np.array_equal(run_eval(cfg, full, use_graph=False)["returns"], res["returns"])
    # the command line
    sets = ["replay.burn_in=4", "replay.learn=6", "replay.overlap=5", "replay.n_step=3", "learner.batch_size=8",
            "actor.envs_per_actor=16", "env.episode_len=12", "eval.envs=4"]
    out = main.run(["--mode", "eval", "--config", "pong", "--checkpoint", ckpt, "--episodes", "2", "--set", *sets])
    assert np.array_equal(out["returns"], res["returns"]) and out["mean_return"] == res["mean_return"]
    more = main.run(["--mode", "eval", "--config", "pong", "--checkpoint", ckpt, "--episodes", "1",
                     "--eval-eps", "1.0", "--set", *sets])
    assert more["episodes"] == 4 and more["complete"]
