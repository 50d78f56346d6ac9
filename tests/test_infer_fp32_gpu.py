"""fp32 (split-precision) inference of the batched actor and the evaluator
(``actor.compute_dtype`` / ``eval.compute_dtype`` = "fp32", infer.PolicyInference._run_fp32) on the
GPU: Q values and next states against float64 ``QNet`` under the project's split-precision bound,
with the bf16-operand emulation as the control that must miss it; graph replay against eager
steps; the replay rows the actor writes from the fp32 states; the evaluator's bookkeeping against
``eval_ref`` on its own Q; a training run with and without fp32 evaluations in it; the drivers.

The bound (tests/test_split_gpu.py's rule, forward activations): per output
``max(2 x the error of fp32 PyTorch QNet against float64 on the same inputs, 2e-5 x max|float64|)``.
The fp32 PyTorch term is computed on the CPU here, so the bound is measured on the reference alone.

With R2D2_INFER_FP32_REPORT=<file> the measured figures are written there
(profiles/actor_fp32_oracle_errors.txt)."""
import copy

import numpy as np
import pytest
import torch

from gpu_support import (DEV, LogEnv, engine_state, np_copy, packed_weights, pong_small, qnet64,
                         report_fixture, train_with_evals)
from gpu_support import stop_after_a_gpu_error  # noqa: F401
from pytorch_r2d2_amd import actor_ref as ar
from pytorch_r2d2_amd import eval_ref as er
from pytorch_r2d2_amd import replay_ref as rr
from pytorch_r2d2_amd.actor_batched import BatchedActor
from pytorch_r2d2_amd.config import get_config
from pytorch_r2d2_amd.engine.replay_hbm import HBMReplay
from pytorch_r2d2_amd.envs.synthetic import VecSyntheticAtari
from pytorch_r2d2_amd.evaluator import BatchedEvaluator
from pytorch_r2d2_amd.models import QNet
from pytorch_r2d2_amd.utils.metrics import read_jsonl

pytestmark = pytest.mark.gpu
REL_FLOOR = 2e-5
_REPORT, _report = report_fixture(
    "R2D2_INFER_FP32_REPORT",
    "# fp32 (split-precision) inference against float64 QNet, one line per case\n"
    "# per output: largest error / bound, the largest error itself, and the bf16-operand\n"
    "#             emulation's largest error on the same inputs [in brackets]\n"
    "# bound = max(2 x |fp32 PyTorch QNet - float64|, 2e-5 x max|float64|)  (1.0 = at the bound)\n")


@pytest.fixture(autouse=True)
def _restore_device_facts():
    """The kernel library's CU count is process state that every LearnerEngine sets for its own
    stream; a run under CU masks (the concurrent driver test) leaves the learner's reduced count
    behind, and launchers called later without an engine (other test files) would refuse shapes
    that fit the whole chip.  Put back what was there."""
    from pytorch_r2d2_amd.ops._lib import kernels
    before = int(kernels().r2_get_num_cus())
    yield
    kernels().r2_set_num_cus(before)      # (an even split over the XCDs, the library's default)


SMALL = {"replay.burn_in": 4, "replay.learn": 6, "replay.overlap": 5, "replay.n_step": 3}


class Refs:
    """float64 QNet, fp32 PyTorch QNet and the bf16 emulation of one net, on the CPU."""

    def __init__(self, net):
        self.net32 = net
        self.net64 = copy.deepcopy(net).double()

    @torch.no_grad()
    def step(self, frames, h, c):
        """((q, h', c') float64, per-output bound, per-output error of the bf16 emulation)."""
        E = frames.shape[0]
        x = frames.view(1, E, *self.net32.in_shape)
        q, hs, cs = self.net64.seq_forward(x.double() / 255.0, h.double(), c.double())
        exact = (q[0], hs[0], cs[0])
        q, hs, cs = self.net32.seq_forward(x.float() / 255.0, h.float(), c.float())
        f32 = (q[0].double(), hs[0].double(), cs[0].double())
        emu = qnet64(self.net32, frames, h, c, rounded=True)
        bound = [max(2.0 * float((a - x_).abs().max()), REL_FLOOR * float(x_.abs().max()))
                 for a, x_ in zip(f32, exact)]
        return exact, bound, [float((m - x_).abs().max()) for m, x_ in zip(emu, exact)]


def _check_outputs(label, got, exact, bound, emu, worst):
    for nm, g, x, b, m in zip(("q", "h", "c"), got, exact, bound, emu):
        err = float((g.cpu().double() - x).abs().max())
        key = f"{nm}_{label[1]}"
        print(f"infer-fp32: {label[0]} {key}: error {err:.3g}, bound {b:.3g}, bf16 emulation {m:.3g}")
        worst[key] = max(worst.get(key, (0.0, 0.0, 0.0)), (err / b, err, m))
        assert err <= b, f"{label[0]} {key}: error {err:.3g}, bound {b:.3g}"
    # the control: the bf16-operand path misses this bound on Q, so the test tells the two apart
    assert emu[0] > bound[0], f"{label[0]}: the bf16 emulation is inside the bound ({emu[0]:.3g} <= {bound[0]:.3g})"


def _check_planes(o, key):
    h = o.h32_new[key]
    hi = h.bfloat16()
    assert torch.equal(o.h_bf_new[key], hi)
    assert torch.equal(o.h_lo_new[key], (h - hi.float()).bfloat16())


def _report_line(tag, worst):
    _REPORT.append(f"{tag:24s}" + "  ".join("%s %.3f (%.2e) [%.2e]" % (k, *worst[k]) for k in sorted(worst)))


# ================================================================== actor
@pytest.mark.parametrize("E", [5, 130])
def test_actor_fp32_inference_against_float64_qnet(E):
    """Atari geometry, six steps with carried state and a reset of every env after the third
    (episode_len 3).  E = 130 runs the LSTM step as two row halves of 65 per net."""
    cfg = get_config("atari57", **SMALL, **{"actor.compute_dtype": "fp32"})
    rp = HBMReplay(cfg, DEV, capacity=E * 40, n_subrings=E)
    nets = dict(zip(("on", "tg"), (packed_weights(cfg, 0, split=True), packed_weights(cfg, 1, split=True))))
    refs = {k: Refs(net) for k, (net, _) in nets.items()}
    env = VecSyntheticAtari(E, DEV, seed=4, episode_len=3, randomize_start=False)
    actor = BatchedActor(cfg, rp, env, nets["on"][1], nets["tg"][1], seed=2)
    assert actor.infer.sp and actor.infer.fused_torso
    worst = {}
    for step in range(6):
        frames = env.frames.cpu()
        carried = {k: (actor.infer.h32[k].cpu(), actor.infer.c[k].cpu()) for k in nets}
        if step == 3:
            assert all(not h.any() and not c.any() for h, c in carried.values()), "reset"
        elif step:
            assert all(h.any() for h, _ in carried.values())
        actor.step()
        torch.cuda.synchronize()
        for k in nets:
            exact, bound, emu = refs[k].step(frames, *carried[k])
            _check_outputs((f"E {E} step {step}", k), (actor.infer.q[k], actor.infer.h32_new[k], actor.infer.c_new[k]),
                           exact, bound, emu, worst)
            top = exact[0].topk(2, dim=1)
            clear = (top.values[:, 0] - top.values[:, 1]) > bound[0]
            assert torch.equal(actor.infer.q[k].cpu().argmax(dim=1)[clear], top.indices[:, 0][clear])
            _check_planes(actor.infer, k)
    _report_line(f"actor E {E}, 6 steps", worst)


def _actor(cfg, E, cap_e, seed_env=3, env_cls=VecSyntheticAtari):
    rp = HBMReplay(cfg, DEV, capacity=E * cap_e, n_subrings=E)
    _, won = packed_weights(cfg, 0, split=True)
    _, wtg = packed_weights(cfg, 1, split=True)
    env = env_cls(E, DEV, seed=seed_env, episode_len=37, randomize_start=True)
    return rp, env, BatchedActor(cfg, rp, env, won, wtg, seed=1)


def test_captured_fp32_step_replays_bit_for_bit():
    """8 replays of the captured fp32 env step against 8 eager steps from the same seeds: Q, states,
    actions and every replay column the actor writes."""
    cfg = get_config("atari57", **SMALL, **{"actor.compute_dtype": "fp32"})
    outs = []
    for graph in (False, True):
        rp, env, actor = _actor(cfg, 8, 60)
        if graph:
            assert actor.can_capture
            actor.capture(warmup=0)
            assert actor.graphs is not None
        log = []
        for _ in range(8):
            actor.step()
            log += [actor.infer.q[k].clone() for k in ("on", "tg")] + [actor.act.clone()]
        torch.cuda.synchronize()
        state = {f"log{i}": t for i, t in enumerate(log)}
        for k in ("on", "tg"):
            state.update({f"h32_{k}": actor.infer.h32[k], f"c_{k}": actor.infer.c[k], f"h32_new_{k}": actor.infer.h32_new[k],
                          f"c_new_{k}": actor.infer.c_new[k], f"h_lo_new_{k}": actor.infer.h_lo_new[k]})
        state.update(frames=rp.frames, hs_cs=rp.hs_cs, ths_cs=rp.target_hs_cs, action=rp.action,
                     reward=rp.reward, done=rp.done, priority=rp.priority, is_start=rp.is_start,
                     tree=rp.tree, n_valid=rp.n_valid)
        outs.append(state)
    bad = [k for k in outs[0] if not torch.equal(outs[0][k], outs[1][k])]
    assert not bad, bad
    assert outs[0]["hs_cs"].any() and outs[0]["priority"].any()


def test_fp32_actor_replay_rows_against_the_oracle():
    """150 steps of an fp32 BatchedActor (E 8, sub-rings of 60 rows): the stored states of the
    first 40 rows are bit for bit the carried fp32 (h32, c), and every column passes the class-level
    check of actor_ref on the logged Q values, states, actions and env outputs -- the bookkeeping
    kernels are fed the fp32 branch's buffers."""
    E, cap_e, N = 8, 60, 150
    cfg = get_config("atari57", **SMALL, **{"actor.compute_dtype": "fp32"})
    rp, env, actor = _actor(cfg, E, cap_e, env_cls=LogEnv)
    assert cfg.replay.stored_state == "pre" and actor.infer.sp
    rc, lc = cfg.replay, cfg.learner
    sp = ar.ActorSpec(E=E, A=actor.A, H=actor.H, n=actor.n, T=actor.T, stride=actor.stride, cap_e=cap_e,
                      FB=rp.frames.shape[1], R=actor.R, value_rescale=bool(lc.value_rescale),
                      gamma=actor.gamma, prio_eps=rc.priority_eps, alpha=rc.alpha,
                      vr_eps=lc.value_rescale_eps, eta=float(rc.eta), stored=rc.stored_state)
    cols = dict(frames=rp.frames, hs_cs=rp.hs_cs, ths_cs=rp.target_hs_cs, action=rp.action,
                reward=rp.reward, done=rp.done, priority=rp.priority, is_start=rp.is_start,
                n_valid=rp.n_valid, h_row=actor.h_row, h_q=actor.h_q, h_a=actor.h_a, h_r=actor.h_r,
                h_step=actor.h_step, ep_start=actor.ep_start, t=actor.t_d, head=actor.head_d,
                act=actor.act, ret_ring=actor.ret_ring[: actor.R], ret_env=actor.ret_env[: actor.R],
                ret_cnt=actor.ret_cnt)
    init = {k: np_copy(v) for k, v in cols.items()}
    init["marks"] = np_copy(actor.marks).reshape(actor.n + 2, E)
    log = {k: [] for k in ("obs", "q_on", "q_tg", "h_new", "c_new", "reward", "done", "finished", "act")}
    carried = []
    for s in range(N):
        log["obs"].append(np_copy(env.frames))
        if s < 40:
            carried.append(np.stack([np.concatenate([np_copy(actor.infer.h32[k]), np_copy(actor.infer.c[k])], axis=1)
                                     for k in ("on", "tg")]))
        actor.step()
        log["q_on"].append(np_copy(actor.infer.q["on"]))
        log["q_tg"].append(np_copy(actor.infer.q["tg"]))
        log["h_new"].append(np.stack([np_copy(actor.infer.h32_new[k]) for k in ("on", "tg")]))
        log["c_new"].append(np.stack([np_copy(actor.infer.c_new[k]) for k in ("on", "tg")]))
        r, d, f = env.outputs()
        log["reward"].append(r)
        log["done"].append(d)
        log["finished"].append(f)
        log["act"].append(np_copy(actor.act))
        if s == 39:     # rows 0 .. 39 of every sub-ring, before the ring wraps
            want = np.stack(carried)                                  # (40, 2, E, 2H)
            for i, col in enumerate((rp.hs_cs, rp.target_hs_cs)):
                got = np_copy(col).reshape(E, cap_e, -1)[:, :40].transpose(1, 0, 2)
                assert np.array_equal(got.view(np.uint32), want[:, i].view(np.uint32)), \
                    "stored states are not the carried fp32 states"
            assert want[1:].any()
    torch.cuda.synchronize()
    lg = ar.ActorLogs(**{k: np.stack(log[k]) for k in ar.ActorLogs._fields if k in log},
                      eps=np_copy(actor.eps), seed=actor.seed)
    ref = ar.ActorRef(sp, lg)
    assert np.array_equal(ref.act, np.stack(log["act"])), "chosen actions"
    want = ref.at(N)
    assert lg.done.sum() >= 2 * E and want["is_start"].sum() > E
    got = {k: np_copy(v) for k, v in cols.items()}
    got["h_valid"] = np_copy(actor.h_valid).astype(np.uint8)
    got["marks"] = np_copy(actor.marks).reshape(actor.n + 2, E)
    got["h32"] = np.stack([np_copy(actor.infer.h32[k]) for k in ("on", "tg")])
    got["c"] = np.stack([np_copy(actor.infer.c[k]) for k in ("on", "tg")])
    got["h_bf"] = np.stack([np_copy(actor.infer.h_bf[k].view(torch.int16)).view(np.uint16) for k in ("on", "tg")])
    ar.check_exact(got, want, init)
    worst = dict(reward=ar.check_reward(got["reward"], want, sp, init["reward"]))
    worst.update(ar.check_priority(got["priority"], want, sp, init["priority"]))
    leaves = np_copy(rp.tree[: rp.capacity])
    worst["leaf"] = ar.check_leaves(leaves, got["is_start"], got["priority"], want, sp)
    rr.check_tree(np_copy(rp.tree), rp.tree_offs.tolist(), rp.tree_sizes.tolist(), leaves)
    print("infer-fp32: class-level check", worst)
    assert worst["reward"] < 1.0 and worst["use"] < 1.0 and worst["leaf"] < 1.0


# ================================================================== evaluator
def test_fp32_evaluator_inference_and_bookkeeping():
    """The evaluator's one-net fp32 inference (E 5, six steps, a reset after the third) under the
    bound, and eval.hip's bookkeeping against eval_ref bit for bit on the evaluator's own Q, states
    and env outputs."""
    n, K = 5, 2
    cfg = get_config("atari57", **{"eval.compute_dtype": "fp32"})
    net, w = packed_weights(cfg, 0, split=True)
    ref = Refs(net)
    env = LogEnv(n, DEV, seed=4, episode_len=3, randomize_start=False)
    ev = BatchedEvaluator(cfg, env, w, episodes_per_env=K, seed=2)
    assert ev.infer.sp and ev.infer.fused_torso
    worst = {}
    log = {k: [] for k in ("q", "h_new", "c_new", "reward", "done", "finished")}
    for step in range(6):
        frames = env.frames.cpu()
        h, c = ev.infer.h32["on"].cpu(), ev.infer.c["on"].cpu()
        if step in (0, 3):
            assert not h.any() and not c.any(), "reset"
        else:
            assert h.any()
        ev.step()
        torch.cuda.synchronize()
        exact, bound, emu = ref.step(frames, h, c)
        _check_outputs((f"eval step {step}", "on"), (ev.infer.q["on"], ev.infer.h32_new["on"], ev.infer.c_new["on"]),
                       exact, bound, emu, worst)
        top = exact[0].topk(2, dim=1)
        clear = (top.values[:, 0] - top.values[:, 1]) > bound[0]
        act = ev.act.cpu()
        assert torch.equal(act, ev.infer.q["on"].cpu().argmax(dim=1))
        assert torch.equal(act[clear], top.indices[:, 0][clear])
        _check_planes(ev.infer, "on")
        r, d, f = env.outputs()
        for k, v in (("q", np_copy(ev.infer.q["on"])), ("h_new", np_copy(ev.infer.h32_new["on"])), ("c_new", np_copy(ev.infer.c_new["on"])),
                     ("reward", r), ("done", d), ("finished", f)):
            log[k].append(v)
        lg = er.EvalLogs(**{k: np.stack(v) for k, v in log.items()}, eps=np_copy(ev.eps), seed=ev.seed)
        got = dict(act=np_copy(ev.act), h32=np_copy(ev.infer.h32["on"]), c=np_copy(ev.infer.c["on"]),
                   h_bf=np_copy(ev.infer.h_bf["on"].view(torch.int16)).view(np.uint16), ret=np_copy(ev.ret),
                   ep_len=np_copy(ev.ep_len), n_done=np_copy(ev.n_done), len=np_copy(ev.len),
                   total_done=np_copy(ev.total_done), counted_steps=np_copy(ev.counted_steps), t=np_copy(ev.t_d))
        assert er.check(got, er.EvalRef(lg, K).at(step + 1)) == len(er.EXACT)
    res = ev.result()
    assert res["complete"] and res["episodes"] == K * n and (res["lengths"] == 3).all()
    _report_line("evaluator E 5, 6 steps", worst)


def test_run_eval_with_fp32_inference(tmp_path):
    from pytorch_r2d2_amd.runner import run_eval
    from pytorch_r2d2_amd.utils.checkpoint import save_reference_checkpoint
    cfg = pong_small(**{"eval.compute_dtype": "fp32"})
    torch.manual_seed(3)
    net = QNet("cpu", cfg.model, cfg.env)
    ckpt = save_reference_checkpoint(net.state_dict(), 7, str(tmp_path / "save"))
    path = str(tmp_path / "e.jsonl")
    res = run_eval(cfg, ckpt, metrics_path=path)
    assert res["complete"] and res["episodes"] == 8 and res["returns"].shape == (4, 2)
    assert (res["lengths"] == 12).all() and 0 <= res["min_return"] <= res["mean_return"] <= res["max_return"] <= 12
    rec, = read_jsonl(path)
    assert rec["kind"] == "eval" and rec["episodes"] == 8 and rec["mean_return"] == res["mean_return"]
    assert np.array_equal(run_eval(cfg, ckpt, use_graph=False)["returns"], res["returns"])


def test_training_is_untouched_by_fp32_evaluations(tmp_path):
    """6 learner steps, once with an fp32 evaluation of the live hi / lo weights after every step:
    master weights, optimizer moments, packed planes, priorities and the tree are bit-equal.  Then
    the driver: run_native(eval_every=2) with an fp32 evaluator logs complete evaluations."""
    fp32 = {"eval.compute_dtype": "fp32"}
    a, b = train_with_evals(False, **fp32), train_with_evals(True, **fp32)
    sa, sb = engine_state(a[0], a[1]), engine_state(b[0], b[1])
    sa.update(is_start=a[0].is_start, n_valid=a[0].n_valid)
    sb.update(is_start=b[0].is_start, n_valid=b[0].n_valid)
    bad = [k for k in sa if not torch.equal(sa[k], sb[k])]
    assert not bad, bad
    assert a[0].total_written == b[0].total_written
    assert a[1].hoist and a[1].hoisted_steps == b[1].hoisted_steps > 0
    assert len(b[2]) == 6 and np.isfinite(b[2]).all()
    from pytorch_r2d2_amd.runner import run_native
    cfg = pong_small(**{"eval.compute_dtype": "fp32"})
    path = str(tmp_path / "m.jsonl")
    out = run_native(cfg, steps=4, eval_every=2, warmup_rows=16 * 40, capacity=16 * 128, log_every=2,
                     metrics_path=path)
    assert [s for s, _ in out["eval_returns"]] == [2, 4]
    recs = [r for r in read_jsonl(path) if r["kind"] == "eval"]
    assert all(r["episodes"] == 8 and r["complete"] for r in recs) and len(recs) == 2


# ================================================================== drivers
@pytest.mark.parametrize("concurrent", [False, True], ids=["serial", "concurrent"])
def test_run_native_with_an_fp32_actor(concurrent):
    """A short pong-preset run with actor.compute_dtype=fp32.  run_native raises on a non-zero error
    word (LearnerEngine.check_errors, ConcurrentDriver.check_errors) at its end; the concurrent
    driver's words are also read here."""
    from pytorch_r2d2_amd.runner import run_native
    cfg = pong_small(**{"actor.compute_dtype": "fp32"})
    out = run_native(cfg, steps=6, actor_steps_per_update=2, warmup_rows=16 * 40, capacity=16 * 128,
                     log_every=3, concurrent=concurrent, actor_cus_per_xcd=4 if concurrent else 0,
                     check_every=3)
    assert all(np.isfinite(out["losses"])) and out["env_steps"] > 16 * 40
    if concurrent:
        drv = out["driver"]
        assert drv.actor.infer.sp and drv.w_on.pk_lo is not None
        assert drv.eng.error_word() == 0 and int(drv.err.item()) == 0
