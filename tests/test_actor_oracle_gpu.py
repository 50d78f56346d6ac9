"""The three launches of the batched actor (csrc/kernels/actor.hip) and ``BatchedActor._infer``
against the float64 oracle (pytorch_r2d2_amd/actor_ref.py).

The launches go through the ctypes entry points on the test's own tensors, in the order of
``BatchedActor._body``: pre, post, then (not deferred) mark_starts and tree_update, then tail.  Every
buffer a kernel writes sits between two runs of guard elements and starts poisoned (NaN floats,
-1 ints, 0xAB bytes) unless the kernels read it before they write it; the guards must keep
their bits, and so must every cell the oracle says is not written yet.  The per-step inputs
(Q values, states, observations, env outputs) are scripted on the host.  The cases and their
builders live in test_actor_ref_cpu.py, which also shows on the CPU that the checks reject wrong
kernels.

With R2D2_ACTOR_ORACLE_REPORT=<file> the measured figures are written there
(profiles/actor_oracle_errors.txt)."""
import ctypes

import numpy as np
import pytest
import torch

from gpu_support import (DEV, Buf, LogEnv, Tree, buf_from_host, np_copy, packed_weights, qnet64,
                         report_fixture, word)
from gpu_support import stop_after_a_gpu_error  # noqa: F401
from pytorch_r2d2_amd import actor_ref as ar
from pytorch_r2d2_amd import replay_ref as rr
from pytorch_r2d2_amd.actor_batched import ActArgs, BatchedActor
from pytorch_r2d2_amd.config import get_config
from pytorch_r2d2_amd.engine.replay_hbm import HBMReplay
from pytorch_r2d2_amd.envs.synthetic import VecSyntheticAtari
from pytorch_r2d2_amd.ops._lib import kernels, stream_handle
from test_actor_ref_cpu import CASES, check_steps, initial_flags, oracle, poison_init

pytestmark = pytest.mark.gpu

MAX_DIRTY = 512
PEND_SLACK = 32          # poisoned elements behind a pending list's capacity
_REPORT, _report = report_fixture(
    "R2D2_ACTOR_ORACLE_REPORT",
    "# actor.hip and BatchedActor._infer against actor_ref.py, one line per case\n"
    "# reward / priority / leaf : largest use of the oracle's bound (1.0 = at the bound);\n"
    "#          floor : largest share of the fp32 floor in a row's priority bound\n"
    "# infer  : largest error against float64 QNet / (2 x the error of the bf16-rounded\n"
    "#          float64 QNet), per output, and that error itself\n")


def _host(buf, like):
    return buf.bits().view(like.dtype).reshape(like.shape)


class Launches:
    """The device state of one case and the launches of one step."""

    OUT = ("frames", "hs_cs", "ths_cs", "action", "reward", "done", "priority", "is_start", "n_valid",
           "h_row", "h_q", "h_a", "h_r", "h_step", "h_valid", "ep_start", "t", "head", "act", "marks",
           "ret_ring", "ret_env", "ret_cnt", "h32", "c", "h_bf")

    def __init__(self, c):
        self.c, self.sp, self.lg = c, c["spec"], c["logs"]
        sp = self.sp
        self.init = poison_init(c)
        self.b = {k: buf_from_host(self.init[k]) for k in self.OUT}
        fl, lv, _ = initial_flags(c)
        self.tree = Tree(lv.astype(np.float32))
        self.b["dirty"] = Buf.poisoned(MAX_DIRTY, torch.int32, -1)
        self.dcount = word(0)
        z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=DEV)   # noqa: E731
        E, A, H = sp.E, sp.A, sp.H
        self.i = dict(obs=z(E, sp.FB, dt=torch.uint8), q_on=z(E, A), q_tg=z(E, A), h_new=z(2, E, H),
                      c_new=z(2, E, H), reward=z(E), done=z(E, dt=torch.bool), finished=z(E),
                      eps=torch.from_numpy(np.asarray(self.lg.eps, np.float32)).to(DEV))
        self.pend = [Buf.poisoned(sp.pend_cap + PEND_SLACK, torch.int32, -1) for _ in range(2)]
        self.pend_cnt = [word(0), word(0)]
        self.S = 0

    def args(self, parity=0, **over):
        sp, b, i = self.sp, self.b, self.i
        a = ActArgs()
        for name in ("frames", "hs_cs", "ths_cs", "action", "reward", "done", "priority", "is_start",
                     "n_valid", "h_row", "h_q", "h_a", "h_r", "h_step", "h_valid", "ep_start", "t",
                     "head", "act", "ret_ring", "ret_cnt", "ret_env", "marks", "dirty"):
            setattr(a, name, b[name].p)
        a.leaves, a.dcount = self.tree.buf.p, self.dcount.data_ptr()
        a.obs, a.q_on, a.q_tg, a.eps = (i[k].data_ptr() for k in ("obs", "q_on", "q_tg", "eps"))
        a.env_reward, a.env_done, a.env_finished = (i[k].data_ptr() for k in ("reward", "done", "finished"))
        EH = sp.E * sp.H
        for k in range(2):
            a.h_new[k], a.c_new[k] = i["h_new"][k].data_ptr(), i["c_new"][k].data_ptr()
            a.h32[k], a.c[k] = b["h32"].p + 4 * k * EH, b["c"].p + 4 * k * EH
            a.h_bf[k] = b["h_bf"].p + 2 * k * EH
            # the row stores the carried state (pre) or the state after this step (post)
            a.st_h[k], a.st_c[k] = (a.h32[k], a.c[k]) if sp.stored == "pre" else (a.h_new[k], a.c_new[k])
        a.FB, a.seed = sp.FB, self.lg.seed
        a.E, a.A, a.H, a.n, a.T, a.stride = sp.E, sp.A, sp.H, sp.n, sp.T, sp.stride
        a.cap_e, a.W, a.wrap = sp.cap_e, sp.W, int(self.S % sp.cap_e == 0)
        a.max_dirty, a.R, a.value_rescale = MAX_DIRTY, sp.R, int(sp.value_rescale)
        if sp.defer_D > 0:
            a.pend, a.pend_cnt = self.pend[parity].p, self.pend_cnt[parity].data_ptr()
            a.pend_cap, a.defer_D = sp.pend_cap, sp.defer_D
        a.ahead = sp.ahead
        a.gamma, a.gamma_n = sp.gamma, sp.gamma ** sp.n
        a.prio_eps, a.alpha, a.vr_eps = sp.prio_eps, sp.alpha, sp.vr_eps
        for k, v in over.items():
            setattr(a, k, v)
        return a

    def step(self, read_count=False):
        """One step: upload its scripted inputs, launch.  Returns the dirty count before the tail
        launch resets it (``read_count``, not deferred)."""
        sp, lg, s, k = self.sp, self.lg, self.S, kernels()
        up = lambda name, x: self.i[name].copy_(torch.from_numpy(np.ascontiguousarray(x)))   # noqa: E731
        up("obs", lg.obs[s])
        up("q_on", lg.q_on[s])
        up("q_tg", lg.q_tg[s])
        up("h_new", lg.h_new[s])
        up("c_new", lg.c_new[s])
        up("reward", lg.reward[s])
        up("done", lg.done[s])
        up("finished", lg.finished[s])
        parity = 0
        if sp.defer_D > 0:
            parity = (s // sp.round_len) % 2
            if s % sp.round_len == 0:       # a round begins: its list was applied and reset
                self.pend_cnt[parity].zero_()
                self.pend[parity].full.copy_(self.pend[parity].init)
        a = self.args(parity)
        st = stream_handle()
        assert k.r2_actor_pre(ctypes.byref(a), st) == 0
        assert k.r2_actor_post(ctypes.byref(a), st) == 0
        count = None
        if sp.defer_D == 0:
            assert k.r2_mark_starts(self.b["marks"].p, 0, sp.E * (sp.n + 2), self.b["is_start"].p,
                                    self.b["priority"].p, self.tree.buf.p, sp.T, sp.cap_e,
                                    float(np.float32(sp.eta)), self.b["n_valid"].p, self.b["dirty"].p,
                                    self.dcount.data_ptr(), MAX_DIRTY, st) == 0
            assert k.r2_tree_update(*self.tree.geom(), self.b["dirty"].p, self.dcount.data_ptr(),
                                    MAX_DIRTY, st) == 0
            if read_count:
                count = int(self.dcount.item())
        assert k.r2_actor_tail(ctypes.byref(a), st) == 0
        self.S += 1
        return count

    def got(self):
        torch.cuda.synchronize()
        for name, buf in self.b.items():
            buf.assert_guards(name)
        self.tree.buf.assert_guards("tree")
        for p in self.pend:
            p.assert_guards("pending list")
        g = {k: _host(self.b[k], self.init[k]) for k in self.OUT}
        g["leaves"] = self.tree.host()[: self.sp.cap]
        g["dirty"] = self.b["dirty"].body()
        return g

    def check(self, ref, count=None):
        sp = self.sp
        got, want = self.got(), ref.at(self.S)
        ar.check_exact(got, want, self.init)
        rep = dict(reward=ar.check_reward(got["reward"], want, sp, self.init["reward"]))
        rep.update(ar.check_priority(got["priority"], want, sp, self.init["priority"]))
        if sp.defer_D > 0:
            # the actor touches neither the flags (check_exact), the tree, the dirty list nor the marks
            self.tree.buf.assert_untouched("tree")
            self.b["dirty"].assert_untouched("dirty")
            self.b["marks"].assert_untouched("marks")
            assert int(self.dcount.item()) == 0
            for k in range(2):
                ar.check_pending(self.pend[k].body(), int(self.pend_cnt[k].item()), want["pend"][k],
                                 sp.pend_cap)
        else:
            rep["leaf"] = ar.check_leaves(got["leaves"], got["is_start"], got["priority"], want, sp)
            ar.check_dirty(got["dirty"], want, sp.cap, count)
            assert int(self.dcount.item()) == 0
            self.tree.check()
        return rep


def _line(name, worst):
    _REPORT.append("%-22s reward %.3f  priority %.3f  floor %.3f  leaf %.3f" %
                   (name, worst.get("reward", 0), worst.get("use", 0), worst.get("floor_share", 0),
                    worst.get("leaf", 0)))


@pytest.mark.parametrize("name", list(CASES))
def test_actor_launches_against_the_oracle(name):
    c = CASES[name]
    ref = oracle(c)
    run = Launches(c)
    when = set(check_steps(c))
    worst = {}
    for _ in range(c["N"]):
        checked = run.S + 1 in when
        count = run.step(read_count=checked and c["checks"] == "every")
        if checked:
            for k, v in run.check(ref, count).items():
                worst[k] = max(worst.get(k, 0.0), v)
    _line(name, worst)
    assert worst["reward"] < 1.0 and worst["use"] < 1.0 and worst.get("leaf", 0.0) < 1.0
    if c["spec"].pend_cap and c["spec"].pend_cap < c["spec"].E:
        assert int(run.pend_cnt[0].item()) > c["spec"].pend_cap      # the overflow case overflows


REFUSALS = dict(A65=dict(A=65), cap_e_W=dict(cap_e=8), cap_e_ahead_W=dict(ahead=16),
                ahead_and_deferred=dict(ahead=2, defer_D=3, pend_cap=64, _pend=True),
                deferred_no_list=dict(defer_D=3, pend_cap=64))


@pytest.mark.parametrize("name", list(REFUSALS))
def test_actor_launches_refuse_bad_arguments(name):
    """Returns -1, nothing launched: every buffer keeps its poison."""
    run = Launches(CASES["base"])
    over = dict(REFUSALS[name])
    if over.pop("_pend", False):
        over.update(pend=run.pend[0].p, pend_cnt=run.pend_cnt[0].data_ptr())
    assert run.sp.W == 8 and run.sp.cap_e == 24
    a = run.args(**over)
    assert kernels().r2_actor_pre(ctypes.byref(a), stream_handle()) == -1
    assert kernels().r2_actor_post(ctypes.byref(a), stream_handle()) == -1
    torch.cuda.synchronize()
    for nm, buf in run.b.items():
        buf.assert_untouched(nm)
    run.tree.buf.assert_untouched("tree")
    for p in run.pend:
        p.assert_untouched("pending list")
    assert int(run.dcount.item()) == 0 and int(run.pend_cnt[0].item()) == 0
    # the same arguments without the fault are accepted
    assert kernels().r2_actor_pre(ctypes.byref(run.args()), stream_handle()) == 0


# ================================================================== through the class
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_batched_actor_replay_against_the_oracle(graph):
    """150 steps of a BatchedActor (E 8, sub-rings of 60 rows): the host's choice of the wrap
    variant, mark_starts + update_tree in place and graph replay, every column against the oracle
    of the logged Q values, states, actions and env outputs."""
    E, cap_e, N = 8, 60, 150
    cfg = get_config("atari57", **{"replay.burn_in": 4, "replay.learn": 6, "replay.overlap": 5,
                                   "replay.n_step": 3})
    rp = HBMReplay(cfg, DEV, capacity=E * cap_e, n_subrings=E)
    _, won = packed_weights(cfg, 0)
    _, wtg = packed_weights(cfg, 1)
    env = LogEnv(E, DEV, seed=3, episode_len=37, randomize_start=True)
    actor = BatchedActor(cfg, rp, env, won, wtg, seed=1)
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
    if graph:
        assert actor.can_capture
        actor.capture(warmup=0)
    log = {k: [] for k in ("obs", "q_on", "q_tg", "h_new", "c_new", "reward", "done", "finished", "act")}
    for _ in range(N):
        log["obs"].append(np_copy(env.frames))
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
    assert int(rp.dirty_count.item()) == 0
    ar.check_dirty(np_copy(rp.dirty), want, sp.cap)
    rets = actor.finished_returns
    assert len(rets) == want["ret_cnt"] <= actor.R
    assert [np.float32(x) for x in rets] == [lg.finished[s, e] for s, e in ref.rets]
    assert actor._return_envs == [e for _, e in ref.rets]
    _line("class_" + ("graph" if graph else "eager"), worst)
    assert worst["reward"] < 1.0 and worst["use"] < 1.0 and worst["leaf"] < 1.0


# ================================================================== inference
def test_actor_inference_against_float64_qnet():
    """BatchedActor._infer (fused torso, bf16 x-projection, one LSTM step, head GEMM, dueling
    epilogue) on the Atari geometry, E = 5, six steps with carried state and a reset of every env
    after the third.  The path is bf16-operand by design, so its bound is measured on the
    reference alone: twice the error, per output, of float64 QNet with bf16-rounded operands
    against float64 QNet; the greedy action must be the float64 one wherever the float64 top-two
    gap exceeds the bound of Q."""
    E = 5
    cfg = get_config("atari57", **{"replay.burn_in": 4, "replay.learn": 6, "replay.overlap": 5,
                                   "replay.n_step": 3})
    rp = HBMReplay(cfg, DEV, capacity=E * 40, n_subrings=E)
    nets = dict(zip(("on", "tg"), (packed_weights(cfg, 0), packed_weights(cfg, 1))))
    env = VecSyntheticAtari(E, DEV, seed=4, episode_len=3, randomize_start=False)
    actor = BatchedActor(cfg, rp, env, nets["on"][1], nets["tg"][1], seed=2)
    assert actor.infer.fused_torso
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
        for k, (net, _) in nets.items():
            h, c = carried[k]
            exact = qnet64(net, frames, h, c, False)
            emu = qnet64(net, frames, h, c, True)
            got = (actor.infer.q[k], actor.infer.h32_new[k], actor.infer.c_new[k])
            bound_q = None
            for nm, g, x, m in zip(("q", "h", "c"), got, exact, emu):
                bound = 2.0 * float((m - x).abs().max())
                err = float((g.cpu().double() - x).abs().max())
                key = f"{nm}_{k}"
                worst[key] = max(worst.get(key, (0.0, 0.0)), (err / bound, bound / 2))
                assert err <= bound, f"step {step} {key}: error {err:.3g}, bound {bound:.3g}"
                bound_q = bound if nm == "q" else bound_q
            top = exact[0].topk(2, dim=1)
            clear = (top.values[:, 0] - top.values[:, 1]) > bound_q
            assert torch.equal(actor.infer.q[k].cpu().argmax(dim=1)[clear], top.indices[:, 0][clear])
            assert torch.equal(actor.infer.h_bf_new[k].cpu(), actor.infer.h32_new[k].cpu().bfloat16())
    _REPORT.append("infer E 5, 6 steps      " + "  ".join(
        "%s %.3f (%.2e)" % (k, *worst[k]) for k in sorted(worst)))
