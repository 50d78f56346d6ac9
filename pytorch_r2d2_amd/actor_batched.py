"""MI355X-native batched actor group.

The reference runs one process per actor, each doing batch-1 inference of two nets on its own
GPU context with 4 blocking D2H copies per env step (actor.py:96-106, model.py:68-69; SURVEY
§3.2, P2).  Here ONE actor group drives E environments on a GPU:

* envs are vectorised on the device (``VecSyntheticAtari`` / ``VecCartPole``) or fed from CPU;
* inference for all E envs and BOTH nets is a handful of launches (``infer.PolicyInference``,
  shared with the evaluator): the fused uint8 torso kernel, one x-projection GEMM per net, one
  LSTM step launch covering both nets (two chains), the head GEMM + fused dueling epilogue;
* epsilon-greedy with a per-env Ape-X ladder ``eps_i = 0.4^(1 + 7 i/(N-1))`` over the global env
  index (actor.py:22);
* n-step returns, double-Q initial priorities (bootstrapped from Q(s_{t+n}), fixing Q5),
  episode-end flushes with truncated returns (fixing Q3/Q4) and sequence-start marking with
  eta-mixed priorities all happen on the device; rows are written straight into the learner's
  HBM replay (each env owns one sub-ring, so episodes are contiguous);
* weights are read from the co-located learner's packed bf16 buffers (zero-copy "broadcast"
  when actor and learner share a GPU), or from a versioned ``WeightPublisher`` slot;
* ``actor.compute_dtype="fp32"`` (default bf16) acts in split precision (csrc/split.h), the
  learner's precision: the fused split torso straight over the env's frames, split-precision
  x-projection and head GEMMs on hi / lo weight planes, the hand-off-free split LSTM step
  (csrc/kernels/lstm_step_sp.hip) on the carried fp32 state, the fp32 dueling epilogue -- still one
  launch per stage for both nets and one graph per env step.  The stored recurrent states, initial
  priorities and greedy actions then come from an fp32-accurate policy instead of a ~1e-3-relative
  one.  It needs the Atari 4x84x84 geometry, hidden <= 256 and weights with lo planes (an fp32
  learner's live weights, or ``PackedWeights(split=True)``); anything else is refused at construction.

No host synchronisation per step: the whole env step is device-only and replays as a HIP graph
(``capture``); finished-episode returns land in a device ring drained when read.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional

import numpy as np
import torch

from .config import R2D2Config, epsilon_ladder
from .engine.layout import ParamLayout
from .engine.replay_hbm import HBMReplay
from .infer import COMPUTE_DTYPES, NetWeights, PolicyInference, check_compute_dtype  # noqa: F401
from .ops._lib import check, kernels, ptr, stream_handle


_VP = ctypes.c_void_p


class ActArgs(ctypes.Structure):
    """Mirror of ``struct ActArgs`` (csrc/kernels/actor.hip); size checked against the .so."""
    _fields_ = [(name, _VP) for name in (
        "frames", "obs", "hs_cs", "ths_cs", "action", "reward", "done", "priority", "is_start",
        "leaves", "n_valid", "dirty", "dcount", "q_on", "q_tg")] + [
        (name, _VP * 2) for name in ("st_h", "st_c", "h_new", "c_new", "h32", "c", "h_bf")] + [
        (name, _VP) for name in (
            "h_row", "h_q", "h_a", "h_r", "h_step", "h_valid", "ep_start", "t", "head", "eps", "act",
            "env_reward", "env_done", "env_finished", "ret_ring", "ret_cnt", "ret_env", "marks",
            "pend", "pend_cnt")] + [
        ("FB", ctypes.c_longlong), ("seed", ctypes.c_ulonglong)] + [
        (name, ctypes.c_int) for name in ("E", "A", "H", "n", "T", "stride", "cap_e", "W", "wrap",
                                          "max_dirty", "R", "value_rescale", "pend_cap",
                                          "defer_D", "ahead")] + [
        (name, ctypes.c_float) for name in ("gamma", "gamma_n", "prio_eps", "alpha", "vr_eps")]


class PackedWeights:
    """Own packed bf16/fp32 kernel-layout copy of a QNet (for actors not co-located with the
    learner), with the fields of ``NetWeights``: ``pk``, ``pk_lo``, ``lstm_b``, ``flat``.
    ``load(state_dict)`` / ``load_flat(flat)`` repack on device.  ``split``: hold the
    bf16 layouts as (2, bf_numel) hi / lo planes (csrc/split.h, filled by ``r2_pack_split``):
    ``pk`` views the hi planes, ``pk_lo`` the lo planes (``None`` without ``split``) -- what fp32
    inference (``compute_dtype="fp32"``) reads."""

    def __init__(self, layout: ParamLayout, device, split: bool = False):
        self.L = layout
        self.split = bool(split)
        d = torch.device(device)
        self.flat = torch.zeros(layout.padded, dtype=torch.float32, device=d)
        nb = (2, layout.bf_numel) if self.split else (layout.bf_numel,)
        self.bf = torch.zeros(nb, dtype=torch.bfloat16, device=d)
        self.f32 = torch.zeros(layout.f_numel, dtype=torch.float32, device=d)
        self.bf_index = layout.bf_index.to(d)
        self.f_index = layout.f_index.to(d)
        if self.split:
            self.pk = layout.packed_views(self.bf[0], self.f32)
            self.pk_lo = layout.packed_views(self.bf[1], self.f32)
        else:
            self.pk = layout.packed_views(self.bf, self.f32)
            self.pk_lo = None
        self.lstm_b = torch.zeros(layout.G, dtype=torch.float32, device=d)
        self.version = -1

    def load_flat(self, flat: torch.Tensor, version: int = -1):
        self.flat.copy_(flat)
        k = kernels()
        s = stream_handle()
        n = self.L.bf_numel
        if self.split:
            check(k.r2_pack_split(ptr(self.flat), ptr(self.bf_index), ptr(self.bf), n, n, s), "pack_split")
        else:
            check(k.r2_pack_bf16(ptr(self.flat), ptr(self.bf_index), ptr(self.bf), n, s), "pack")
        check(k.r2_gather_f32(ptr(self.flat), ptr(self.f_index), ptr(self.f32), self.L.f_numel, s), "gather")
        torch.add(self.pk["b_ih"], self.pk["b_hh"], out=self.lstm_b)
        self.version = version

    def load(self, sd, version: int = -1):
        self.L.load_state_dict(self.flat, sd)
        self.load_flat(self.flat, version)


class BatchedActor:
    def __init__(self, cfg: R2D2Config, replay: HBMReplay, env, online, target,
                 global_env_offset: int = 0, total_envs: Optional[int] = None, seed: int = 0):
        """online/target: ``NetWeights`` of a LearnerEngine (``engine_weights(engine)``) or
        ``PackedWeights``."""
        # inference precision (actor.compute_dtype): refused here, before anything is allocated
        check_compute_dtype("actor.compute_dtype", cfg.actor.compute_dtype, cfg, (online, target))
        self.cfg, self.replay, self.env = cfg, replay, env
        self.online, self.target = online, target
        rc, m = cfg.replay, cfg.model
        self.E = E = env.E
        if E != replay.n_sub:
            raise ValueError(f"one sub-ring per env: env.E={E} replay.n_sub={replay.n_sub}")
        if E > 256:
            raise ValueError("an actor group drives <= 256 envs (one LSTM launch)")
        self.device = d = replay.device
        self.H, self.A, self.n = m.hidden, m.n_actions, rc.n_step
        self.T, self.stride = rc.seq_len, rc.overlap
        self.gamma = cfg.learner.gamma
        self.gamma_n = self.gamma ** self.n
        total = total_envs or E
        eps = [epsilon_ladder(global_env_offset + i, total, cfg.actor.eps_base, cfg.actor.eps_alpha)
               for i in range(E)]
        self.eps = torch.tensor(eps, dtype=torch.float32, device=d)
        # epsilon-greedy draws: counter-based hash of (seed, step, env) inside actor_pre_kernel
        self.seed = ((seed + 7919 * global_env_offset) * 0x9E3779B97F4A7C15 + 1) & ((1 << 64) - 1)
        A, n = self.A, self.n
        z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=d)  # noqa: E731
        # inference of both nets: its buffers, settings (lstm_step, n_workers) and launches
        self.infer = PolicyInference(cfg, env, ("on", "tg"), "actor.compute_dtype", d)
        # n-step history ring (device)
        # each env's history rows point into its own sub-ring (initially its first row), so the
        # masked scatters below never see two envs on one row
        self.h_row = (torch.arange(E, device=d, dtype=torch.int64) * replay.cap_e).repeat(n, 1)
        self.h_q = z(n, E, A)
        self.h_a = z(n, E, dt=torch.int64)
        self.h_r = z(n, E)
        self.h_step = torch.full((n, E), -1, dtype=torch.int64, device=d)
        self.h_valid = z(n, E, dt=torch.bool)
        # episode bookkeeping.  The step counter and the common sub-ring write position live on
        # the device (t_d, head_d) so one captured graph serves every step; host mirrors (t, head)
        # only pick the graph variant (the sub-ring wrap step also invalidates the old windows).
        self.t = 0                                  # actor step counter (all envs in lockstep)
        self.head = 0                               # common sub-ring write position
        self.t_d = z(1, dt=torch.int64)
        self.head_d = z(1, dt=torch.int64)
        self.ep_start = z(E, dt=torch.int64)        # actor step at which each episode started
        self.base = torch.arange(E, device=d, dtype=torch.int64) * replay.cap_e
        W = self.T + n
        self.tail_off = torch.arange(replay.cap_e - W + 1, replay.cap_e, device=d)
        # finished-episode returns: device ring + count, drained into a host list on read
        self.R = max(int(cfg.actor.return_ring), E)
        if ctypes.sizeof(ActArgs) != kernels().r2_actor_args_bytes():
            raise RuntimeError("ActArgs layout differs from csrc/kernels/actor.hip")
        self.act = z(E, dt=torch.int64)
        self.marks = z(E * (n + 2), dt=torch.int32)
        self.ret_ring = z(self.R + 1)
        self.ret_cnt = z(1, dt=torch.int64)
        self.ret_env = z(self.R + 1, dt=torch.int32)
        self._ret_read = 0
        self._returns = []
        self._return_envs = []
        self.global_env_offset = int(global_env_offset)
        self.eps_host = [float(x) for x in eps]
        self.env_steps = 0
        self.graphs = None
        # concurrent topology (engine/concurrent.py): start edits go to one of two pending lists
        # (round parity) instead of the tree, and the LSTM runs as the plain step kernel
        # (``infer.lstm_step``: no persistent co-residency requirement on the actor's few CUs)
        self.defer = None            # dict(pend=[2 x int32], cnt=[2 x int32], cap, D)
        # serial clear-ahead (actor.hip, ahead > 0): every step clears the start ``clear_ahead``
        # rows ahead of the write head instead of the row it overwrites, so a batch the learner
        # sampled before the next ``clear_ahead`` steps stays whole (LearnerEngine.cover_writes).
        # It keeps clear_ahead * E starts out of the replay.
        self.clear_ahead = A_ = int(cfg.actor.clear_ahead)
        if A_ < 0:
            raise ValueError("actor.clear_ahead must be >= 0")
        if A_ > 0:
            if replay.cap_e <= A_ + W:
                raise ValueError(f"sub-ring of {replay.cap_e} rows too small for clear_ahead {A_}")
            # a pre-filled replay starts in the invariant: no start in the first A rows of any ring
            rows = (self.base[:, None] + (self.head + torch.arange(A_, device=d))[None, :]
                    % replay.cap_e).reshape(-1)
            replay.clear_rows(rows)
            replay.flush_tree()
        if hasattr(env, "reset_all"):
            env.reset_all()

    def set_weights(self, online, target) -> None:
        """Point inference at other packed weights (captured graphs must be re-captured)."""
        check_compute_dtype("actor.compute_dtype", self.cfg.actor.compute_dtype, self.cfg,
                            (online, target))
        self.online, self.target = online, target
        self.graphs = None

    def enable_deferred(self, pend, cnt, cap: int, lookahead: int) -> None:
        """Deferred (concurrent) mode: ``pend``/``cnt`` = two pending lists + counts (round
        parity); rows are invalidated ``lookahead`` steps ahead of the write head."""
        if self.clear_ahead > 0:
            raise ValueError("actor.clear_ahead is the serial loop's rule; the concurrent driver's "
                             "lookahead does that job (build the actor with clear_ahead=0)")
        if self.replay.cap_e <= lookahead + self.T + self.n:
            raise ValueError(f"sub-ring of {self.replay.cap_e} rows too small for lookahead {lookahead}")
        self.defer = dict(pend=pend, cnt=cnt, cap=int(cap), D=int(lookahead))
        self.infer.lstm_step = True
        self.graphs = None

    @property
    def finished_returns(self):
        """Returns of the episodes finished so far (host list; syncs to drain the device ring,
        keeping at most ``actor.return_ring`` returns per drain)."""
        cnt = int(self.ret_cnt.item())
        lo = max(self._ret_read, cnt - self.R)
        if cnt > lo:
            ring = self.ret_ring[: self.R].cpu()
            envs = self.ret_env[: self.R].cpu()
            self._returns.extend(float(ring[i % self.R]) for i in range(lo, cnt))
            self._return_envs.extend(int(envs[i % self.R]) for i in range(lo, cnt))
        self._ret_read = cnt
        return self._returns

    def returns_by_epsilon(self, last: int = 256, buckets: int = 4) -> Dict[str, float]:
        """Mean return of the last ``last`` finished episodes per epsilon bucket (the Ape-X ladder
        split into ``buckets`` contiguous env ranges, keyed by the bucket's mean epsilon): the
        reference prints every actor's return next to its fixed epsilon (actor.py:109-110)."""
        rets = self.finished_returns[-last:]
        envs = self._return_envs[-len(rets):] if rets else []
        out: Dict[str, list] = {}
        for r, e in zip(rets, envs):
            b = min(buckets - 1, e * buckets // max(self.E, 1))
            lo_, hi_ = b * self.E // buckets, max(b * self.E // buckets + 1, (b + 1) * self.E // buckets)
            key = f"{sum(self.eps_host[lo_:hi_]) / (hi_ - lo_):.3g}"
            out.setdefault(key, []).append(r)
        return {k: float(np.mean(v)) for k, v in sorted(out.items(), key=lambda kv: -float(kv[0]))}

    # ------------------------------------------------------------------ inference
    def _infer(self):
        """Q values + next recurrent state of both nets for the current observations
        (``PolicyInference.run``)."""
        self.infer.run((("on", self.online), ("tg", self.target)))

    # ------------------------------------------------------------------ one env step
    @property
    def can_capture(self) -> bool:
        return (self.device.type == "cuda" and self.infer.fused_torso
                and getattr(self.env, "capture_safe", False))

    def capture(self, warmup: int = 1):
        """Capture the env step into two HIP graphs (plain step / sub-ring wrap step).  The
        warmup steps are real steps; capture itself executes nothing."""
        for _ in range(warmup):
            self.step()
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        gens = [self.env.g] if hasattr(self.env, "g") else []
        graphs, pool = {}, None
        # variants: (sub-ring wrap step?, pending-list parity) -- parity only in deferred mode
        for parity in ((0, 1) if self.defer else (0,)):
            for wrap in (False, True):
                g = torch.cuda.CUDAGraph()
                for gen in gens:
                    g.register_generator_state(gen)
                with torch.cuda.graph(g, pool=pool, stream=side):
                    self._body(wrap, parity)
                pool = g.pool()
                graphs[(wrap, parity)] = g
        torch.cuda.current_stream(self.device).wait_stream(side)
        self.graphs = graphs

    @torch.no_grad()
    def step(self, parity: int = 0):
        """One env step of every env.  ``parity``: pending list of the current round (deferred)."""
        wrap = self.head == 0
        if self.graphs is not None:
            self.graphs[(wrap, parity if self.defer else 0)].replay()
        else:
            self._body(wrap, parity)
        rp = self.replay
        self.t += 1
        self.head = (self.head + 1) % rp.cap_e
        rp.total_written += self.E
        if self.clear_ahead > 0:
            rp.covered_written += self.E
        self.env_steps += self.E

    def _args(self, wrap: bool, parity: int = 0) -> ActArgs:
        rp, rc, lc, inf = self.replay, self.cfg.replay, self.cfg.learner, self.infer
        pre = rc.stored_state == "pre"
        a = ActArgs()
        for name, t in (("frames", rp.frames), ("obs", self.env.frames), ("hs_cs", rp.hs_cs),
                        ("ths_cs", rp.target_hs_cs), ("action", rp.action), ("reward", rp.reward),
                        ("done", rp.done), ("priority", rp.priority), ("is_start", rp.is_start),
                        ("leaves", rp.tree), ("n_valid", rp.n_valid), ("dirty", rp.dirty),
                        ("dcount", rp.dirty_count), ("q_on", inf.q["on"]), ("q_tg", inf.q["tg"]),
                        ("h_row", self.h_row), ("h_q", self.h_q), ("h_a", self.h_a), ("h_r", self.h_r),
                        ("h_step", self.h_step), ("h_valid", self.h_valid), ("ep_start", self.ep_start),
                        ("t", self.t_d), ("head", self.head_d), ("eps", self.eps), ("act", self.act),
                        ("ret_ring", self.ret_ring), ("ret_cnt", self.ret_cnt), ("ret_env", self.ret_env),
                        ("marks", self.marks)):
            setattr(a, name, ptr(t))
        for i, key in enumerate(("on", "tg")):
            a.st_h[i] = ptr(inf.h32[key] if pre else inf.h32_new[key])
            a.st_c[i] = ptr(inf.c[key] if pre else inf.c_new[key])
            a.h_new[i], a.c_new[i] = ptr(inf.h32_new[key]), ptr(inf.c_new[key])
            a.h32[i], a.c[i], a.h_bf[i] = ptr(inf.h32[key]), ptr(inf.c[key]), ptr(inf.h_bf[key])
        a.FB, a.seed = rp.frames.shape[1] if rp.frame_bytes else 0, self.seed
        a.E, a.A, a.H, a.n, a.T, a.stride = self.E, self.A, self.H, self.n, self.T, self.stride
        a.cap_e, a.W, a.wrap = rp.cap_e, self.T + self.n, int(wrap)
        a.max_dirty, a.R, a.value_rescale = rp.max_dirty, self.R, int(lc.value_rescale)
        if self.defer:
            a.pend, a.pend_cnt = ptr(self.defer["pend"][parity]), ptr(self.defer["cnt"][parity])
            a.pend_cap, a.defer_D = self.defer["cap"], self.defer["D"]
        a.ahead = self.clear_ahead
        a.gamma, a.gamma_n = self.gamma, self.gamma_n
        a.prio_eps, a.alpha, a.vr_eps = rc.priority_eps, rc.alpha, lc.value_rescale_eps
        return a

    def _body(self, wrap: bool, parity: int = 0):
        """One env step for all E envs, device-only (no host sync, capture-safe): inference of
        both nets, then actor.hip's fused bookkeeping around the device env step."""
        k = kernels()
        s = stream_handle()
        if self.cfg.actor.reset_state_every_step:   # ablation: memoryless acting
            self.infer.zero_state()
        self._infer()
        a = self._args(wrap, parity)
        check(k.r2_actor_pre(ctypes.byref(a), s), "actor_pre")
        reward, done, finished = self.env.step(self.act)
        a.env_reward, a.env_finished = ptr(reward.float().contiguous()), ptr(finished.contiguous())
        a.env_done = ptr(done.to(torch.bool).contiguous())
        check(k.r2_actor_post(ctypes.byref(a), s), "actor_post")
        if not self.defer:   # deferred: the learner's stream applies the pending list
            self.replay.mark_starts(self.marks)
            self.replay.update_tree()
        check(k.r2_actor_tail(ctypes.byref(a), s), "actor_tail")

    def run(self, n_steps: int):
        for _ in range(n_steps):
            self.step()


def engine_weights(engine):
    """A LearnerEngine's live online / target packed weights as ``NetWeights`` (``pk_lo``: the lo
    planes of an fp32 engine, ``None`` on a bf16 one)."""
    return (NetWeights(engine.pk, engine.pk_lo, engine.lstm_b, engine.master),
            NetWeights(engine.pk_t, engine.pk_t_lo, engine.lstm_b_t, engine.target))
