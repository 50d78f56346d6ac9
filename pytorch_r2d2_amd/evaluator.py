"""Device-side policy evaluator.

The reference has no evaluator: it prints the returns of its exploring actors
(actor.py:109-110), and so did this project (``BatchedActor.finished_returns`` are returns on the
Ape-X epsilon ladder, produced while the replay is being written).  ``BatchedEvaluator`` answers
"how good is this policy?": E envs act on the ONLINE net alone, greedily by default, and every env
records the returns of its first ``episodes_per_env`` episodes (a per-env quota; "the first N
episodes to finish" would favour short episodes).

* inference is the acting path of ``BatchedActor`` for one net (``infer.PolicyInference``:
  fused torso, x-projection GEMM, one LSTM step, head GEMM, dueling epilogue), i.e. the policy
  that acts: bf16 operands by default; ``eval.compute_dtype="fp32"`` runs the split-precision
  stages (hi / lo weight planes, fp32 carried state into the recurrence) on weights that have lo
  planes -- ``PackedWeights(split=True)`` or an fp32 learner's live weights.
* the bookkeeping is two launches of csrc/kernels/eval.hip around the device env step; their
  oracle is ``eval_ref``.
* nothing of ``HBMReplay`` is read or written, so an evaluation between two learner steps leaves
  the training run bit for bit as it was.
* no host synchronisation per step: ``run`` reads the device's episode count every ``poll_every``
  steps; the whole step replays as one HIP graph (``capture``).

Build evaluation envs with ``randomize_start=False`` so that no recorded episode is partial.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional

import numpy as np
import torch

from .config import R2D2Config
from .infer import PolicyInference, check_compute_dtype
from .ops._lib import check, kernels, ptr, stream_handle

_VP = ctypes.c_void_p


class EvalArgs(ctypes.Structure):
    """Mirror of ``struct EvalArgs`` (csrc/kernels/eval.hip); size checked against the .so."""
    _fields_ = [(name, _VP) for name in (
        "q", "eps", "act", "h_new", "c_new", "h32", "c", "h_bf", "env_done", "env_finished", "ret",
        "ep_len", "len", "n_done", "total_done", "counted_steps", "t", "ticket")] + [
        ("seed", ctypes.c_ulonglong)] + [(name, ctypes.c_int) for name in ("E", "A", "H", "K")]


def check_eval_params(n_envs: int, episodes_per_env: int, epsilon) -> np.ndarray:
    """Validate the constructor's arguments; returns the per-env float32 epsilon vector."""
    E, K = int(n_envs), int(episodes_per_env)
    if E < 1 or E > 256:
        raise ValueError(f"an evaluator drives 1 .. 256 envs (one LSTM launch), not {E}")
    if K < 1:
        raise ValueError(f"episodes_per_env must be >= 1, not {K}")
    eps = np.asarray(epsilon, dtype=np.float32)
    if eps.ndim == 0:
        eps = np.full(E, eps, dtype=np.float32)
    if eps.shape != (E,):
        raise ValueError(f"epsilon: a scalar or one value per env ({E}), not shape {eps.shape}")
    if not (np.isfinite(eps).all() and (eps >= 0).all() and (eps <= 1).all()):
        raise ValueError("epsilon must lie in [0, 1]")
    return eps


def aggregate(returns, lengths, n_done, counted_steps: int) -> Dict:
    """The result of an evaluation from its tables (pure numpy).  ``returns`` / ``lengths``
    (E, K) as the kernels left them, ``n_done`` (E) recorded episodes per env: cells at or past
    ``n_done[e]`` are not finished and come back as NaN / -1.  Statistics are over the finished
    cells, in float64 (NaN when there is none); ``complete`` iff every cell is finished."""
    n_done = np.asarray(n_done).astype(np.int64).reshape(-1)
    E = n_done.size
    ret = np.asarray(returns, dtype=np.float32).reshape(E, -1).copy()
    ln = np.asarray(lengths).astype(np.int64).reshape(E, -1).copy()
    K = ret.shape[1]
    fin = np.arange(K)[None, :] < n_done[:, None]
    ret[~fin] = np.nan
    ln[~fin] = -1
    r, l = ret[fin].astype(np.float64), ln[fin]
    some = r.size > 0
    nan = float("nan")
    return dict(mean_return=float(r.mean()) if some else nan, std_return=float(r.std()) if some else nan,
                min_return=float(r.min()) if some else nan, max_return=float(r.max()) if some else nan,
                mean_length=float(l.mean()) if some else nan, episodes=int(fin.sum()),
                env_steps=int(counted_steps), complete=bool(fin.all()), returns=ret, lengths=ln)


def make_eval_env(cfg: R2D2Config, device, n_envs: Optional[int] = None, seed: Optional[int] = None):
    """The device env of ``cfg`` (``envs.make_device_env``) for evaluation: every env starts at the
    beginning of an episode."""
    from .envs import make_device_env
    return make_device_env(cfg, int(n_envs or cfg.eval.envs), device,
                           seed=cfg.seed + cfg.eval.seed if seed is None else seed,
                           randomize_start=False)


def evaluator_from_config(cfg: R2D2Config, device, online, episodes_per_env: Optional[int] = None,
                          epsilon=None, envs: Optional[int] = None) -> "BatchedEvaluator":
    """A ``BatchedEvaluator`` on ``make_eval_env`` with ``cfg.eval``'s settings (arguments override)."""
    ec = cfg.eval
    return BatchedEvaluator(cfg, make_eval_env(cfg, device, envs), online,
                            episodes_per_env=ec.episodes_per_env if episodes_per_env is None else episodes_per_env,
                            epsilon=ec.epsilon if epsilon is None else epsilon, seed=cfg.seed + ec.seed)


class BatchedEvaluator:
    def __init__(self, cfg: R2D2Config, env, online, episodes_per_env: int = 1, epsilon=0.0,
                 seed: int = 0):
        """online: ``NetWeights`` -- a ``PackedWeights`` or ``engine_weights(engine)[0]`` (the live
        weights)."""
        for name in ("frames", "step", "reset_all", "E"):
            if not hasattr(env, name):
                raise TypeError(f"the env lacks {name!r} (the VecSyntheticAtari contract)")
        self.cfg, self.env, self.online = cfg, env, online
        m = cfg.model
        self.E = E = int(env.E)
        self.K = K = int(episodes_per_env)
        eps = check_eval_params(E, K, epsilon)
        # inference precision (eval.compute_dtype): bf16, or split precision on hi / lo weights
        check_compute_dtype("eval.compute_dtype", cfg.eval.compute_dtype, cfg, (online,))
        self.device = d = env.frames.device
        self.H, self.A = m.hidden, m.n_actions
        self.eps = torch.from_numpy(eps).to(d)
        self.seed = (int(seed) * 0x9E3779B97F4A7C15 + 0xE7A1) & ((1 << 64) - 1)
        if ctypes.sizeof(EvalArgs) != kernels().r2_eval_args_bytes():
            raise RuntimeError("EvalArgs layout differs from csrc/kernels/eval.hip")
        z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=d)  # noqa: E731
        # inference of the one net: its buffers, settings (lstm_step, n_workers) and launches
        self.infer = PolicyInference(cfg, env, ("on",), "eval.compute_dtype", d)
        self.act = z(E, dt=torch.int64)
        self.ret = z(E, K)
        self.ep_len = z(E, K, dt=torch.int32)
        self.len = z(E, dt=torch.int32)
        self.n_done = z(E, dt=torch.int32)
        self.total_done = z(1, dt=torch.int32)
        self.counted_steps = z(1, dt=torch.int64)
        self.t_d = z(1, dt=torch.int64)
        self.ticket = z(1, dt=torch.int32)
        self.steps = 0               # host mirror of t_d
        self.graph = None
        self.reset()

    def set_weights(self, online) -> None:
        """Point inference at other packed weights; a captured graph is dropped."""
        check_compute_dtype("eval.compute_dtype", self.cfg.eval.compute_dtype, self.cfg, (online,))
        self.online = online
        self.graph = None

    def reset(self) -> None:
        """Restart every env and forget everything recorded (a captured graph stays valid: it
        holds pointers only)."""
        self.env.reset_all()
        self.infer.zero_state()
        for t in (self.act, self.ret, self.ep_len, self.len, self.n_done, self.total_done,
                  self.counted_steps, self.t_d, self.ticket):
            t.zero_()
        self.steps = 0

    # ------------------------------------------------------------------ one env step
    @property
    def can_capture(self) -> bool:
        return (self.device.type == "cuda" and self.infer.fused_torso
                and getattr(self.env, "capture_safe", False))

    def _args(self) -> EvalArgs:
        a, inf = EvalArgs(), self.infer
        for name, t in (("q", inf.q["on"]), ("eps", self.eps), ("act", self.act),
                        ("h_new", inf.h32_new["on"]), ("c_new", inf.c_new["on"]),
                        ("h32", inf.h32["on"]), ("c", inf.c["on"]), ("h_bf", inf.h_bf["on"]),
                        ("ret", self.ret), ("ep_len", self.ep_len), ("len", self.len),
                        ("n_done", self.n_done), ("total_done", self.total_done),
                        ("counted_steps", self.counted_steps), ("t", self.t_d), ("ticket", self.ticket)):
            setattr(a, name, ptr(t))
        a.seed = self.seed
        a.E, a.A, a.H, a.K = self.E, self.A, self.H, self.K
        return a

    def _body(self, capturing: bool = False):
        """One env step of all E envs, device-only (no host sync, capture-safe)."""
        k = kernels()
        s = stream_handle()
        self.infer.run((("on", self.online),))
        a = self._args()
        check(k.r2_eval_act(ctypes.byref(a), s), "eval_act")
        reward, done, finished = self.env.step(self.act)
        if capturing and not (done.dtype == torch.bool and finished.dtype == torch.float32
                              and done.is_contiguous() and finished.is_contiguous()):
            raise ValueError("a captured step takes the env's persistent output buffers as they "
                             "are: done bool, finished float32, contiguous")
        self._out = (done.to(torch.bool).contiguous(), finished.float().contiguous())
        a.env_done, a.env_finished = ptr(self._out[0]), ptr(self._out[1])
        check(k.r2_eval_post(ctypes.byref(a), s), "eval_post")

    def capture(self) -> None:
        """Capture the env step into one HIP graph.  Capture executes nothing."""
        if not self.can_capture:
            raise RuntimeError("capture needs a GPU, the fused torso and a capture-safe env")
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        g = torch.cuda.CUDAGraph()
        if hasattr(self.env, "g") and not getattr(self.env, "fused", False):
            g.register_generator_state(self.env.g)     # an env whose step draws from a torch generator
        with torch.cuda.graph(g, stream=side):
            self._body(capturing=True)
        torch.cuda.current_stream(self.device).wait_stream(side)
        self.graph = g

    @torch.no_grad()
    def step(self) -> None:
        if self.graph is not None:
            self.graph.replay()
        else:
            self._body()
        self.steps += 1

    def default_max_steps(self) -> Optional[int]:
        """K episodes of the env's fixed ``episode_len`` or, where episodes vary (VecPong), of its
        ``max_episode_len``, plus one step."""
        L = getattr(self.env, "episode_len", None) or getattr(self.env, "max_episode_len", None)
        return None if L is None else self.K * int(L) + 1

    @torch.no_grad()
    def run(self, max_steps: Optional[int] = None, poll_every: int = 64) -> Dict:
        """``reset`` (unless nothing was stepped since the last one), then step until every env has
        recorded its K episodes or ``max_steps`` steps were taken (default ``default_max_steps``).  The device's episode count is read once
        every ``poll_every`` steps, nothing else syncs.  Where the env has an ``episode_len`` the
        first read falls on step K * episode_len, the earliest at which envs that all start at the
        beginning of an episode can be complete."""
        if max_steps is None:
            max_steps = self.default_max_steps()
            if max_steps is None:
                raise ValueError("max_steps is required: the env has no episode_len")
        if poll_every < 1:
            raise ValueError("poll_every must be >= 1")
        if self.steps:               # a fresh (or just reset) evaluator runs from where it stands
            self.reset()
        want = self.E * self.K
        first = self.K * int(getattr(self.env, "episode_len", 0) or 0)
        while self.steps < max_steps:
            stop = min(max_steps, first if self.steps < first else self.steps + poll_every)
            while self.steps < stop:
                self.step()
            if int(self.total_done.item()) >= want:
                break
        return self.result()

    def result(self) -> Dict:
        """The tables as they stand (syncs)."""
        out = aggregate(self.ret.cpu().numpy(), self.ep_len.cpu().numpy(), self.n_done.cpu().numpy(),
                        int(self.counted_steps.item()))
        out["steps"] = self.steps
        return out
