"""Oracle of the batched evaluator's two launches (csrc/kernels/eval.hip).

Pure host code (numpy, exact integers, no torch, no GPU).  ``EvalRef(logs, K)`` takes the scripted
per-step inputs of N steps (``EvalLogs``: Q values, next recurrent state, env reward / done /
finished return, epsilons, seed) and ``EvalRef.at(S)`` is everything the launches leave behind
after S steps: the chosen actions of step S - 1, the carried state of the one net, the (E, K)
return and length tables, the per-env counters, ``total_done``, ``counted_steps`` and ``t``, and
which table cells no launch has written yet.

Rules (one env e, quota K):

* action: ``actor_ref.choose_actions`` -- greedy is the FIRST maximum of q[e, :]; the uniform of
  (seed, t, 2e) below eps[e] takes the random action of (seed, t, 2e + 1).  Uniforms are >= 0, so
  eps 0 never takes it.
* the carried state after step s is (h_new, c_new) of step s, or zero where the env was done.
* the j-th episode of env e to end (j counted from 0) is recorded in cell (e, j) while j < K:
  ``ret`` takes the env's ``finished`` value, ``ep_len`` the number of steps since the previous
  end.  Later episodes are stepped and not recorded.  ``n_done[e]`` = min(episodes ended, K),
  ``total_done`` their sum, ``len[e]`` the steps of the running episode.
* ``counted_steps``: steps taken by an env while it had fewer than K recorded episodes (the step
  that ends its K-th episode included).
* ``t`` = S.

Every output is a copy or an integer: ``check`` compares bit for bit, there is no tolerance.
The env's reward is part of the logs (it is what ``finished`` sums) but no launch reads it.

``mutation`` (tests only): a deliberately wrong variant of one rule, used on the CPU to show that
``check`` rejects it.  ``MUTATIONS`` lists them.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

from .actor_ref import choose_actions
from .refnum import as_bytes, bf16_bits

MUTATIONS = ("last_max", "past_quota", "no_state_reset", "t_twice")

_f32 = np.float32


class EvalLogs(NamedTuple):
    q: np.ndarray          # (N, E, A) float32
    h_new: np.ndarray      # (N, E, H) float32: state after the step
    c_new: np.ndarray
    reward: np.ndarray     # (N, E) float32 (not read by the launches)
    done: np.ndarray       # (N, E) bool
    finished: np.ndarray   # (N, E) float32: the finished episode's return where done
    eps: np.ndarray        # (E) float32
    seed: int


class EvalRef:
    def __init__(self, logs: EvalLogs, K: int, mutation: Optional[str] = None):
        assert mutation is None or mutation in MUTATIONS, mutation
        assert K >= 1
        self.logs, self.K, self.mut = logs, int(K), mutation
        q = np.asarray(logs.q, _f32)
        self.N, self.E, self.A = q.shape
        self.H = int(np.asarray(logs.h_new).shape[2])
        self.done = np.asarray(logs.done).astype(bool)
        amut = "last_max" if mutation == "last_max" else None
        self.act = np.stack([choose_actions(q[t], logs.eps, logs.seed, t, amut)[1]
                             for t in range(self.N)]) if self.N else np.zeros((0, self.E), np.int64)
        # episodes ended by env e before step s (exclusive prefix count), (N + 1, E)
        self.ended = np.concatenate([np.zeros((1, self.E), np.int64),
                                     np.cumsum(self.done, axis=0, dtype=np.int64)])

    def at(self, S: int) -> dict:
        lg, E, K, H = self.logs, self.E, self.K, self.H
        assert 0 <= S <= self.N
        cells = K + 1 if self.mut == "past_quota" else K       # the mutant records one more
        o = {}
        o["act"] = self.act[S - 1].copy() if S > 0 else None
        if S > 0:
            keep = np.ones(E, bool) if self.mut == "no_state_reset" else ~self.done[S - 1]
            o["h32"] = np.where(keep[:, None], np.asarray(lg.h_new[S - 1], _f32), _f32(0))
            o["c"] = np.where(keep[:, None], np.asarray(lg.c_new[S - 1], _f32), _f32(0))
        else:
            o["h32"] = o["c"] = np.zeros((E, H), _f32)
        o["carried_w"] = S > 0
        o["h_bf"] = bf16_bits(o["h32"])
        ret = np.zeros((E, K), _f32)
        ep_len = np.zeros((E, K), np.int32)
        ret_w = np.zeros((E, K), bool)
        n_done = np.zeros(E, np.int32)
        run_len = np.zeros(E, np.int32)
        counted = 0
        for e in range(E):
            ends = np.flatnonzero(self.done[:S, e]).tolist()
            prev = -1
            for j, s in enumerate(ends):
                flat = e * K + j                 # the mutant's extra episode: the next env's cell 0
                if j < cells and flat < E * K:
                    for tab, v in ((ret, lg.finished[s, e]), (ep_len, s - prev), (ret_w, True)):
                        tab.reshape(-1)[flat] = v
                prev = s
            n_done[e] = min(len(ends), cells)
            run_len[e] = S - 1 - prev
            # steps while fewer than K episodes were recorded: through the K-th end, or all S
            counted += ends[K - 1] + 1 if len(ends) >= K else S
        o["ret"], o["ep_len"], o["ret_w"] = ret, ep_len, ret_w
        o["n_done"], o["len"] = n_done, run_len
        o["total_done"] = int(n_done.sum())
        o["counted_steps"] = int(counted)
        o["t"] = 2 * S if self.mut == "t_twice" else S
        return o


# ------------------------------------------------------------------ comparison with the kernels
EXACT = ("act", "h32", "c", "h_bf", "ret", "ep_len", "n_done", "len", "total_done", "counted_steps", "t")
_SCALARS = ("total_done", "counted_steps", "t")


def check(got: dict, want: dict, init: Optional[dict] = None) -> int:
    """Every item of ``got`` (host arrays of the kernels' dtypes) against ``EvalRef.at``, bit for
    bit; table cells and state the oracle says are not written yet must equal ``init``.  Returns
    the number of items compared."""
    init = init or {}
    count = 0
    for name in EXACT:
        if name not in got:
            continue
        if want.get(name) is None:           # act before the first step: not written
            if name in init:
                assert np.array_equal(as_bytes(got[name]), as_bytes(init[name])), f"{name}: written before a step"
            count += 1
            continue
        w = np.asarray(want[name])
        g = np.asarray(got[name])
        if name in _SCALARS:
            assert int(g.reshape(-1)[0]) == int(w), f"{name}: {int(g.reshape(-1)[0])}, oracle {int(w)}"
            count += 1
            continue
        g = g.reshape(w.shape)
        assert g.dtype == w.dtype or (g.dtype.kind in "iu" and w.dtype.kind in "iu"), \
            f"{name}: {g.dtype} vs oracle {w.dtype}"
        w = w.astype(g.dtype)
        if name in ("ret", "ep_len"):
            mask = np.asarray(want["ret_w"])
        elif name in ("h32", "c", "h_bf"):
            mask = np.full(w.shape, bool(want["carried_w"]))
        else:
            mask = np.ones(w.shape, bool)
        isz = g.dtype.itemsize
        gb, wb = as_bytes(g).reshape(-1, isz), as_bytes(w).reshape(-1, isz)
        m = np.broadcast_to(mask, w.shape).reshape(-1)
        bad = np.flatnonzero(m & (gb != wb).any(axis=1))
        assert bad.size == 0, (f"{name}: cells {bad[:8]} hold {g.reshape(-1)[bad[:8]]}, "
                               f"oracle {w.reshape(-1)[bad[:8]]}")
        if name in init:
            ib = as_bytes(np.asarray(init[name]).astype(g.dtype).reshape(w.shape)).reshape(-1, isz)
            bad = np.flatnonzero(~m & (gb != ib).any(axis=1))
            assert bad.size == 0, f"{name}: cells {bad[:8]} were written but the oracle says not yet"
        count += 1
    return count
