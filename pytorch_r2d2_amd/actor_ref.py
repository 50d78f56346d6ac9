"""Float64 oracle of the batched actor's bookkeeping kernels (csrc/kernels/actor.hip).

Pure host code (numpy float64 for arithmetic, exact integers for bookkeeping, no torch, no GPU).
The kernels keep an n-slot history ring per env and act on it step by step; the oracle does not.
It works from per-env trajectories: ``ActorRef(spec, logs)`` cuts every env's done log into
episodes and gives, in closed form, for every step s the time at which its transition is
finalised and what it holds then, and for every episode its sequence starts and the time each
is marked.  ``ActorRef.at(S)`` is the whole state after S steps: what every replay column, the
carried recurrent state, the history arrays, the marks, the return ring and the pending lists
must hold, and which cells no launch has written yet.  The ``check_*`` functions compare what
the kernels left in memory with it; tests/test_actor_oracle_gpu.py runs the three launches
through them, tests/test_actor_ref_cpu.py checks the oracle against a brute-force simulation
(one object per env with a deque) and shows that the checks reject every entry of ``MUTATIONS``.

Definitions (episode covering steps ep0 .. ep0 + L - 1 of one env, transition of step s):

* horizon m = min(n, ep0 + L - s); R = sum_{i<m} gamma^i r_{s+i}; done iff ep0 + L - s <= n;
  y = h(R + gamma_n h^-1(q_tg[s+n][argmax q_on[s+n]])), or h(R) when done; priority
  (|q_on[s][a_s] - y| + prio_eps)^alpha.  It is finalised at step s + n (not done) or at the
  episode's last step (done); until then its reward / done / priority cells keep what the ring
  held.  gamma, gamma_n = fp32(gamma^n), prio_eps, alpha, vr_eps and eta are the float32 values
  the kernel receives, taken as float64.
* starts: offsets o on the stride grid with o + T <= L, plus L - T when L >= T.  A grid start
  whose last row is finalised by the n-step rule (o + T - 1 + n <= L - 1) is marked at step
  ep0 + o + T - 1 + n, every other one at the episode's last step.  The write head invalidates:
  plain mode clears the row it reaches and, when it is at row 0, rows cap_e - W + 1 .. cap_e - 1
  (W = T + n); clear-ahead clears the row ``ahead`` rows in front of it; deferred mode applies
  nothing and appends ``row`` (mark) / ``-2 - row`` (clear, D rows ahead) to the pending list.

Bounds (u = 2^-24).  Derived here, not fitted to a run:

* everything integer-valued or copied (frames, states, actions, flags, marks, counters, ring
  entries, the bf16 copy of h) is compared for equality.
* reward (``check_reward``): |R_kernel - R_64| <= c_R u sum_i |gamma^i r_i|, c_R = n + 5: what a
  kernel needs that adds n terms r * powf(gamma, k) in fp32 (powf two ulp = 4 u, an assumption;
  one rounding per product and per partial sum a term passes through: (n + 4) u per term, one u
  to spare).  actor.hip sums in double and rounds once (at most u |R|, a use of 1 / (n + 5)):
  the priority bound below has no term for the return's own error, and an fp32 sum of rewards
  that cancel (+-1e3 beside +-1e-3) misses it by an order of magnitude.
* priority (``check_priority``), in TD-error space: d = priority^(1/alpha) - prio_eps in float64,
  |d - |delta_64|| <= 4 u (|q| + |R| + gamma_n |h^-1(boot)|) + (4 u / alpha)(|delta_64| + prio_eps)
  + floor.  The first term is td_ref.delta_bound's (two roundings of the target, one of the
  difference, one to spare); the second is powf's two ulp and the rounding of the stored
  priority carried through the inverse power (d(p^(1/alpha)) = (1/alpha) p^(1/alpha) dp/p).
  floor is 0 without value rescaling.  With it, the closed forms cancel in fp32 (h^-1 twice:
  absolute error of the order of 1e-4 at vr_eps = 1e-3), which no count of roundings describes;
  floor is then twice the error of a numpy float32 evaluation of the same closed forms
  (``h32`` / ``h_inv32``: td_ref.h / h_inv as written) against float64 on the same element's
  inputs -- measured on the reference alone, never on the kernel.
* leaves of marked starts (``check_leaves``): replay_ref.leaf_bound(T) around
  replay_ref.seq_leaf of the kernel's own priorities (a start stays flagged only while the
  priorities of its window are the ones it was marked with, see ``ActorRef``).

``mutation`` (tests only): a deliberately wrong variant of one rule, used on the CPU to show that
the checks reject it.  ``MUTATIONS`` lists them.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

from . import replay_ref as rr
from . import td_ref
from .refnum import as_bytes, bf16_bits

MUTATIONS = ("boot_argmax_tg", "terminal_bootstraps", "gamma_n_minus_1", "done_last_row_only",
             "no_final_start", "final_start_on_grid", "start_one_step_early", "last_max",
             "random_reuses_first_uniform", "stored_post", "no_state_reset", "ret_reverse_env_order")

U24 = 2.0 ** -24
_BIG = 1 << 60
_f32 = np.float32


class ActorSpec(NamedTuple):
    E: int
    A: int
    H: int
    n: int
    T: int
    stride: int
    cap_e: int
    FB: int
    R: int
    value_rescale: bool = False
    gamma: float = 0.997
    prio_eps: float = 1e-6
    alpha: float = 0.9
    vr_eps: float = 1e-3
    eta: float = 0.9
    stored: str = "pre"          # which recurrent state a row stores: before or after its step
    ahead: int = 0               # clear-ahead mode: rows in front of the head
    ctor_clears: bool = False    # clear-ahead: rows 0 .. ahead - 1 cleared before the first step
    defer_D: int = 0             # deferred mode: rows in front of the head
    pend_cap: int = 0
    round_len: int = 1           # deferred: steps per round; round r appends to list r % 2,
    #                              whose count is reset when the round begins

    @property
    def W(self):
        return self.T + self.n

    @property
    def cap(self):
        return self.E * self.cap_e

    def f32(self, name):
        """The float32 the kernel receives for a parameter, as float64."""
        v = self.gamma ** self.n if name == "gamma_n" else getattr(self, name)
        return float(_f32(v))


class ActorLogs(NamedTuple):
    obs: np.ndarray        # (N, E, FB) uint8
    q_on: np.ndarray       # (N, E, A) float32
    q_tg: np.ndarray
    h_new: np.ndarray      # (N, 2, E, H) float32: state after the step, online / target
    c_new: np.ndarray
    reward: np.ndarray     # (N, E) float32
    done: np.ndarray       # (N, E) bool
    finished: np.ndarray   # (N, E) float32: the finished episode's return where done
    eps: np.ndarray        # (E) float32
    seed: int


def h32(x, eps):
    """td_ref.h as written, every operation in float32."""
    x = np.asarray(x, dtype=_f32)
    one = _f32(1.0)
    return (np.sign(x) * (np.sqrt(np.abs(x) + one) - one) + _f32(eps) * x).astype(_f32)


def h_inv32(x, eps):
    """td_ref.h_inv as written, every operation in float32."""
    x = np.asarray(x, dtype=_f32)
    one, e = _f32(1.0), _f32(eps)
    s = (np.sqrt(one + _f32(4.0) * e * (np.abs(x) + one + e)) - one) / (_f32(2.0) * e)
    return (np.sign(x) * (s * s - one)).astype(_f32)


def choose_actions(q_on, eps, seed: int, t: int, mutation: Optional[str] = None):
    """(greedy, chosen) of one step: first maximum; u = uniform(seed, t, 2e) < eps[e] (float32)
    takes min(int(float32(u') * A), A - 1) with u' = uniform(seed, t, 2e + 1)."""
    q = np.asarray(q_on, dtype=_f32)
    E, A = q.shape
    if mutation == "last_max":
        greedy = A - 1 - np.argmax(q[:, ::-1], axis=1)
    else:
        greedy = np.argmax(q, axis=1)
    e = np.arange(E)
    u = rr.uniform(seed, t, 2 * e)
    u2 = u if mutation == "random_reuses_first_uniform" else rr.uniform(seed, t, 2 * e + 1)
    ra = np.minimum((u2 * _f32(A)).astype(_f32).astype(np.int64), A - 1)
    return greedy.astype(np.int64), np.where(u < np.asarray(eps, dtype=_f32), ra, greedy).astype(np.int64)


class ActorRef:
    """Everything the actor's launches leave behind, from the logs of N steps.

    Per step s and env e (arrays (N, E)): ``ep0`` / ``end`` of its episode (end = a huge number
    while the episode runs past the log), ``tfin`` the step whose launches finalise it, and its
    float64 ``R``, ``Rabs`` = sum |gamma^i r|, ``term``, ``boot`` (q_tg before h^-1, 0 when
    terminal), ``q_sel``, ``y``, ``delta``, ``prio``.  tfin never decreases along an env's steps,
    so the finalised steps of an env are a prefix and a ring row holds the last of them that
    maps to it.  A start is cleared when the head reaches its row (or earlier); the priority of
    a row of its window is rewritten only after the head has passed that row, which is no
    earlier: a flagged start's window holds the priorities it was marked with."""

    def __init__(self, spec: ActorSpec, logs: ActorLogs, mutation: Optional[str] = None,
                 flags0=None, leaves0=None, n_valid0: int = 0):
        assert mutation is None or mutation in MUTATIONS, mutation
        self.spec, self.logs, self.mut = spec, logs, mutation
        sp = spec
        N = self.N = int(np.asarray(logs.done).shape[0])
        E, n = sp.E, sp.n
        self.flags0 = np.zeros(sp.cap, np.uint8) if flags0 is None else np.asarray(flags0, np.uint8)
        self.leaves0 = np.zeros(sp.cap) if leaves0 is None else np.asarray(leaves0, np.float64)
        self.n_valid0 = int(n_valid0)
        self.g, self.gn = sp.f32("gamma"), sp.f32("gamma_n")
        if mutation == "gamma_n_minus_1":
            self.gn = float(_f32(sp.gamma ** (n - 1)))
        self.peps, self.alpha, self.veps, self.eta = (sp.f32(k) for k in ("prio_eps", "alpha", "vr_eps", "eta"))
        done = np.asarray(logs.done).astype(bool)
        # actions
        self.greedy = np.zeros((N, E), np.int64)
        self.act = np.zeros((N, E), np.int64)
        for t in range(N):
            self.greedy[t], self.act[t] = choose_actions(logs.q_on[t], logs.eps, logs.seed, t, mutation)
        # episodes
        self.ep0 = np.zeros((N, E), np.int64)
        self.end = np.full((N, E), _BIG, np.int64)
        self.episodes = []           # per env: list of (ep0, end or _BIG)
        for e in range(E):
            ends = np.flatnonzero(done[:, e]).tolist()
            first, eps_ = 0, []
            for x in ends + [_BIG]:
                hi = min(x, N - 1)
                if first <= hi:
                    self.ep0[first: hi + 1, e] = first
                    self.end[first: hi + 1, e] = x
                    eps_.append((first, x))
                first = x + 1
            self.episodes.append(eps_)
        s = np.arange(N)[:, None]
        left = self.end - s + 1                      # steps left in the episode, s included
        self.term = left <= n
        self.tfin = np.where(self.term, self.end, s + n)
        self._transitions()
        self._starts()
        self._returns()
        # the finalised prefix of every env as a function of S: fin_count[S][e]
        self._carried()

    # ------------------------------------------------------------------ transitions
    def _transitions(self):
        sp, lg, N = self.spec, self.logs, self.N
        E, n = sp.E, sp.n
        r = np.asarray(lg.reward, np.float64)
        self.R = np.zeros((N, E))
        self.Rabs = np.zeros((N, E))
        self.boot = np.zeros((N, E))
        self.q_sel = np.zeros((N, E))
        self.known = self.tfin < N                   # finalised within the log
        self.done_flag = self.term.copy()
        if self.mut == "done_last_row_only":
            self.done_flag = self.end == np.arange(N)[:, None]
        boots = np.zeros((N, E), bool)
        for s in range(N):
            for e in range(E):
                if not self.known[s, e]:
                    continue
                m = int(min(n, self.end[s, e] - s + 1))
                terms = [self.g ** i * r[s + i, e] for i in range(m)]
                self.R[s, e] = float(np.sum(terms))
                self.Rabs[s, e] = float(np.sum(np.abs(terms)))
                self.q_sel[s, e] = float(lg.q_on[s, e, self.act[s, e]])
                b = None
                if not self.term[s, e]:
                    b = s + n
                elif self.mut == "terminal_bootstraps":
                    b = int(self.end[s, e])
                if b is not None:
                    if self.mut == "boot_argmax_tg":
                        a = int(np.argmax(lg.q_tg[b, e]))
                    else:
                        a = int(self.greedy[b, e])
                    self.boot[s, e] = float(lg.q_tg[b, e, a])
                    boots[s, e] = True
        self.boots = boots
        bv = td_ref.h_inv(self.boot, self.veps) if sp.value_rescale else self.boot
        self.bv = np.where(boots, bv, 0.0)
        y = self.R + self.gn * self.bv
        self.y = td_ref.h(y, self.veps) if sp.value_rescale else y
        self.delta = self.q_sel - self.y
        self.prio = (np.abs(self.delta) + self.peps) ** self.alpha

    # ------------------------------------------------------------------ starts
    def _starts(self):
        """self.marks: per env a list of (time, row in the sub-ring, slot of the marks array,
        first step of the window)."""
        sp, N = self.spec, self.N
        T, n, st = sp.T, sp.n, sp.stride
        self.marks = []
        for e in range(sp.E):
            out = []
            for ep0, end in self.episodes[e]:
                running = end >= _BIG
                L = (N - ep0 + n + T) if running else end - ep0 + 1     # running: long enough
                offs = set(range(0, max(L - T + 1, 0), st))
                if not running and L >= T:
                    offs.add(L - T)
                    if self.mut == "no_final_start" or (self.mut == "final_start_on_grid" and (L - T) % st):
                        offs.discard(L - T)
                for o in sorted(offs):
                    if o % st == 0 and o + T - 1 + n <= L - 1:
                        time, slot = ep0 + o + T - 1 + n, 0
                        if self.mut == "start_one_step_early":
                            time -= 1
                    else:
                        time, slot = end, 1 + (L - T - o)
                    if time < N:
                        out.append((int(time), int((ep0 + o) % sp.cap_e), int(slot), int(ep0 + o)))
            self.marks.append(out)

    def _clears(self, s: int):
        """Rows of a sub-ring the pre launch of step s invalidates."""
        sp = self.spec
        if sp.defer_D > 0:
            return [(s + sp.defer_D) % sp.cap_e]
        if sp.ahead > 0:
            return [(s + sp.ahead) % sp.cap_e]
        rows = [s % sp.cap_e]
        if s % sp.cap_e == 0:
            rows += list(range(sp.cap_e - sp.W + 1, sp.cap_e))
        return rows

    def _leaf(self, e: int, first: int) -> float:
        """replay_ref.seq_leaf of the start whose window begins at step ``first``."""
        sp = self.spec
        ring = np.zeros(sp.cap_e)
        steps = first + np.arange(sp.T)
        ring[steps % sp.cap_e] = self.prio[np.minimum(steps, self.N - 1), e]
        return rr.seq_leaf(ring, int(first % sp.cap_e), sp.T, sp.cap_e, self.eta)

    # ------------------------------------------------------------------ return ring, carried state
    def _returns(self):
        done = np.asarray(self.logs.done).astype(bool)
        self.rets = []               # (step, env) in ring order
        for s in range(self.N):
            envs = np.flatnonzero(done[s]).tolist()
            if self.mut == "ret_reverse_env_order":
                envs = envs[::-1]
            self.rets += [(s, e) for e in envs]
        self.ret_upto = np.concatenate([[0], np.cumsum(done.sum(axis=1))]).astype(np.int64)

    def _carried(self):
        lg = self.logs
        done = np.asarray(lg.done).astype(bool)
        keep = np.ones_like(done) if self.mut == "no_state_reset" else ~done
        m = keep[:, None, :, None]
        self.h_after = np.where(m, np.asarray(lg.h_new, _f32), _f32(0))    # carried after step s
        self.c_after = np.where(m, np.asarray(lg.c_new, _f32), _f32(0))

    def stored_state(self, s: int):
        """(h, c) (2, E, H) stored with the row of step s."""
        post = (self.spec.stored == "post") != (self.mut == "stored_post")
        if post:
            return np.asarray(self.logs.h_new[s], _f32), np.asarray(self.logs.c_new[s], _f32)
        if s == 0:
            z = np.zeros_like(np.asarray(self.logs.h_new[0], _f32))
            return z, z
        return self.h_after[s - 1], self.c_after[s - 1]

    def pending_of(self, s: int):
        """Entries step s appends to its pending list (deferred mode), sorted."""
        sp = self.spec
        out = []
        for e in range(sp.E):
            base = e * sp.cap_e
            out += [-2 - (base + r) for r in self._clears(s)]
            out += [base + row for time, row, _, _ in self.marks[e] if time == s]
        return sorted(out)

    # ------------------------------------------------------------------ the state after S steps
    def at(self, S: int) -> dict:
        sp, lg = self.spec, self.logs
        E, n, cap_e, cap, H, A = sp.E, sp.n, sp.cap_e, sp.cap, sp.H, sp.A
        assert 0 <= S <= self.N
        o = {}
        # rows written: the last step s < S with s % cap_e == p
        p = np.arange(cap_e)
        last = np.where(S - 1 >= p, p + cap_e * ((S - 1 - p) // cap_e), -1)
        o["row_w"] = np.tile(last >= 0, E)
        frames = np.zeros((cap, sp.FB), np.uint8)
        hs = np.zeros((2, cap, 2 * H), _f32)
        action = np.zeros(cap, np.uint8)
        for s in sorted(set(last[last >= 0].tolist())):
            rows = np.arange(E) * cap_e + s % cap_e
            frames[rows] = lg.obs[s]
            h, c = self.stored_state(s)
            hs[:, rows, :H] = h
            hs[:, rows, H:] = c
            action[rows] = self.act[s].astype(np.uint8)
        o["frames"], o["hs_cs"], o["ths_cs"], o["action"] = frames, hs[0], hs[1], action
        # finalised transitions: per env the prefix with tfin <= S - 1
        for k in ("fin", "term"):
            o[k] = np.zeros(cap, bool)
        for k in ("reward", "reward_abs", "priority", "q_sel", "boot", "bv", "delta"):
            o[k] = np.zeros(cap)
        o["done"] = np.zeros(cap, np.uint8)
        o["step"] = np.full(cap, -1, np.int64)
        for e in range(E):
            F = int(np.searchsorted(self.tfin[:, e], S - 1, side="right"))
            src = np.where(F - 1 >= p, p + cap_e * ((F - 1 - p) // cap_e), -1)
            ok = src >= 0
            rows, ss = e * cap_e + p[ok], src[ok]
            o["fin"][rows] = True
            o["step"][rows] = ss
            o["term"][rows] = self.boots[ss, e] == 0
            o["done"][rows] = self.done_flag[ss, e]
            for k, a in (("reward", self.R), ("reward_abs", self.Rabs), ("priority", self.prio),
                         ("q_sel", self.q_sel), ("boot", self.boot), ("bv", self.bv), ("delta", self.delta)):
                o[k][rows] = a[ss, e]
        # flags, leaves, n_valid, dirty rows of the last step, pending lists
        flags, leaves, n_valid = self.flags0.copy(), self.leaves0.copy(), self.n_valid0
        marked = np.zeros(cap, bool)          # flags the actor's own marks set
        deferred = sp.defer_D > 0
        dirty, appends = set(), 0
        if not deferred:
            if sp.ahead > 0 and sp.ctor_clears:
                for e in range(E):
                    for r in range(sp.ahead):
                        n_valid -= int(flags[e * cap_e + r] != 0)
                        flags[e * cap_e + r], leaves[e * cap_e + r] = 0, 0.0
            by_time = {}
            for e in range(E):
                for time, row, _, first in self.marks[e]:
                    if time < S:
                        by_time.setdefault(time, []).append((e, row, first))
            for s in range(S):
                lastst = s == S - 1
                for e in range(E):
                    for r in self._clears(s):
                        g = e * cap_e + r
                        if flags[g] != 0 or leaves[g] != 0:
                            n_valid -= int(flags[g] != 0)
                            flags[g], leaves[g], marked[g] = 0, 0.0, False
                            if lastst:
                                dirty.add(g)
                                appends += 1
                for e, row, first in by_time.get(s, ()):
                    g = e * cap_e + row
                    n_valid += int(flags[g] == 0)
                    flags[g], leaves[g], marked[g] = 1, self._leaf(e, first), True
                    if lastst:
                        dirty.add(g)
                        appends += 1
        o["is_start"], o["leaves"], o["n_valid"], o["marked"] = flags, leaves, n_valid, marked
        o["dirty_last"], o["dcount"] = np.asarray(sorted(dirty), np.int64), appends
        o["pend"] = [[], []]
        if deferred and S > 0:
            cur = (S - 1) // sp.round_len
            for rnd in (cur - 1, cur):
                if rnd >= 0:
                    ent = []
                    for s in range(rnd * sp.round_len, min((rnd + 1) * sp.round_len, S)):
                        ent += self.pending_of(s)
                    o["pend"][rnd % 2] = sorted(ent)
        # marks of the last step
        o["marks"] = None
        if not deferred and S > 0:
            mk = np.full((n + 2, E), -1, np.int32)
            for e in range(E):
                for time, row, slot, _ in self.marks[e]:
                    if time == S - 1:
                        mk[slot, e] = e * cap_e + row
            o["marks"] = mk
        # n-step history: slot j holds the last step s < S with s % n == j
        j = np.arange(n)
        hl = np.where(S - 1 >= j, j + n * ((S - 1 - j) // n), -1)
        o["h_w"] = np.repeat((hl >= 0)[:, None], E, axis=1)
        o["h_row"], o["h_a"] = np.zeros((n, E), np.int64), np.zeros((n, E), np.int64)
        o["h_step"] = np.full((n, E), -1, np.int64)
        o["h_q"], o["h_r"] = np.zeros((n, E, A), _f32), np.zeros((n, E), _f32)
        o["h_valid"] = np.zeros((n, E), np.uint8)
        for jj, s in enumerate(hl.tolist()):
            if s >= 0:
                o["h_row"][jj] = np.arange(E) * cap_e + s % cap_e
                o["h_a"][jj], o["h_step"][jj] = self.act[s], s
                o["h_q"][jj], o["h_r"][jj] = lg.q_on[s], lg.reward[s]
                o["h_valid"][jj] = self.tfin[s] > S - 1
        # episode bookkeeping, counters, chosen actions
        o["ep_start"] = np.zeros(E, np.int64)
        for e in range(E):
            ends = [x for _, x in self.episodes[e] if x < S]
            o["ep_start"][e] = ends[-1] + 1 if ends else 0
        o["t"], o["head"] = S, S % cap_e
        o["act"] = self.act[S - 1].copy() if S > 0 else None
        # return ring
        cnt = int(self.ret_upto[S])
        o["ret_cnt"] = cnt
        o["ret_ring"], o["ret_env"] = np.zeros(sp.R, _f32), np.zeros(sp.R, np.int32)
        o["ret_w"] = np.zeros(sp.R, bool)
        for i in range(max(0, cnt - sp.R), cnt):
            s, e = self.rets[i]
            o["ret_ring"][i % sp.R], o["ret_env"][i % sp.R] = lg.finished[s, e], e
            o["ret_w"][i % sp.R] = True
        # carried state
        o["carried_w"] = S > 0
        if S > 0:
            o["h32"], o["c"] = self.h_after[S - 1], self.c_after[S - 1]
        else:
            o["h32"] = o["c"] = np.zeros((2, E, H), _f32)
        o["h_bf"] = bf16_bits(o["h32"])
        return o


# ------------------------------------------------------------------ comparison with the kernels
EXACT = ("frames", "hs_cs", "ths_cs", "action", "done", "is_start", "h_row", "h_a", "h_step", "h_q",
         "h_r", "h_valid", "ep_start", "t", "head", "act", "marks", "ret_ring", "ret_env", "ret_cnt",
         "h32", "c", "h_bf", "n_valid")
_ROW_MASK = dict(frames="row_w", hs_cs="row_w", ths_cs="row_w", action="row_w", done="fin",
                 h_row="h_w", h_a="h_w", h_step="h_w", h_q="h_w", h_r="h_w", ret_ring="ret_w",
                 ret_env="ret_w")


def _rows_equal(name, got, want, mask, init):
    """``got`` equals ``want`` bit for bit where ``mask`` (leading axes), ``init`` elsewhere."""
    want = np.asarray(want)
    got = np.asarray(got).reshape(want.shape)
    assert got.dtype == want.dtype, f"{name}: {got.dtype} vs oracle {want.dtype}"
    lead = mask.shape
    g = as_bytes(got).reshape(int(np.prod(lead)), -1)
    w = as_bytes(want).reshape(g.shape)
    m = np.asarray(mask).reshape(-1)
    bad = np.flatnonzero(m & (g != w).any(axis=1))
    assert bad.size == 0, f"{name}: cells {bad[:8]} hold {got.reshape(g.shape[0], -1)[bad[:4]][:, :4]}, " \
                          f"oracle {want.reshape(g.shape[0], -1)[bad[:4]][:, :4]}"
    if init is not None:
        i = as_bytes(np.asarray(init).reshape(want.shape)).reshape(g.shape)
        bad = np.flatnonzero(~m & (g != i).any(axis=1))
        assert bad.size == 0, f"{name}: cells {bad[:8]} were written but the oracle says not yet"


def check_exact(got: dict, want: dict, init: Optional[dict] = None, skip=()) -> int:
    """Every integer-valued or copied item of ``got`` (host arrays of the kernels' dtypes) against
    ``ActorRef.at``; cells the oracle says are not written must equal ``init``.  Returns the
    number of items compared."""
    init = init or {}
    count = 0
    for name in EXACT:
        if name in skip or name not in got or want.get(name) is None:
            continue
        w = np.asarray(want[name])
        if name in _ROW_MASK:
            mask = np.asarray(want[_ROW_MASK[name]])
        elif name in ("h32", "c", "h_bf"):
            mask = np.full(w.shape[:1], bool(want["carried_w"]))
        else:
            mask = np.ones(w.shape[:1] if w.ndim else (1,), bool)
        g = np.asarray(got[name])
        if name in ("t", "head", "ret_cnt", "n_valid"):
            assert int(g.reshape(-1)[0]) == int(w), f"{name}: {int(g.reshape(-1)[0])}, oracle {int(w)}"
        else:
            _rows_equal(name, g, w.astype(g.dtype) if w.dtype != g.dtype and w.dtype.kind in "iub"
                        else w, mask, init.get(name))
        count += 1
    return count


def check_reward(got, want: dict, spec: ActorSpec, init=None) -> float:
    """The reward column: finalised rows within c_R u sum |gamma^i r_i| (c_R = n + 5), every other
    row untouched.  Returns the largest use of the bound."""
    got = np.asarray(got, dtype=_f32).reshape(-1)
    fin = want["fin"]
    if init is not None:
        keep = as_bytes(got).reshape(-1, 4)[~fin] == as_bytes(np.asarray(init, _f32)).reshape(-1, 4)[~fin]
        assert keep.all(), "reward: rows written that are not finalised"
    g = got[fin].astype(np.float64)
    assert np.isfinite(g).all(), "reward: finalised rows not written"
    err = np.abs(g - want["reward"][fin])
    bound = (spec.n + 5) * U24 * want["reward_abs"][fin]
    bad = np.flatnonzero(err > bound)
    assert bad.size == 0, (f"reward rows {np.flatnonzero(fin)[bad[:6]]}: {g[bad[:6]]} vs "
                           f"{want['reward'][fin][bad[:6]]}, bound {bound[bad[:6]]}")
    pos = bound > 0
    return float((err[pos] / bound[pos]).max()) if pos.any() else 0.0


def priority_floor(want: dict, spec: ActorSpec) -> np.ndarray:
    """(cap) floor of the priority bound: 0 without value rescaling, else twice the error of the
    float32 evaluation of h(R + gamma_n h^-1(boot)) (h(R) on terminal rows) on the element's
    own inputs.  ``floor_error`` is that error itself."""
    return 2.0 * floor_error(want, spec)


def floor_error(want: dict, spec: ActorSpec) -> np.ndarray:
    if not spec.value_rescale:
        return np.zeros(want["reward"].shape)
    ve, gn = spec.f32("vr_eps"), spec.f32("gamma_n")
    R = want["reward"].astype(_f32)
    b = want["boot"].astype(_f32)
    arg = np.where(want["term"], R, R + _f32(gn) * h_inv32(b, ve)).astype(_f32)
    y32 = h32(arg, ve).astype(np.float64)
    y64 = td_ref.h(want["reward"] + np.where(want["term"], 0.0, gn * td_ref.h_inv(want["boot"], ve)), ve)
    return np.abs(y32 - y64)


def priority_bound(want: dict, spec: ActorSpec) -> np.ndarray:
    alpha, peps, gn = spec.f32("alpha"), spec.f32("prio_eps"), spec.f32("gamma_n")
    mag = np.abs(want["q_sel"]) + np.abs(want["reward"]) + gn * np.abs(want["bv"])
    return (4 * U24 * mag + (4 * U24 / alpha) * (np.abs(want["delta"]) + peps)
            + priority_floor(want, spec))


def check_priority(got, want: dict, spec: ActorSpec, init=None) -> dict:
    """The priority column in TD-error space (module docstring).  Returns the largest use of the
    bound and the largest share the floor has in the bound of a row."""
    got = np.asarray(got, dtype=_f32).reshape(-1)
    fin = want["fin"]
    if init is not None:
        keep = as_bytes(got).reshape(-1, 4)[~fin] == as_bytes(np.asarray(init, _f32)).reshape(-1, 4)[~fin]
        assert keep.all(), "priority: rows written that are not finalised"
    p = got[fin].astype(np.float64)
    assert np.isfinite(p).all() and (p > 0).all(), "priority: finalised rows not written or not positive"
    d = p ** (1.0 / spec.f32("alpha")) - spec.f32("prio_eps")
    err = np.abs(d - np.abs(want["delta"][fin]))
    bound = priority_bound(want, spec)[fin]
    bad = np.flatnonzero(err > bound)
    assert bad.size == 0, (f"priority rows {np.flatnonzero(fin)[bad[:6]]}: |delta| {d[bad[:6]]} vs "
                           f"{np.abs(want['delta'][fin][bad[:6]])}, use {(err / bound)[bad[:6]]}")
    floor = priority_floor(want, spec)[fin]
    return dict(use=float((err / bound).max()) if err.size else 0.0,
                floor_share=float((floor / bound).max()) if err.size else 0.0)


def check_leaves(leaves, flags, priority, want: dict, spec: ActorSpec) -> float:
    """Leaves of the starts the actor marked within replay_ref.leaf_bound(T) of seq_leaf of the
    kernel's own priorities; every other leaf as the oracle has it (0 once cleared, else what the
    replay began with).  Flags are compared by check_exact.  Returns the largest use of the bound."""
    leaves = np.asarray(leaves, dtype=_f32).reshape(-1)[: spec.cap]
    flags = np.asarray(flags).reshape(-1)[: spec.cap]
    eta = spec.f32("eta")
    off = ~(want["marked"] & (flags != 0))
    assert np.array_equal(leaves[off].astype(np.float64), want["leaves"][off]), "leaf of a row not marked"
    use = 0.0
    for s in np.flatnonzero(~off):
        w = rr.seq_leaf(priority, int(s), spec.T, spec.cap_e, eta)
        err = abs(float(leaves[s]) - w)
        assert err <= rr.leaf_bound(spec.T) * w, f"leaf {s}: {float(leaves[s])!r} vs {w!r}"
        use = max(use, err / (rr.leaf_bound(spec.T) * w))
    return use


def check_dirty(dirty, want: dict, cap: int, count=None):
    """The dirty list after a step: its first entries are the rows the step touched, in any
    order; ``count`` (read before the tail launch resets it) is the number of appends."""
    dirty = np.asarray(dirty).astype(np.int64).reshape(-1)
    k = int(want["dcount"])
    if count is not None:
        assert int(count) == k, f"dirty count {int(count)}, oracle {k}"
    assert sorted(dirty[:k].tolist()) == want["dirty_last"].tolist(), \
        f"dirty rows {sorted(dirty[:k].tolist())[:8]}, oracle {want['dirty_last'][:8]}"
    assert ((dirty >= -1) & (dirty < cap)).all(), "dirty list holds a row outside the replay"


def check_pending(pend, cnt, want_entries, pend_cap: int, poison: int = -1):
    """One pending list as a multiset (its order is not defined).  When more was appended than
    fits, the count still is the oracle's, the list holds pend_cap of the expected entries and
    nothing is written past it (``pend`` is the whole buffer behind the list's start)."""
    pend = np.asarray(pend).astype(np.int64).reshape(-1)
    want = sorted(int(v) for v in want_entries)
    assert int(cnt) == len(want), f"pending count {int(cnt)}, oracle {len(want)}"
    k = min(len(want), pend_cap)
    assert (pend[k:] == poison).all(), "pending list written past its count or its capacity"
    got = sorted(pend[:k].tolist())
    if len(want) <= pend_cap:
        assert got == want, f"pending entries {got[:8]}, oracle {want[:8]}"
    else:
        left = list(want)
        for v in got:
            assert v in left, f"pending entry {v} is not one the oracle expects (or too often)"
            left.remove(v)
