"""The float64 oracle of the batched actor's kernels (pytorch_r2d2_amd/actor_ref.py) against a
brute-force simulation (one object per env with a deque-based n-step memory and an episode
flush, written from the operation's definition: PARITY.md C11 NStepMemory, C12 calc_priority,
C13 sequence segmentation), an fp32 emulation of the kernels' arithmetic against every
``check_*``, and every entry of ``MUTATIONS`` against the checks.

Also holds the case table and its builders, which the GPU test (test_actor_oracle_gpu.py) shares.
"""
from collections import deque

import numpy as np
import pytest

from pytorch_r2d2_amd import actor_ref as ar
from pytorch_r2d2_amd import refnum as rn
from pytorch_r2d2_amd import replay_ref as rr
from pytorch_r2d2_amd import td_ref

f32 = np.float32
SEED = (0x9E3779B97F4A7C15 * 5 + 1) & ((1 << 64) - 1)


# ------------------------------------------------------------------ scripted logs
def _done_from_lengths(N, lens_per_env):
    done = np.zeros((N, len(lens_per_env)), bool)
    for e, lens in enumerate(lens_per_env):
        s, i = -1, 0
        while True:
            s += lens[i % len(lens)]
            i += 1
            if s >= N:
                break
            done[s, e] = True
    return done


def make_logs(spec, N, seed, done, rewards=(0.0, 1.0, -1.0, 0.5), q_scale=1.0, eps=None,
              q_int=False):
    g = np.random.default_rng(seed)
    E, A, H = spec.E, spec.A, spec.H
    q = lambda: (g.standard_normal((N, E, A)) * q_scale).astype(f32)   # noqa: E731
    q_on, q_tg = q(), q()
    if q_int:      # few distinct values: duplicated maxima in most rows
        q_on = g.integers(0, 3, (N, E, A)).astype(f32)
    reward = np.asarray(rewards, f32)[g.integers(0, len(rewards), (N, E))]
    finished = np.full((N, E), np.nan, f32)
    ret = np.zeros(E, f32)
    for s in range(N):
        ret = ret + reward[s]
        finished[s, done[s]] = ret[done[s]]
        ret[done[s]] = 0
    if eps is None:
        eps = [0.4 ** (1 + 7 * i / max(E - 1, 1)) for i in range(E)]
    return ar.ActorLogs(
        obs=g.integers(0, 256, (N, E, spec.FB), dtype=np.uint8), q_on=q_on, q_tg=q_tg,
        h_new=g.standard_normal((N, 2, E, H)).astype(f32), c_new=g.standard_normal((N, 2, E, H)).astype(f32),
        reward=reward, done=done, finished=finished, eps=np.asarray(eps, f32), seed=SEED + seed)


BASE = dict(E=3, A=4, H=8, n=3, T=5, stride=2, cap_e=24, FB=48, R=8)
# episode lengths 1, 1, 2 (< n), 3 (= n), 4 (< T), 5 (= T), 6, 7 (final start on the grid), 8 (off
# it), 30 (> cap_e); every env is done at step 66, envs 0 and 2 on the wrap step 72
BASE_LENS = ([1, 1, 2, 3, 4, 5, 6, 7, 8, 30, 6, 5, 9], [30, 8, 7, 6, 5, 4, 3, 2, 1, 1, 5, 7, 8],
             [4, 8, 2, 7, 1, 6, 3, 5, 1, 30, 6, 4, 11])


def _base_like(name, N=90, seed=1, lens=BASE_LENS, checks="every", log_kw=None, flags="zero", **over):
    spec = ar.ActorSpec(**{**BASE, **over})
    done = _done_from_lengths(N, lens)
    logs = make_logs(spec, N, seed, done, **(log_kw or {}))
    return dict(name=name, spec=spec, logs=logs, N=N, checks=checks, flags=flags)


def _exact_zero_delta(c):
    """Numerics cases: q and boot exactly 0 in places, and q_sel == fp32(y) on some rows of the
    env that always explores (its action does not depend on q_on, y does not depend on
    q_on[s])."""
    lg = c["logs"]
    q_on, q_tg = lg.q_on.copy(), lg.q_tg.copy()
    q_tg[5::7] = 0.0
    q_on[3::11, 0] = 0.0
    ref = ar.ActorRef(c["spec"], lg._replace(q_on=q_on, q_tg=q_tg))
    e = c["spec"].E - 1
    for s in range(2, c["N"], 5):
        if ref.known[s, e]:
            q_on[s, e, ref.act[s, e]] = f32(ref.y[s, e])
    c["logs"] = lg._replace(q_on=q_on, q_tg=q_tg)
    again = ar.ActorRef(c["spec"], c["logs"])
    assert np.array_equal(again.act[:, e], ref.act[:, e])
    return c


def build_cases():
    c = {}
    c["base"] = _base_like("base")
    g = np.random.default_rng(7)
    wide = ar.ActorSpec(E=70, A=64, H=300, n=1, T=3, stride=2, cap_e=9, FB=50, R=100)
    c["wide"] = dict(name="wide", spec=wide, N=30, checks="wraps", flags="zero",
                     logs=make_logs(wide, 30, 2, g.random((30, 70)) < 0.4))
    long_lens = ([1, 2, 3, 4, 5, 6, 7, 8, 9, 13], [13, 9, 8, 7, 6, 5, 4, 3, 2, 1], [3, 5, 8, 11, 6, 4, 7])
    for stride in (1, 3, 4):      # 1, = T, > T
        c[f"long_n_stride{stride}"] = _base_like(f"long_n_stride{stride}", N=60, seed=3 + stride,
                                                 lens=long_lens, checks="wraps", n=5, T=3, stride=stride)
    pal = (0.0, 1e-3, -1e-3, 1.0, -1.0, 1e3, -1e3)
    for vr in (0, 1):
        for gamma in (0.997, 1.0):
            name = f"numerics_vr{vr}_g{gamma}"
            c[name] = _exact_zero_delta(_base_like(
                name, seed=10 + 2 * vr + int(gamma == 1.0), checks="wraps", value_rescale=bool(vr),
                gamma=gamma, log_kw=dict(rewards=pal, q_scale=3.0, eps=[0.0, 0.3, 1.0])))
    c["argmax"] = _base_like("argmax", N=50, seed=20, checks="wraps", E=6,
                             lens=BASE_LENS + BASE_LENS,
                             log_kw=dict(q_int=True, eps=[0.0, 1.0, 0.5, 0.01, 1.0, 0.0]))
    c["stored_post"] = _base_like("stored_post", N=40, seed=21, checks="wraps", stored="post")
    for ahead in (1, 4):
        c[f"ahead{ahead}"] = _base_like(f"ahead{ahead}", seed=22 + ahead, checks="wraps", ahead=ahead,
                                        flags="all")
    c["deferred"] = _base_like("deferred", N=60, seed=30, checks="every", defer_D=6, pend_cap=4096,
                               round_len=4, cap_e=24, flags="all")
    c["deferred_overflow"] = _base_like("deferred_overflow", N=30, seed=31, checks="every", defer_D=6,
                                        pend_cap=2, round_len=1, flags="all")
    return c


CASES = build_cases()


def initial_flags(c):
    """(flags, leaves, n_valid) the replay starts with: empty, or every row a start."""
    cap = c["spec"].cap
    if c["flags"] == "all":
        return np.ones(cap, np.uint8), np.full(cap, 0.5), cap
    return np.zeros(cap, np.uint8), np.zeros(cap), 0


def oracle(c, mutation=None):
    fl, lv, nv = initial_flags(c)
    return ar.ActorRef(c["spec"], c["logs"], mutation, fl, lv, nv)


def check_steps(c):
    """After which numbers of steps a case is checked."""
    N, cap_e = c["N"], c["spec"].cap_e
    if c["checks"] == "every":
        return list(range(1, N + 1))
    return sorted({1, 2, N} | {s for s in range(1, N + 1) if s % cap_e in (0, 1)})


def poison_init(c):
    """What every buffer holds before the first launch: poison (NaN, -1, 0xAB) where the kernels
    only write, the required start values where they read first (flags, leaves, counters, the
    carried state, h_step / h_valid)."""
    sp = c["spec"]
    fl, lv, nv = initial_flags(c)
    nan = lambda *s: np.full(s, np.nan, f32)          # noqa: E731
    m1 = lambda *s, dt=np.int64: np.full(s, -1, dt)   # noqa: E731
    ab = lambda *s: np.full(s, 0xAB, np.uint8)        # noqa: E731
    cap, n, E, H = sp.cap, sp.n, sp.E, sp.H
    return dict(frames=ab(cap, sp.FB), hs_cs=nan(cap, 2 * H), ths_cs=nan(cap, 2 * H), action=ab(cap),
                reward=nan(cap), done=ab(cap), priority=nan(cap), is_start=fl, leaves=lv.astype(f32),
                n_valid=np.asarray([nv], np.int32), h_row=m1(n, E), h_q=nan(n, E, sp.A), h_a=m1(n, E),
                h_r=nan(n, E), h_step=m1(n, E), h_valid=np.zeros((n, E), np.uint8),
                ep_start=np.zeros(E, np.int64), t=np.zeros(1, np.int64), head=np.zeros(1, np.int64),
                act=m1(E), marks=m1(n + 2, E, dt=np.int32), ret_ring=nan(sp.R),
                ret_env=m1(sp.R, dt=np.int32), ret_cnt=np.zeros(1, np.int64),
                h32=np.zeros((2, E, H), f32), c=np.zeros((2, E, H), f32),
                h_bf=np.full((2, E, H), 0x7FC0, np.uint16))


def as_kernel(st, init, spec):
    """An oracle state as the kernels would have left it: fp32 columns, ``init`` where nothing
    was written."""
    out = {}
    for name in ar.EXACT:
        w = st.get(name)
        if w is None:
            out[name] = init[name].copy()
            continue
        w = np.asarray(w)
        if name in ar._ROW_MASK:
            m = np.asarray(st[ar._ROW_MASK[name]])
            a = init[name].copy()
            a[m] = w.astype(a.dtype)[m]
            out[name] = a
        elif name in ("h32", "c", "h_bf") and not st["carried_w"]:
            out[name] = init[name].copy()
        else:
            out[name] = w.astype(init[name].dtype).reshape(init[name].shape)
    for name in ("reward", "priority"):
        a = init[name].copy()
        a[st["fin"]] = st[name][st["fin"]].astype(f32)
        out[name] = a
    out["leaves"] = st["leaves"].astype(f32)
    dirty = np.full(64 + spec.cap, -1, np.int32)
    dirty[: len(st["dirty_last"])] = st["dirty_last"][::-1]
    out["dirty"], out["dcount"] = dirty, st["dcount"]
    out["pend"] = [np.asarray(p[::-1], np.int32) for p in st["pend"]]
    return out


def check_all(got, want, init, spec):
    """Every check of the oracle on one state; returns the measured uses."""
    ar.check_exact(got, want, init)
    rep = dict(reward=ar.check_reward(got["reward"], want, spec, init["reward"]))
    rep.update(ar.check_priority(got["priority"], want, spec, init["priority"]))
    if spec.defer_D > 0:
        for k in range(2):
            buf = np.full(len(want["pend"][k]) + 8, -1, np.int64)
            buf[: min(len(got["pend"][k]), spec.pend_cap)] = got["pend"][k][: spec.pend_cap]
            ar.check_pending(buf, len(got["pend"][k]), want["pend"][k], spec.pend_cap)
        assert np.array_equal(got["leaves"], init["leaves"])
    else:
        rep["leaf"] = ar.check_leaves(got["leaves"], got["is_start"], got["priority"], want, spec)
        ar.check_dirty(got["dirty"], want, spec.cap, got["dcount"])
    return rep


# ------------------------------------------------------------------ brute force
class EnvSim:
    """One env, from the definitions: a deque of the last n steps that are not finalised; a step
    leaves it when n successors exist (bootstrapped target) or the episode ends (truncated)."""

    def __init__(self, e, spec, replay):
        self.e, self.sp, self.rp = e, spec, replay
        self.mem = deque()
        self.ep0, self.finalised, self.marked = 0, -1, set()
        self.carry = None

    def _finalise(self, item, rewards, boot, sp):
        g, gn = sp.f32("gamma"), sp.f32("gamma_n")
        R = sum(g ** i * float(r) for i, r in enumerate(rewards))
        hinv = (lambda x: float(td_ref.h_inv(x, sp.f32("vr_eps")))) if sp.value_rescale else float
        hh = (lambda x: float(td_ref.h(x, sp.f32("vr_eps")))) if sp.value_rescale else float
        y = hh(R) if boot is None else hh(R + gn * hinv(boot))
        row = item["row"]
        self.rp["reward"][row], self.rp["done"][row] = R, int(boot is None)
        self.rp["priority"][row] = (abs(item["q"] - y) + sp.f32("prio_eps")) ** sp.f32("alpha")
        self.rp["fin"][row] = True
        self.finalised = item["step"]

    def pre(self, t, q_on, q_tg):
        if len(self.mem) == self.sp.n:
            item = self.mem.popleft()
            rewards = [item["r"]] + [m["r"] for m in self.mem]
            self._finalise(item, rewards, float(q_tg[int(np.argmax(q_on))]), self.sp)

    def post(self, t, row, q_sel, r, done):
        """Returns the starts (first step, slot) that became complete."""
        sp = self.sp
        self.mem.append(dict(step=t, row=row, q=float(q_sel), r=r))
        out = []
        o = self.finalised - self.ep0 - sp.T + 1
        if self.finalised >= self.ep0 and o >= 0 and o % sp.stride == 0 and o not in self.marked:
            out.append((self.ep0 + o, 0))
            self.marked.add(o)
        if done:
            while self.mem:
                item = self.mem.popleft()
                self._finalise(item, [item["r"]] + [m["r"] for m in self.mem], None, sp)
            L = t - self.ep0 + 1
            for o in range(0, L - sp.T + 1):
                if (o % sp.stride == 0 or o == L - sp.T) and o not in self.marked:
                    out.append((self.ep0 + o, 1 + L - sp.T - o))
            self.ep0, self.marked, self.finalised = t + 1, set(), -1
        return out


def brute_force(c, S):
    sp, lg = c["spec"], c["logs"]
    fl, lv, nv = initial_flags(c)
    cap, cap_e, E, H = sp.cap, sp.cap_e, sp.E, sp.H
    rp = dict(reward=np.zeros(cap), done=np.zeros(cap, np.uint8), priority=np.zeros(cap),
              fin=np.zeros(cap, bool), is_start=fl.copy(), leaves=lv.copy(), n_valid=nv,
              frames=np.zeros((cap, sp.FB), np.uint8), action=np.zeros(cap, np.uint8),
              hs_cs=np.zeros((cap, 2 * H), f32), ths_cs=np.zeros((cap, 2 * H), f32),
              row_w=np.zeros(cap, bool))
    envs = [EnvSim(e, sp, rp) for e in range(E)]
    if sp.ahead > 0 and sp.ctor_clears:      # BatchedActor starts in the invariant
        for g in (e * cap_e + r for e in range(E) for r in range(sp.ahead)):
            rp["n_valid"] -= int(rp["is_start"][g] != 0)
            rp["is_start"][g], rp["leaves"][g] = 0, 0.0
    carry_h, carry_c = np.zeros((2, E, H), f32), np.zeros((2, E, H), f32)
    rets, pend = [], {}
    dirty, marks, act = set(), None, None
    for t in range(S):
        head = t % cap_e
        dirty, marks = set(), np.full((sp.n + 2, E), -1, np.int32)
        entries = pend.setdefault(t // sp.round_len, [])

        def clear(g):
            if rp["is_start"][g] or rp["leaves"][g] != 0:
                rp["n_valid"] -= int(rp["is_start"][g] != 0)
                rp["is_start"][g], rp["leaves"][g] = 0, 0.0
                dirty.add(g)

        greedy, act = ar.choose_actions(lg.q_on[t], lg.eps, lg.seed, t)
        new = []
        for e, env in enumerate(envs):
            base = e * cap_e
            if sp.defer_D > 0:
                entries.append(-2 - (base + (head + sp.defer_D) % cap_e))
            elif sp.ahead > 0:
                clear(base + (head + sp.ahead) % cap_e)
            else:
                clear(base + head)
                if head == 0:
                    for r in range(cap_e - sp.W + 1, cap_e):
                        clear(base + r)
            row = base + head
            rp["frames"][row], rp["action"][row], rp["row_w"][row] = lg.obs[t, e], act[e], True
            h, c_ = (lg.h_new[t], lg.c_new[t]) if sp.stored == "post" else (carry_h, carry_c)
            for k, name in enumerate(("hs_cs", "ths_cs")):
                rp[name][row] = np.concatenate([h[k, e], c_[k, e]])
            env.pre(t, lg.q_on[t, e], lg.q_tg[t, e])
        for e, env in enumerate(envs):
            row = e * cap_e + head
            for first, slot in env.post(t, row, lg.q_on[t, e, act[e]], lg.reward[t, e], lg.done[t, e]):
                new.append((e, first, slot))
            if lg.done[t, e]:
                rets.append((lg.finished[t, e], e))
        carry_h = np.where(lg.done[t][None, :, None], f32(0), lg.h_new[t])
        carry_c = np.where(lg.done[t][None, :, None], f32(0), lg.c_new[t])
        for e, first, slot in new:
            g = e * cap_e + first % cap_e
            if sp.defer_D > 0:
                entries.append(g)
                continue
            marks[slot, e] = g
            rp["n_valid"] += int(rp["is_start"][g] == 0)
            win = e * cap_e + (first + np.arange(sp.T)) % cap_e
            p = rp["priority"][win]
            rp["is_start"][g] = 1
            rp["leaves"][g] = sp.f32("eta") * p.max() + (1 - sp.f32("eta")) * p.mean()
            dirty.add(g)
    rp.update(dirty_last=np.asarray(sorted(dirty), np.int64), marks=marks, act=act, rets=rets,
              h32=carry_h, c=carry_c, ep_start=np.asarray([env.ep0 for env in envs]),
              pend=pend)
    return rp


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_equals_brute_force(name):
    c = CASES[name]
    sp = c["spec"]
    ref = oracle(c)
    steps = check_steps(c)
    for S in (steps if len(steps) < 12 else steps[:: max(1, len(steps) // 8)] + [c["N"]]):
        o, b = ref.at(S), brute_force(c, S)
        for k in ("frames", "action", "hs_cs", "ths_cs", "row_w", "fin", "is_start", "dirty_last",
                  "h32", "c", "ep_start"):
            assert np.array_equal(o[k], b[k]), (name, S, k)
        assert np.array_equal(o["done"][o["fin"]], b["done"][b["fin"]]), (name, S)
        for k in ("reward", "priority", "leaves"):
            m = o["fin"] if k != "leaves" else np.ones(sp.cap, bool)
            np.testing.assert_allclose(o[k][m], b[k][m], rtol=1e-12, atol=0, err_msg=f"{name} {S} {k}")
        assert o["n_valid"] == b["n_valid"], (name, S)
        assert np.array_equal(o["act"], b["act"])
        if sp.defer_D > 0:
            cur = (S - 1) // sp.round_len
            for rnd in (cur - 1, cur):
                if rnd >= 0:
                    assert o["pend"][rnd % 2] == sorted(b["pend"][rnd]), (name, S, rnd)
        else:
            assert np.array_equal(o["marks"], b["marks"]), (name, S)
        assert o["ret_cnt"] == len(b["rets"])
        for i in range(max(0, o["ret_cnt"] - sp.R), o["ret_cnt"]):
            assert o["ret_ring"][i % sp.R] == b["rets"][i][0] and o["ret_env"][i % sp.R] == b["rets"][i][1]


def test_constructor_clears_of_clear_ahead():
    """BatchedActor clears rows 0 .. ahead - 1 of a pre-filled replay before its first step; the
    launches alone reach them only when the ahead pointer comes round."""
    c = dict(CASES["ahead4"])
    plain = oracle(c).at(1)
    c["spec"] = c["spec"]._replace(ctor_clears=True)
    ref = oracle(c)
    cap_e = c["spec"].cap_e
    assert plain["is_start"][:4].all() and not ref.at(1)["is_start"][:4].any()
    for S in (1, cap_e - 4, cap_e, c["N"]):
        o, b = ref.at(S), brute_force(c, S)
        assert np.array_equal(o["is_start"], b["is_start"]) and o["n_valid"] == b["n_valid"], S
        np.testing.assert_allclose(o["leaves"], b["leaves"], rtol=1e-12, atol=0)


def test_the_base_case_holds_what_it_is_for():
    c = CASES["base"]
    done, cap_e = c["logs"].done, c["spec"].cap_e
    assert done.all(axis=1).any(), "no step with every env done"
    assert done[cap_e::cap_e].any(), "no done on a wrap step"
    assert c["N"] // cap_e == 3
    ref = oracle(c)
    lens = {end - ep0 + 1 for eps in ref.episodes for ep0, end in eps if end < c["N"]}
    assert {1, 2, 3, 4, 5, 6, 7, 8, 30} <= lens
    w = CASES["wide"]
    assert (w["logs"].done.sum(axis=1) > 20).any() and w["logs"].done[:, 64:].any()
    assert oracle(w).at(w["N"])["ret_cnt"] > w["spec"].R
    a = oracle(CASES["argmax"])
    q = CASES["argmax"]["logs"].q_on
    assert ((q == q.max(axis=2, keepdims=True)).sum(axis=2) > 1).mean() > 0.3
    assert (a.act != a.greedy).any() and (a.act[:, 0] == a.greedy[:, 0]).all()


# ------------------------------------------------------------------ fp32 emulation of the kernels
def emulate(c, ref, S):
    """The state after S steps with reward, priority and leaves computed as the kernels do: the
    return summed in double over the history slots in slot order (step % n) and rounded once,
    everything else in fp32."""
    sp, lg = c["spec"], c["logs"]
    st = ref.at(S)
    got = as_kernel(st, poison_init(c), sp)
    g, gn, ve = f32(sp.gamma), f32(sp.gamma ** sp.n), f32(sp.vr_eps)
    for row in np.flatnonzero(st["fin"]):
        e, s = row // sp.cap_e, int(st["step"][row])
        m = int(min(sp.n, ref.end[s, e] - s + 1))
        R = 0.0
        for step in sorted(range(s, s + m), key=lambda x: x % sp.n):
            R += float(lg.reward[step, e]) * float(g) ** (step - s)
        R = f32(R)
        if st["term"][row]:
            y = ar.h32(R, ve) if sp.value_rescale else R
        else:
            b = f32(st["boot"][row])
            y = ar.h32(f32(R + gn * ar.h_inv32(b, ve)), ve) if sp.value_rescale else f32(R + gn * b)
        q = f32(st["q_sel"][row])
        got["reward"][row] = R
        got["priority"][row] = np.power(f32(np.abs(f32(q - y)) + f32(sp.prio_eps)), f32(sp.alpha))
    eta = f32(sp.eta)
    for s in np.flatnonzero(st["marked"]):
        p = got["priority"][rr.ring_row(int(s), np.arange(sp.T), sp.cap_e)]
        got["leaves"][s] = f32(eta * p.max() + f32(f32(1) - eta) * f32(p.sum(dtype=f32) / f32(sp.T)))
    return st, got


@pytest.mark.parametrize("name", list(CASES))
def test_fp32_emulation_passes_every_check(name):
    c = CASES[name]
    sp = c["spec"]
    ref = oracle(c)
    init = poison_init(c)
    worst = {}
    for S in check_steps(c)[-3:] + check_steps(c)[:4]:
        want, got = emulate(c, ref, S)
        for k, v in check_all(got, want, init, sp).items():
            worst[k] = max(worst.get(k, 0.0), v)
        # the reference alone: the float32 evaluation of the target stays inside the bound
        fin = want["fin"]
        err = ar.floor_error(want, sp)[fin] + 2 * ar.U24 * (np.abs(want["q_sel"]) + np.abs(want["delta"]))[fin]
        assert (err <= ar.priority_bound(want, sp)[fin]).all()
    assert worst["reward"] < 1.0 and worst["use"] < 1.0


# ------------------------------------------------------------------ mutations
SHOWN_ON = dict(boot_argmax_tg="base", terminal_bootstraps="base", gamma_n_minus_1="base",
                done_last_row_only="base", no_final_start="base", final_start_on_grid="base",
                start_one_step_early="base", last_max="argmax", random_reuses_first_uniform="argmax",
                stored_post="base", no_state_reset="base", ret_reverse_env_order="base")


def test_every_mutation_is_named():
    assert set(SHOWN_ON) == set(ar.MUTATIONS)


@pytest.mark.parametrize("mutation", ar.MUTATIONS)
def test_checks_reject_a_mutated_oracle(mutation):
    c = CASES[SHOWN_ON[mutation]]
    sp = c["spec"]
    ref, bad = oracle(c), oracle(c, mutation)
    init = poison_init(c)
    rejected = 0
    for S in check_steps(c):
        got = as_kernel(bad.at(S), init, sp)
        try:
            check_all(got, ref.at(S), init, sp)
        except AssertionError:
            rejected += 1
    assert rejected > 0, f"{mutation} passes every check on {c['name']}"
    # and the unmutated oracle passes them
    got = as_kernel(ref.at(c["N"]), init, sp)
    check_all(got, ref.at(c["N"]), init, sp)


def test_bf16_rounding_and_uniform_draws():
    x = np.asarray([1.0, 1.00390625, 1.01171875, -3.1415927, 1e-20, 0.0], f32)
    # 1 + 2^-8 ties to even (down), 1 + 3 * 2^-8 ties to even (up)
    assert rn.bf16_bits(x)[:3].tolist() == [0x3F80, 0x3F80, 0x3F82]
    import torch
    t = torch.from_numpy(np.random.default_rng(0).standard_normal(4096).astype(f32))
    assert np.array_equal(rn.bf16_bits(t.numpy()), t.bfloat16().view(torch.int16).numpy().view(np.uint16))
