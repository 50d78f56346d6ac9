"""Float64 oracle of the TD / dueling-head kernel family (csrc/kernels/td.hip, head.hip).

Pure host code (numpy float64, no torch, no GPU).  Each function is the plain definition of one
operation the kernels fuse; the GPU tests (tests/test_td_head_gpu.py) compare every entry point
with it element by element, and tests/test_td_ref_cpu.py checks it against independent float64
PyTorch (``learner_ref.r2d2_loss``'s formulation, autograd through the dueling combine).

``mutation`` (tests only): a deliberately wrong variant of one rule, used once on the CPU to show
that the comparison functions below reject it -- a check that accepts a mutated oracle tests
nothing.  ``MUTATIONS`` lists them.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

MUTATIONS = ("terminal_ignored", "last_max", "is_max_first_wave", "relu_ge", "first_dup")

U24 = 2.0 ** -24     # fp32 unit roundoff (round to nearest)


class TdRef(NamedTuple):
    delta: np.ndarray      # (Tl, B) q(s_t, a_t) - y
    dq: np.ndarray         # (Tl, B, A) dL/dQ, nonzero at the taken action only
    loss: float            # mean(w * 0.5 * delta^2)
    is_w: np.ndarray       # (B) importance-sampling weights
    rows: np.ndarray       # (Tl, B) ring rows of the learning transitions (int64)
    best: np.ndarray       # (Tl, B) argmax_a q_arg (first maximum)
    act: np.ndarray        # (Tl, B) taken actions
    q_taken: np.ndarray    # (Tl, B) q_sa at the taken action
    boot: np.ndarray       # (Tl, B) q_tgt at best (before h^-1)
    reward: np.ndarray     # (Tl, B)
    done: np.ndarray       # (Tl, B) bool


def ring_rows(starts, Tl: int, burn_in: int, cap_e: int) -> np.ndarray:
    """(Tl, B) global rows of the learning transitions: ``ring_row`` of td.hip -- a window wraps
    inside the sub-ring that holds its start."""
    s = np.asarray(starts, dtype=np.int64)
    base = s - s % cap_e
    t = burn_in + np.arange(Tl, dtype=np.int64)
    return base[None, :] + (s[None, :] - base[None, :] + t[:, None]) % cap_e


def h(x, eps):
    """R2D2 value rescaling (models/qnet.py value_rescale)."""
    x = np.asarray(x, dtype=np.float64)
    return np.sign(x) * (np.sqrt(np.abs(x) + 1.0) - 1.0) + eps * x


def h_inv(x, eps):
    """Closed-form inverse of ``h`` (models/qnet.py value_rescale_inv)."""
    x = np.asarray(x, dtype=np.float64)
    s = (np.sqrt(1.0 + 4.0 * eps * (np.abs(x) + 1.0 + eps)) - 1.0) / (2.0 * eps)
    return np.sign(x) * (s * s - 1.0)


def is_weights(probs, B: int, beta: float, n_valid: int, dp=None,
               mutation: Optional[str] = None) -> np.ndarray:
    """td.hip ``is_weight``: (max(n_valid, 1) * p clamped at 1e-30)^-beta over the batch maximum;
    with ``dp`` = [f, ratio, N_global, gmax]: f * (N_global * p * ratio clamped)^-beta / gmax,
    already normalised across ranks (no division by the batch maximum)."""
    if dp is not None:
        f, ratio, n_glob, gmax = (float(v) for v in np.asarray(dp, dtype=np.float64))
        w = np.ones(B)
        if probs is not None and beta > 0:
            p = np.asarray(probs, dtype=np.float64)
            w = np.maximum(n_glob * p * ratio, 1e-30) ** (-beta)
        return f * w / gmax
    if probs is None or not beta > 0:
        return np.ones(B)
    p = np.asarray(probs, dtype=np.float64)
    w = np.maximum(max(int(n_valid), 1) * p, 1e-30) ** (-beta)
    wmax = w[:64].max() if mutation == "is_max_first_wave" else w.max()
    return w / wmax


def td_reference(q_sa, q_arg, q_tgt, starts, probs, action, reward, done, Tl, B, A, burn_in,
                 cap_e, gamma_n, value_rescale, vr_eps, alpha, prio_eps, beta, n_valid, dp=None,
                 mutation: Optional[str] = None) -> TdRef:
    """n-step double-Q TD error, loss, dL/dQ and IS weights of ``Tl x B`` transitions.  The Q
    arrays are (Tl, B, A) (or (Tl * B, A)); ``action`` / ``reward`` / ``done`` are the replay's
    per-row columns, read at the ring rows of the learning window.  ``alpha`` / ``prio_eps``
    belong to ``priority_reference``; they are accepted so that one argument list serves both."""
    del alpha, prio_eps
    f64 = lambda x: np.asarray(x, dtype=np.float64).reshape(Tl, B, A)   # noqa: E731
    q_sa, q_arg, q_tgt = f64(q_sa), f64(q_arg), f64(q_tgt)
    rows = ring_rows(starts, Tl, burn_in, cap_e)
    act = np.asarray(action)[rows].astype(np.int64)
    rew = np.asarray(reward, dtype=np.float64)[rows]
    dn = np.asarray(done)[rows] != 0
    if mutation == "last_max":
        best = A - 1 - np.argmax(q_arg[..., ::-1], axis=-1)
    else:
        best = np.argmax(q_arg, axis=-1)
    boot = np.take_along_axis(q_tgt, best[..., None], axis=-1)[..., 0]
    bv = h_inv(boot, vr_eps) if value_rescale else boot
    live = np.ones_like(dn) if mutation == "terminal_ignored" else ~dn
    y = rew + np.where(live, gamma_n * bv, 0.0)
    if value_rescale:
        y = h(y, vr_eps)
    q_taken = np.take_along_axis(q_sa, act[..., None], axis=-1)[..., 0]
    delta = q_taken - y
    w = is_weights(probs, B, beta, n_valid, dp, mutation)
    n = Tl * B
    loss = float((w[None, :] * 0.5 * delta * delta).sum() / n)
    dq = np.zeros((Tl, B, A))
    np.put_along_axis(dq, act[..., None], (w[None, :] * delta / n)[..., None], axis=-1)
    return TdRef(delta, dq, loss, w, rows, best, act, q_taken, boot, rew, dn)


def priority_reference(td_abs, rows, cap: int, alpha: float, prio_eps: float, fill: float,
                       mutation: Optional[str] = None) -> np.ndarray:
    """Row priorities (|delta| + eps)^alpha scattered to ``rows``; where two transitions share a
    row the LAST one in (t, b) row-major order wins (numpy's duplicate-index assignment, the
    reference's ``update_priority``).  Rows no transition maps to keep ``fill``."""
    out = np.full(cap, fill, dtype=np.float64)
    p = (np.asarray(td_abs, dtype=np.float64) + prio_eps) ** alpha
    order = zip(np.asarray(rows).reshape(-1).tolist(), p.reshape(-1).tolist())
    if mutation == "first_dup":
        order = reversed(list(order))
    for r, v in order:
        out[r] = v
    return out


def dueling_forward_reference(z, b1, w2, b2, A: int, HD: int):
    """Q = V + Adv - mean(Adv) of the dueling head after its first layer.  z: (N, 2 HD) pre-bias
    outputs [value half; advantage half]; w2: (1 + A, HD) rows [value; advantages]; returns
    (Q (N, A), relu(z + b1) (N, 2 HD))."""
    z = np.asarray(z, dtype=np.float64).reshape(-1, 2 * HD)
    w2 = np.asarray(w2, dtype=np.float64).reshape(1 + A, HD)
    b2 = np.asarray(b2, dtype=np.float64).reshape(1 + A)
    hr = np.maximum(z + np.asarray(b1, dtype=np.float64)[None, :], 0.0)
    v = hr[:, :HD] @ w2[0] + b2[0]
    adv = hr[:, HD:] @ w2[1:].T + b2[1:][None, :]
    return v[:, None] + adv - adv.mean(axis=1, keepdims=True), hr


def dueling_backward_reference(dq, zr, w2, A: int, HD: int, mutation: Optional[str] = None):
    """Backward of the dueling combine and the ReLU.  Returns (dva (N, 1 + A) = [dV, dAdv],
    dz (N, 2 HD) = relu'(zr) * (dva . w2)) with the mask ``zr > 0``."""
    dq = np.asarray(dq, dtype=np.float64).reshape(-1, A)
    zr = np.asarray(zr, dtype=np.float64).reshape(-1, 2 * HD)
    w2 = np.asarray(w2, dtype=np.float64).reshape(1 + A, HD)
    dv = dq.sum(axis=1)
    da = dq - dv[:, None] / A
    dz = np.concatenate([dv[:, None] * w2[0][None, :], da @ w2[1:]], axis=1)
    mask = zr >= 0 if mutation == "relu_ge" else zr > 0
    return np.concatenate([dv[:, None], da], axis=1), np.where(mask, dz, 0.0)


# ------------------------------------------------------------------ comparison with a kernel
# The bounds of a kernel that evaluates the same formulas in fp32.  Without value rescaling the
# target takes two roundings (gamma_n * boot, + r) and the subtraction one, so
#   |delta_kernel - delta_64| <= 4 u (|q| + |r| + gamma_n |boot|),  u = 2^-24
# (a terminal row has no bootstrap term at all).  With value rescaling the caller passes
# ``floor``: the closed-form h^-1 cancels in fp32, and the yardstick is fp32 PyTorch's own error
# on the same inputs (the tests measure it and pass twice that).

def delta_bound(ref: TdRef, gamma_n: float, floor=0.0, extra=0.0) -> np.ndarray:
    """(Tl, B) bound on |delta_kernel - delta_64|.  ``extra``: what the inputs' own error adds
    (a fused head forward hands the TD its fp32 Q rows, the oracle its float64 ones)."""
    boot = np.where(ref.done, 0.0, np.abs(ref.boot))
    b = 4.0 * U24 * (np.abs(ref.q_taken) + np.abs(ref.reward) + gamma_n * boot)
    return np.maximum(b, floor) + extra


def check_td(out: dict, ref: TdRef, gamma_n: float, floor=0.0, extra=0.0,
             is_w_rtol: float = 1e-5) -> dict:
    """Assert a TD launch's ``dq`` (Tl, B, A), ``td_abs`` (Tl, B), ``loss`` and ``is_w`` (B, or
    None) against the oracle, element by element.  Returns the measured maxima."""
    Tl, B, A = ref.dq.shape
    n = Tl * B
    dq = np.asarray(out["dq"], dtype=np.float64).reshape(Tl, B, A)
    td_abs = np.asarray(out["td_abs"], dtype=np.float64).reshape(Tl, B)
    bound = delta_bound(ref, gamma_n, floor, extra)
    w = ref.is_w[None, :]
    assert np.isfinite(dq).all() and np.isfinite(td_abs).all() and np.isfinite(out["loss"])
    taken = np.zeros((Tl, B, A), dtype=bool)
    np.put_along_axis(taken, ref.act[..., None], True, axis=-1)
    assert not dq[~taken].any(), "dq is nonzero off the taken action"
    # dq = w delta / n: delta within `bound`, w within is_w_rtol, two fp32 roundings
    got = np.take_along_axis(dq, ref.act[..., None], axis=-1)[..., 0]
    want = w * ref.delta / n
    tol_dq = w * bound / n + (is_w_rtol + 4 * U24) * np.abs(want)
    err_dq = np.abs(got - want)
    assert (err_dq <= tol_dq).all(), f"dq: worst {float((err_dq / tol_dq).max()):.3g} x bound"
    err_d = np.abs(td_abs - np.abs(ref.delta))
    assert (err_d <= bound).all(), f"td_abs: worst {float((err_d / bound).max()):.3g} x bound"
    if out.get("is_w") is not None:
        np.testing.assert_allclose(np.asarray(out["is_w"], dtype=np.float64), ref.is_w,
                                   rtol=is_w_rtol, atol=0)
    tol_l = float((w * np.abs(ref.delta) * bound).sum() / n) + 2.0 ** -21 * abs(ref.loss)
    err_l = abs(float(out["loss"]) - ref.loss)
    assert err_l <= tol_l, f"loss {float(out['loss'])!r} vs {ref.loss!r}: {err_l:.3g} > {tol_l:.3g}"
    return dict(delta_err=float(err_d.max()), loss_err=err_l)


def check_priority(priority, td_abs, ref: TdRef, cap: int, alpha: float, prio_eps: float,
                   fill: float = -1.0, mutation: Optional[str] = None) -> None:
    """A launch's whole priority buffer (tail rows past ``cap`` included) against the scatter of
    its OWN td_abs: owners, last-write-wins and untouched rows."""
    priority = np.asarray(priority, dtype=np.float64)
    want = priority_reference(td_abs, ref.rows, len(priority), alpha, prio_eps, fill, mutation)
    assert (want[cap:] == fill).all()
    np.testing.assert_allclose(priority, want, rtol=1e-6, atol=0)


def check_dueling_backward(out: dict, ref: TdRef, bound, zr, w2, HD: int, split: bool,
                           mutation: Optional[str] = None) -> None:
    """The fused dueling backward of a TD launch: ``dva`` (n, 1 + A) and ``dz`` (n, 2 HD; in
    split precision the hi + lo sum) against the backward of the oracle's dq.

    Every row's dq is g e_act, so dva and dz are g times a per-row coefficient: the TD bound on
    delta (``bound``) propagates as (w bound / n) |coefficient|.  On top of it dz is stored with
    one bf16 rounding (relative 2^-8 allowed), or as a hi / lo bf16 pair (split.h: 16 mantissa
    bits, relative 2^-16), and its A-term fp32 sum rounds (A + 3) times against the sum of the
    terms' magnitudes."""
    Tl, B, A = ref.dq.shape
    n = Tl * B
    w2 = np.asarray(w2, dtype=np.float64).reshape(1 + A, HD)
    zr = np.asarray(zr, dtype=np.float64).reshape(n, 2 * HD)
    act = ref.act.reshape(-1)
    g = np.take_along_axis(ref.dq.reshape(n, A), act[:, None], axis=1)[:, 0]
    tol_g = ((ref.is_w[None, :] * bound / n).reshape(-1) + (1e-5 + 4 * U24) * np.abs(g))
    unit = np.zeros((n, A))
    unit[np.arange(n), act] = 1.0
    cva, cz = dueling_backward_reference(unit, zr, w2, A, HD, mutation)
    # sum of |terms| of the advantage half: |(1 - 1/A) w_act| + sum_{k != act} |w_k| / A
    aw = np.abs(w2[1:])
    mag_a = aw[act] * (1.0 - 2.0 / A) + aw.sum(axis=0)[None, :] / A if A > 1 else aw[act] * 0.0
    mag = np.concatenate([np.tile(np.abs(w2[0]), (n, 1)), mag_a], axis=1)
    dva = np.asarray(out["dva"], dtype=np.float64).reshape(n, 1 + A)
    dz = np.asarray(out["dz"], dtype=np.float64).reshape(n, 2 * HD)
    assert np.isfinite(dva).all() and np.isfinite(dz).all()
    err = np.abs(dva - g[:, None] * cva)
    tol = tol_g[:, None] * np.abs(cva) + 4 * U24 * np.abs(g)[:, None]
    assert (err <= tol).all(), f"dva: worst {float((err / tol).max()):.3g} x bound"
    want = g[:, None] * cz
    rel = 2.0 ** -16 if split else 2.0 ** -8
    tol = rel * np.abs(want) + tol_g[:, None] * np.abs(cz) + (A + 3) * U24 * np.abs(g)[:, None] * mag
    err = np.abs(dz - want)
    assert (err <= tol).all(), f"dz: worst {float((err[err > tol] / tol[err > tol]).max()):.3g} x bound"


def q_bound(z, b1, w2, b2, A: int, HD: int) -> np.ndarray:
    """(N, A) bound on |Q_kernel - Q_64| for a dueling forward evaluated in fp32 from the same
    inputs: a dot product of HD terms summed HD / 64 per lane and then over a 6-level tree, the
    bias, and the combine V + Adv_a - mean(Adv) with the mean accumulated over A terms -- each
    rounding relative to the magnitudes summed so far."""
    z = np.asarray(z, dtype=np.float64).reshape(-1, 2 * HD)
    w2 = np.asarray(w2, dtype=np.float64).reshape(1 + A, HD)
    hr = np.maximum(z + np.asarray(b1, dtype=np.float64)[None, :], 0.0)
    b2 = np.abs(np.asarray(b2, dtype=np.float64))
    sv = hr[:, :HD] @ np.abs(w2[0]) + b2[0]
    sa = hr[:, HD:] @ np.abs(w2[1:]).T + b2[1:][None, :]
    depth = HD // 64 + 6 + 2 + 3          # products and sums of one dot, bias, combine
    return U24 * ((depth) * (sv[:, None] + sa) + (depth + A) * sa.mean(axis=1, keepdims=True))


def check_dueling_forward(q, zr, z, b1, w2, b2, A: int, HD: int, zr_bf16: bool) -> None:
    """A dueling forward's Q (N, A) and relu'd hidden (N, 2 HD, or None) against the oracle."""
    q_ref, hr = dueling_forward_reference(z, b1, w2, b2, A, HD)
    q = np.asarray(q, dtype=np.float64).reshape(-1, A)
    assert q.shape == q_ref.shape and np.isfinite(q).all()
    tol = q_bound(z, b1, w2, b2, A, HD)
    err = np.abs(q - q_ref)
    assert (err <= tol).all(), f"Q: worst {float((err / tol).max()):.3g} x bound"
    if zr is not None:
        zr = np.asarray(zr, dtype=np.float64).reshape(-1, 2 * HD)
        # one fp32 add, then (bf16 mode) one rounding to bf16's 8 significant bits
        rel = (2.0 ** -8 + 2 * U24) if zr_bf16 else U24
        assert (np.abs(zr - hr) <= rel * np.abs(hr)).all(), "zr"
        assert ((zr == 0) == (hr == 0)).all(), "zr: ReLU zeros"
