"""Float64 oracle of the LSTM recurrence kernels (csrc/kernels/lstm.hip, lstm_persist.hip,
lstm_bptt.hip).

Pure host code (numpy, no torch, no GPU).  The oracle is *teacher forced*: it does not run a
trajectory of its own.  For every step it recomputes that step in float64 from the operands the
kernel itself left in memory (the stored ``h_seq[t-1]`` / ``c_seq[t-1]`` in the forward, the stored
``dgates[t+1]`` in the backward), so every check is a one-step check with a bound that can be derived
per element, and by induction from the first step the whole trajectory is covered.  A stale or
misdelivered hand-off word shows up as a next step that is inconsistent with what was stored.

Contents: the packed layouts (built here by plain indexing, independent of optim.hip's pack
kernel), the step references, the per-element bounds (each derivation in the docstring of the
function that computes it), the ``check_*`` comparison functions, an fp32 emulation of the kernels
(``emulate_*``: the condition that the bounds are not too tight, checked on the CPU), and the case
lists that tests/test_lstm_ref_cpu.py and tests/test_lstm_oracle_gpu.py share.

``mutation`` (tests only): a deliberately wrong variant of one rule of the oracle, used on the CPU
to show that the checks reject it -- a check that accepts a mutated oracle tests nothing.
"""
from __future__ import annotations

import zlib
from typing import Optional

import numpy as np

# bf16_val and the ownership checks are not used below: they stay part of this oracle's interface
# (a caller that holds the oracle holds the checks of the buffers it describes)
from .refnum import (bf16_bits, bf16_round, bf16_val, bits_equal, check_ownership,  # noqa: F401
                     check_untouched, compare, compare_bf16, split_planes)

U = 2.0 ** -24              # fp32 unit roundoff (round to nearest)
UNITS, GCOLS = 16, 64       # hidden units / packed gate columns per workgroup (lstm.hip)
DZ_K = 512                  # dz row length of the in-BPTT dh_ext path (lstm_bptt.hip PT_DZ_K)

# ---- activation error (csrc/common.h sigmoidf_ / tanhf_), absolute, in units of 2^-23.
#
# sigmoidf_(x) = rcp(1 + __expf(-x)); __expf(y) = v_exp_f32(y * log2(e)).  With s the exact value and
# e = exp(-x):  ds/de = -1/(1+e)^2, so a relative error r of e moves s by r * e/(1+e)^2 = r s(1-s).
#   v_exp_f32, 1 ulp (relative 2^-23):                          s(1-s) 2^-23      <= 0.25
#   rounding of the product y*log2(e) (relative 2^-24 of the exponent z, i.e. a relative error
#     ln2 |z| 2^-24 = |x| 2^-24 of e):                          |x| s(1-s) 2^-24  <= 0.112
#     (max of x s(1-s) is 0.2239 at x = 1.5434)
#   log2(e) held in fp32 (relative 2^-24): the same again       <= 0.112
#   fp32 rounding of 1 + e (relative 2^-24 of the sum):         s 2^-24           <= 0.5
#   v_rcp_f32, 1 ulp of a result in (0, 1]:                     s 2^-23           <= 1.0
# total <= 1.98 * 2^-23.
# tanhf_(x) = copysign((1 - e) * rcp(1 + e), x), e = __expf(-2|x|); dt/de = -2/(1+e)^2 and
# 2e/(1+e)^2 = (1 - t^2)/2:
#   v_exp_f32 1 ulp:                                            (1-t^2)/2 2^-23   <= 0.5
#   the two roundings of the exponent (2|x| 2^-24 each):        |x|(1-t^2) 2^-23  <= 0.448
#     (max of x (1 - tanh^2 x) is 0.4477 at x = 0.7717)
#   roundings of 1 - e, 1 + e and of the product (2^-24 |t| each)                 <= 1.5
#   v_rcp_f32 1 ulp:                                            |t| 2^-23         <= 1.0
# total <= 3.45 * 2^-23.  A single eps_act = 2^-21 would cover both; the smaller constants are used.  Saturation: for x > 87 e underflows to 0 (s = 1, t = 1 exactly); for x < -88.7 e is
# +inf and rcp(inf) = 0; the exact values are within 2^-126 of those.
EPS_SIG = 2.0 * 2.0 ** -23
EPS_TANH = 3.5 * 2.0 ** -23

MUTATIONS_FWD = ("swap_if", "c_in_t", "slices_swapped", "save_from_off", "gates_preact",
                 "g_sigmoid", "stale_h")
MUTATIONS_BWD = ("drop_dc", "tanh_prev", "fgrad_ct", "cprev_c0", "dh_ext_next", "no_rec_step",
                 "no_rec_wg", "dz_first_omitted")
MUTATIONS_BIAS = ("bias_tail_row", "bias_no_last_tile", "perm_inverse")


# ------------------------------------------------------------------------------------------
# the hand-off word (bf16 and the split planes: refnum.py)

def round19(x) -> np.ndarray:
    """The 4-byte tagged hand-off word without its tag: fp32 rounded to 19 explicit mantissa bits,
    ``(bits + 8) & ~15`` (lstm_persist.hip / lstm_bptt.hip T4)."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((b + np.uint32(8)) & ~np.uint32(15)).view(np.float32)


# ------------------------------------------------------------------------------------------
# packed layouts (header of lstm.hip)

def gate_cols(H: int) -> np.ndarray:
    """(4, H): packed column of gate g (i, f, g, o) of hidden unit n: (n // 16) * 64 + g * 16 + n % 16."""
    n = np.arange(H)
    return np.stack([(n // UNITS) * GCOLS + g * UNITS + n % UNITS for g in range(4)])


def gate_perm(H: int) -> np.ndarray:
    """perm[p] = PyTorch gate row (g * H + n) held by packed column p."""
    perm = np.empty(4 * H, dtype=np.int64)
    cols = gate_cols(H)
    for g in range(4):
        perm[cols[g]] = g * H + np.arange(H)
    return perm


def pack_whh(w) -> np.ndarray:
    """(4H, H) PyTorch-order W_hh -> packed (NWG, 64, H)."""
    H = w.shape[1]
    return np.ascontiguousarray(w[gate_perm(H)].reshape(H // UNITS, GCOLS, H))


def pack_whh_t(wpk) -> np.ndarray:
    """packed (NWG, 64, H) (or (4H, H)) -> transposed (NWG, H, 64): whhT[j][n][k] = W_pk[j][k][n]."""
    H = wpk.shape[-1]
    return np.ascontiguousarray(wpk.reshape(H // UNITS, GCOLS, H).transpose(0, 2, 1))


def unpack_cols(a) -> np.ndarray:
    """(..., 4H) packed gate columns -> PyTorch gate order."""
    H = a.shape[-1] // 4
    out = np.empty_like(a)
    out[..., gate_perm(H)] = a
    return out


# ------------------------------------------------------------------------------------------
# step references

def _sig(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x))


def forward_step(x, h_in, c_in, w, c_forget=None, mutation: Optional[str] = None):
    """One LSTM step in float64 on packed columns.  x (.., B, 4H) packed pre-activations incl.
    biases, h_in / c_in (.., B, H), w (4H, H) packed rows.  Returns (a, gates, c, h): packed
    pre-activations, packed post-activation gates (i, f, g, o blocks), cell, output."""
    H = h_in.shape[-1]
    col = gate_cols(H)
    a = x + h_in @ w.T
    gi, gf, gg, go = _sig(a[..., col[0]]), _sig(a[..., col[1]]), np.tanh(a[..., col[2]]), _sig(a[..., col[3]])
    if mutation == "swap_if":
        gi, gf = gf, gi
    if mutation == "g_sigmoid":
        gg = _sig(a[..., col[2]])
    c = gf * (c_in if c_forget is None else c_forget) + gi * gg
    h = go * np.tanh(c)
    gates = np.empty_like(a)
    gates[..., col[0]], gates[..., col[1]], gates[..., col[2]], gates[..., col[3]] = gi, gf, gg, go
    if mutation == "gates_preact":
        gates = a.copy()
    return a, gates, c, h


def free_forward(xproj, w, h0, c0):
    """The untied oracle: the step reference fed its own outputs, no rounding anywhere.
    Returns (gates (T, B, 4H) packed, c (T, B, H), h (T, B, H))."""
    h, c = np.asarray(h0, np.float64), np.asarray(c0, np.float64)
    gs, cs, hs = [], [], []
    for t in range(xproj.shape[0]):
        _, g, c, h = forward_step(np.asarray(xproj[t], np.float64), h, c, w)
        gs.append(g), cs.append(c), hs.append(h)
    return np.stack(gs), np.stack(cs), np.stack(hs)


def backward_step(dh, dc, gates, c_t, c_prev, mutation: Optional[str] = None, c_tanh=None):
    """Pointwise BPTT step in float64 (the kernels' formulas): returns (dgates packed, dc carry,
    dc_tot, tc).  gates packed post-activation (.., B, 4H)."""
    H = dh.shape[-1]
    col = gate_cols(H)
    gi, gf, gg, go = (gates[..., col[q]] for q in range(4))
    tc = np.tanh(c_t if c_tanh is None else c_tanh)
    dc_tot = dc + dh * go * (1.0 - tc * tc)
    d_o = dh * np.tanh(c_t)
    dg = np.empty_like(gates)
    dg[..., col[0]] = dc_tot * gg * gi * (1.0 - gi)
    dg[..., col[1]] = dc_tot * (c_t if mutation == "fgrad_ct" else c_prev) * gf * (1.0 - gf)
    dg[..., col[2]] = dc_tot * gi * (1.0 - gg * gg)
    dg[..., col[3]] = d_o * go * (1.0 - go)
    return dg, dc_tot * gf, dc_tot, tc


def free_backward(dh_ext, gates, c_seq, c0, w, t0):
    """The untied backward: the step reference fed its own gate gradients, no rounding.
    gates (T - t0, B, 4H), c_seq (T, B, H).  Returns dgates (T - t0, B, 4H) packed."""
    T = c_seq.shape[0]
    dc = np.zeros_like(c_seq[0])
    out = [None] * (T - t0)
    for t in range(T - 1, t0 - 1, -1):
        tl = t - t0
        dh = dh_ext[tl] + (out[tl + 1] @ w if t < T - 1 else 0.0)
        out[tl], dc, _, _ = backward_step(dh, dc, gates[tl], c_seq[t], c_seq[t - 1] if t > 0 else c0)
    return np.stack(out)


# ------------------------------------------------------------------------------------------
# forward: reference, bounds, check

def forward_operands(ch, sp: bool):
    """The operands a forward entry point reads for chain ``ch`` (a dict of fp32 arrays: w (4H, H)
    packed rows, h0, c0, xproj): bf16 kernels take bf16(w) and bf16(h0); split precision takes w as
    hi / lo planes and h0 in fp32.  Returns dict(w_hi, w_lo, w64, h0)."""
    if sp:
        hi, lo = split_planes(ch["w"])
        return dict(w_hi=hi, w_lo=lo, w64=hi.astype(np.float64) + lo, h0=ch["h0"].astype(np.float32))
    hi = bf16_round(ch["w"])
    return dict(w_hi=hi, w_lo=None, w64=hi.astype(np.float64), h0=bf16_round(ch["h0"]))


def forward_reference(ch, ops, out, sp: bool, mutation: Optional[str] = None):
    """Teacher-forced float64 forward of every step of one chain, with per-element bounds.

    h_in(t) = h0 (t = 0) else the stored h_seq[t-1] (+ h_seq_lo[t-1] in split precision);
    c_in(t) = c0 else the stored c_seq[t-1].  Returns dict(gates, c, h, e_gates, e_c, e_h,
    c_in, h_in), every entry (T, B, .).

    Bounds (S = sum_k |h_in||W|, all per element):
      pre-activation  da = (n + 2) u (S + |x|) + r S.  bf16 kernels: n = H products, exact in fp32
        (bf16 x bf16), summed in fp32 in any order, plus the add of x; r = 0 because the kernel
        multiplies exactly the stored bf16 images.  Split precision: n = 3H (three passes), and r
        collects what separates the kernel's operand from ``h_seq + h_seq_lo``.  For x in
        [2^e, 2^(e+1)) bf16 (8 significant bits) leaves |x - hi| <= 2^(e-8) <= 2^-8 |x|, exactly
        representable; lo rounds that remainder (below 2^(e-8), so half an ulp is 2^(e-17)): hi + lo
        represents x to 2^-17 |x|, once for the stored planes and once for the planes the consumer
        makes from the hand-off word; the dropped lo.lo term is <= 2^-8 2^-8 |a||b|; for t > 0 the
        19-bit hand-off word (20 significant bits) adds 2^-20.  r = 2 * 2^-17 + 2^-16 + 2^-20 (t > 0),
        2^-17 + 2^-16 (t = 0: h0 is fp32 and is split once), times (1 + 2^-15) for |kernel operand|
        against |stored|.
      gates  e_q = eps_act + L_q da, L = 1/4 (sigmoid), 1 (tanh).
      cell   c = f c_in + i g, c_in exact (the kernel's register equals what it stored):
        e_c = e_f |c_in| + e_i |g| + e_g |i| + e_i e_g + 3u (|f c_in| + |i g|)   (two products, one sum)
      output h = o tanh(c):  e_h = e_o |tanh c| + (o + e_o)(eps_tanh + e_c) + 2u |h|.
    """
    T, B, H = out["c_seq"].shape
    col = gate_cols(H)
    w = ops["w64"]
    hs = out["h_seq"].astype(np.float64)
    if sp:
        hs = hs + out["h_seq_lo"]
    cs = out["c_seq"].astype(np.float64)
    h_in = np.concatenate([ops["h0"].astype(np.float64)[None], hs[:-1]])
    c_in = np.concatenate([ch["c0"].astype(np.float64)[None], cs[:-1]])
    if mutation == "stale_h" and T > 2:
        h_in[2:] = hs[:-2]
    if mutation == "slices_swapped":     # unit slices j and j ^ 1 exchanged in the recurrent operand
        n = np.arange(H)
        h_in = h_in[..., ((n // UNITS) ^ 1) * UNITS + n % UNITS]
    x = ch["xproj"].astype(np.float64)
    c_forget = cs if mutation == "c_in_t" else None
    a, gates, c, h = forward_step(x, h_in, c_in, w, c_forget=c_forget, mutation=mutation)
    S = np.abs(h_in) @ np.abs(w).T
    n = 3 * H if sp else H
    da = (n + 2) * U * (S + np.abs(x))
    if sp:
        r = np.full((T, 1, 1), 2 * 2.0 ** -17 + 2.0 ** -16 + 2.0 ** -20)
        r[0] = 2.0 ** -17 + 2.0 ** -16
        da = da + r * (1 + 2.0 ** -15) * S
    e_g = np.empty_like(a)
    for q, (eps, lip) in enumerate(((EPS_SIG, 0.25), (EPS_SIG, 0.25), (EPS_TANH, 1.0), (EPS_SIG, 0.25))):
        e_g[..., col[q]] = eps + lip * da[..., col[q]]
    gi, gf, gg, go = (np.abs(gates[..., col[q]]) for q in range(4))
    ei, ef, eg, eo = (e_g[..., col[q]] for q in range(4))
    if mutation == "gates_preact":       # bounds of the true gates (the mutated reference is `a`)
        gi, gf, gg, go = _sig(a[..., col[0]]), _sig(a[..., col[1]]), np.abs(np.tanh(a[..., col[2]])), _sig(a[..., col[3]])
    e_c = ef * np.abs(c_in) + ei * gg + eg * gi + ei * eg + 3 * U * (gf * np.abs(c_in) + gi * gg)
    e_h = eo * np.abs(np.tanh(c)) + (go + eo) * (EPS_TANH + e_c) + 2 * U * np.abs(h)
    return dict(gates=gates, c=c, h=h, e_gates=e_g, e_c=e_c, e_h=e_h, c_in=c_in, h_in=h_in)


def check_forward(label, ch, out, sp: bool, mutation: Optional[str] = None):
    """All forward checks of one chain.  ``ch``: the chain's fp32 operands (w, h0, c0, xproj,
    save_from); ``out``: what the entry point left: h_seq (fp32 values of the bf16 plane),
    h_seq_bits, c_seq, and where present h_seq_lo / h_seq_lo_bits, h32, gates (T - save_from rows).
    Returns the largest use of each bound, dict(gates, c, h (the fp32 output h32), h_seq (the
    stored planes))."""
    ops = forward_operands(ch, sp)
    ref = forward_reference(ch, ops, out, sp, mutation)
    T, B, H = out["c_seq"].shape
    sf = int(ch["save_from"]) + (1 if mutation == "save_from_off" else 0)
    uses = dict(gates=0.0, c=0.0, h=0.0, h_seq=0.0)
    uses["c"] = compare(label, "c_seq", out["c_seq"], ref["c"], ref["e_c"])
    h32 = out.get("h32")
    if h32 is not None:
        uses["h"] = compare(label, "h32", h32, ref["h"], ref["e_h"])
        # bound-free: the stored planes are the roundings of the fp32 output, bit for bit
        bits_equal(label, "h_seq vs bf16(h32)", out["h_seq_bits"], bf16_bits(h32))
        if sp:
            lo = bf16_bits((h32 - bf16_round(h32)).astype(np.float32))
            bits_equal(label, "h_seq_lo vs bf16(h32 - h_seq)", out["h_seq_lo_bits"], lo)
    if sp:    # hi = bf16(x) and lo = bf16(x - hi) for some x within e_h of the reference (x - hi is exact)
        hi = out["h_seq"].astype(np.float64)
        uses["h_seq"] = max(compare_bf16(label, "h_seq", out["h_seq_bits"], ref["h"], ref["e_h"]),
                            compare_bf16(label, "h_seq_lo", out["h_seq_lo_bits"], ref["h"] - hi, ref["e_h"]))
    else:     # bf16 output: some value within e_h of the reference rounds to it (compare_bf16)
        uses["h_seq"] = compare_bf16(label, "h_seq", out["h_seq_bits"], ref["h"], ref["e_h"])
    g = out.get("gates")
    if g is not None and sf < T and g.shape[0] > 0:
        n = min(g.shape[0], T - sf)
        uses["gates"] = compare(label, "gates", g[:n], ref["gates"][sf:sf + n], ref["e_gates"][sf:sf + n],
                                 names=("t-save_from", "b", "packed col"))
        if mutation is None:
            # bound-free: c_seq[t] == f c_in + i g in fp32 from the saved gates and the stored c_in,
            # within 2^-23 (|f c_in| + |i g|) (two roundings more or fewer: fused multiply-add)
            col = gate_cols(H)
            g64 = g.astype(np.float64)
            p1 = g64[..., col[1]] * ref["c_in"][sf:]
            p2 = g64[..., col[0]] * g64[..., col[2]]
            compare(label, "c_seq vs saved gates", out["c_seq"][sf:], p1 + p2,
                     2.0 ** -23 * (np.abs(p1) + np.abs(p2)) + 1e-45)
    return uses


# ------------------------------------------------------------------------------------------
# backward: reference, bounds, checks

def backward_operands(bw, sp: bool):
    """W_hh as the backward entry points read it: bf16(w), or hi / lo planes in split precision."""
    if sp:
        hi, lo = split_planes(bw["w"])
        return dict(w_hi=hi, w_lo=lo, w64=hi.astype(np.float64) + lo)
    hi = bf16_round(bw["w"])
    return dict(w_hi=hi, w_lo=None, w64=hi.astype(np.float64))


def dz_dh_ext(bw):
    """dh_ext of the in-BPTT path: (dz + dz_lo)[(t - t0) B + b, :] @ (w1t + w1t_lo)^T in float64,
    and Z = |dz| @ |w1t|^T for its bound.  Returns ((K, B, H), (K, B, H))."""
    K, B = bw["T"] - bw["t0"], bw["B"]
    dz = bw["dz_hi"].astype(np.float64) + bw["dz_lo"]
    w1 = bw["w1t_hi"].astype(np.float64) + bw["w1t_lo"]
    return (dz @ w1.T).reshape(K, B, -1), (np.abs(dz) @ np.abs(w1).T).reshape(K, B, -1)


def backward_reference(bw, ops, dg_stored, sp: bool, mutation: Optional[str] = None):
    """Teacher-forced float64 BPTT with per-element bounds.  ``dg_stored`` (K, B, 4H): the gate
    gradients the kernel stored (bf16 plane, or hi + lo), the operand of its recurrent product.
    Returns dict(dg (K, B, 4H), e_dg: bound of the *unrounded* gate gradients).

    Step t (descending): dh = dh_ext[t - t0] + dg_stored[t + 1 - t0] @ W (t < T - 1); dc is carried
    here in float64 and its bound e_dc beside it.
      e_dh = cr P + cz Z + u |dh_ext|,  P = |dg_stored| @ |W|, Z = |dz| @ |W1| (dz path only).
        cr: per source workgroup a K = 64 sum of exact products in fp32 ((64 + 2) u, three passes in
        split precision: (192 + 2) u plus the dropped lo.lo term 2^-16), rounded to 19 mantissa bits
        (2^-20), then NWG partials and dh_ext added in fp32 ((NWG + 1) u).  With the dz path the
        source sum has 96 products per pass.  cz: at the first iteration dh_ext is a K = 512 product
        in three passes over four waves ((3 * 512 + 2 + 4) u + 2^-16); afterwards it rides inside the
        partials (cr).
      tc = tanh(c_t) within eps_tanh; (1 - tc^2) within 2 |tc| eps + eps^2 + u (product and
        difference rounded: u tc^2 + u (1 - tc^2)).
      dc_tot = dc + dh o (1 - tc^2):
        e_tot = e_dc + e_dh |o (1 - tc^2)| + (|dh| + e_dh) o (2 |tc| eps + eps^2 + u) + 2u |dh o (1 - tc^2)| + u |dc_tot|
      carry  e_dc' = f e_tot + u |dc_tot f|      (e' = f e + local terms)
      gate gradients: each a product of dc_tot (or dh tc) with saved gates; every factor (1 - q) or
        (1 - q^2) is within u absolutely, each product rounds once:
        e_i = e_tot |g i (1-i)| + 4u |dg_i|     e_f = e_tot |c_prev f (1-f)| + 4u |dg_f|
        e_g = e_tot |i (1-g^2)| + u |dc_tot i| + 3u |dg_g|
        e_o = e_dh |tc o (1-o)| + (|dh| + e_dh) o (1-o) eps_tanh + 4u |dg_o|
    """
    T, t0, B = bw["T"], bw["t0"], bw["B"]
    K = T - t0
    w = ops["w64"]
    H = w.shape[1]
    nwg = H // UNITS
    col = gate_cols(H)
    gates = bw["gates"].astype(np.float64)
    cs = bw["c_seq"].astype(np.float64)
    dz_on = bw.get("dz_hi") is not None
    if dz_on:
        dhx, Z = dz_dh_ext(bw)
    elif bw.get("dh_ext") is not None:
        dhx, Z = bw["dh_ext"].astype(np.float64), None
    else:
        dhx, Z = np.zeros((K, B, H)), None
    per_src = (96 if dz_on else 64) * (3 if sp else 1) + 2
    cr = (per_src + nwg + 1) * U + 2.0 ** -20 + (2.0 ** -16 if sp else 0.0)
    cz0 = (3 * DZ_K + 6) * U + 2.0 ** -16
    dgs = np.asarray(dg_stored, np.float64)
    dc = np.zeros((B, H))
    e_dc = np.zeros((B, H))
    dg = np.zeros((K, B, 4 * H))
    e_dg = np.zeros((K, B, 4 * H))
    for k, t in enumerate(range(T - 1, t0 - 1, -1)):
        tl = t - t0
        x = dhx[min(tl + 1, K - 1)] if mutation == "dh_ext_next" else dhx[tl]
        if mutation == "dz_first_omitted" and k == 0:
            x = np.zeros_like(x)
        dh = x.copy()
        e_dh = (cz0 if k == 0 else cr) * Z[tl] if dz_on else U * np.abs(x)
        if k > 0:
            rec = dgs[tl + 1] @ w
            if mutation == "no_rec_step" and k == 1:
                rec = 0.0 * rec
            if mutation == "no_rec_wg":     # source workgroup 1's partial missing
                s = slice(GCOLS, 2 * GCOLS)
                rec = rec - dgs[tl + 1][:, s] @ w[s]
            dh = dh + rec
            e_dh = e_dh + cr * (np.abs(dgs[tl + 1]) @ np.abs(w))
        c_prev = cs[t - 1] if t > 0 else bw["c0"].astype(np.float64)
        if mutation == "cprev_c0" and t == t0:
            c_prev = bw["c0_stale"].astype(np.float64)
        dc_in = np.zeros_like(dc) if (mutation == "drop_dc" and k == 1) else dc
        c_tanh = c_prev if mutation == "tanh_prev" else None
        g = gates[tl]
        dg[tl], dc, dc_tot, tc = backward_step(dh, dc_in, g, cs[t], c_prev, mutation, c_tanh)
        gi, gf, gg, go = (g[:, col[q]] for q in range(4))
        tcb = np.abs(np.tanh(cs[t]))
        om = 1.0 - tcb * tcb
        e_om = 2 * tcb * EPS_TANH + EPS_TANH ** 2 + U
        adh = np.abs(dh) + e_dh
        e_tot = (e_dc + e_dh * go * om + adh * go * e_om + 2 * U * np.abs(dh * go * om) + U * np.abs(dc_tot))
        a = np.abs(dg[tl])
        e_dg[tl][:, col[0]] = e_tot * np.abs(gg * gi * (1 - gi)) + 4 * U * a[:, col[0]]
        e_dg[tl][:, col[1]] = e_tot * np.abs(c_prev * gf * (1 - gf)) + 4 * U * a[:, col[1]]
        e_dg[tl][:, col[2]] = e_tot * np.abs(gi * (1 - gg * gg)) + U * np.abs(dc_tot * gi) + 3 * U * a[:, col[2]]
        e_dg[tl][:, col[3]] = e_dh * tcb * go * (1 - go) + adh * go * (1 - go) * EPS_TANH + 4 * U * a[:, col[3]]
        e_dc = gf * e_tot + U * np.abs(dc_tot * gf)
    return dict(dg=dg, e_dg=e_dg)


def stored_dgates(out, sp: bool):
    """The gate gradients as stored: fp32 values of the bf16 plane, or hi + lo in float64."""
    d = out["dgates"].astype(np.float64)
    return d + out["dgates_lo"] if sp else d


def check_backward(label, bw, out, sp: bool, mutation: Optional[str] = None, ref=None):
    """Gate gradients of every step against the teacher-forced reference.  The stored format adds
    its rounding: a bf16 plane is accepted exactly when some value x inside the bound rounds to it
    (``compare_bf16``); in split precision the lo plane likewise against x - hi, which fp32 holds
    exactly (csrc/split.h sp_lo).  No allowance is added for the formats.  Returns
    (largest use, reference dict)."""
    got = stored_dgates(out, sp)
    if ref is None:
        ref = backward_reference(bw, backward_operands(bw, sp), got, sp, mutation)
    names = ("t-t0", "b", "packed col")
    if sp:
        hi = out["dgates"].astype(np.float64)
        use = max(compare_bf16(label, "dgates", out["dgates_bits"], ref["dg"], ref["e_dg"], names=names),
                  compare_bf16(label, "dgates_lo", out["dgates_lo_bits"], ref["dg"] - hi, ref["e_dg"], names=names))
    else:
        use = compare_bf16(label, "dgates", out["dgates_bits"], ref["dg"], ref["e_dg"], names=names)
    return use, ref


def bias_reference(bw, ref, mutation: Optional[str] = None):
    """Bias gradient: column sums of the unrounded gate gradients over the valid rows and all steps,
    delivered through ``perm`` (db[perm[c]] = sum of packed column c).  Bound: the sum of the
    elements' bounds plus an fp32 sum of n = K B terms in any order, (n + 2) u sum |dg|.
    Returns (db, e_db) in PyTorch gate order."""
    dg, e = ref["dg"], ref["e_dg"]
    K, B, G = dg.shape
    s = dg.sum((0, 1))
    if mutation == "bias_tail_row" and B % 16:      # the clamped padding rows of the last tile
        s = s + (16 - B % 16) * dg[:, B - 1].sum(0)
    if mutation == "bias_no_last_tile":
        s = s - dg[:, (B - 1) // 16 * 16:].sum((0, 1))
    eb = e.sum((0, 1)) + (K * B + 2) * U * np.abs(dg).sum((0, 1)) + 1e-45
    perm = gate_perm(G // 4)
    db, e_db = np.empty(G), np.empty(G)
    if mutation == "perm_inverse":
        db, e_db = s[perm], eb[perm]
    else:
        db[perm], e_db[perm] = s, eb
    return db, e_db


def check_bias_grad(label, bw, out, ref, mutation: Optional[str] = None):
    """db1 against the reference within its bound; db2 == db1 bit for bit.  Returns the largest use."""
    db, e_db = bias_reference(bw, ref, mutation)
    use = compare(label, "db1", out["db1"], db, e_db, names=("gate row",))
    if out.get("db2") is not None:
        bits_equal(label, "db2 vs db1", np.asarray(out["db2"], np.float32).view(np.uint32),
                    np.asarray(out["db1"], np.float32).view(np.uint32), names=("gate row",))
    return use


# ------------------------------------------------------------------------------------------
# head-gradient side job (csrc/kernels/gradsum.hip header; run by the BPTT's helper workgroups)

def head_case(A: int, N: int = 40, HD: int = 64, seed: int = 0):
    """Operands of the head-gradient job: dva (N, 1 + A) fp32, zr (N, 2 HD) fp32 (relu'd), dz
    (N, 2 HD) fp32; the bf16 entry reads bf16(zr) and bf16(dz), split precision zr in fp32 and dz as
    hi / lo planes."""
    rng = np.random.default_rng(1000 + 31 * A + seed)
    return dict(N=N, A=A, HD=HD, dva=rng.standard_normal((N, 1 + A)).astype(np.float32),
                zr=np.maximum(rng.standard_normal((N, 2 * HD)), 0).astype(np.float32),
                dz=rng.standard_normal((N, 2 * HD)).astype(np.float32))


def head_grads_reference(hc, sp: bool, mutation: Optional[str] = None):
    """d val.2.weight = dva[:, 0]^T zr[:, :HD], d adv.2.weight = dva[:, 1:]^T zr[:, HD:],
    d {val, adv}.2.bias = colsum(dva), d {val, adv}.0.bias = colsum(dz), in float64 over the operands
    the entry point reads.  Bounds: an fp32 sum of N products (or terms) in any order,
    (N + 2) u sum |a||b|; the bf16 x fp32 products are not exact, which the + 2 covers twice over
    together with the final adds.  Returns dict(name -> (ref, bound))."""
    N, HD = hc["N"], hc["HD"]
    dva = hc["dva"].astype(np.float64)
    if sp:
        zr = hc["zr"].astype(np.float64)
        hi, lo = split_planes(hc["dz"])
        dz = hi.astype(np.float64) + lo
    else:
        zr, dz = bf16_round(hc["zr"]).astype(np.float64), bf16_round(hc["dz"]).astype(np.float64)
    zv, za = zr[:, :HD], zr[:, HD:]
    if mutation == "head_halves_swapped":
        zv, za = za, zv
    gw2 = np.concatenate([dva[:, :1].T @ zv, dva[:, 1:].T @ za])
    e_w = (N + 3) * U * np.concatenate([np.abs(dva[:, :1]).T @ np.abs(zv), np.abs(dva[:, 1:]).T @ np.abs(za)])
    rows = slice(0, N - 1) if mutation == "head_last_row_missing" else slice(0, N)
    return dict(gw2=(gw2, e_w + 1e-45),
                gb2=(dva[rows].sum(0), (N + 2) * U * np.abs(dva).sum(0) + 1e-45),
                gb1=(dz[rows].sum(0), (N + 2) * U * np.abs(dz).sum(0) + 1e-45))


def check_head_grads(label, hc, out, sp: bool, mutation: Optional[str] = None):
    """gw2 (1 + A, HD), gb2 (1 + A), gb1 (2 HD) against the reference.  Returns the largest use."""
    ref = head_grads_reference(hc, sp, mutation)
    return max(compare(label, n, out[n], *ref[n], names=("row", "col")[:np.ndim(out[n])] or ("i",))
               for n in ("gw2", "gb2", "gb1"))


def emulate_head_grads(hc, sp: bool):
    """fp32 emulation: row-ordered fp32 accumulation of fp32 products."""
    f32 = np.float32
    N, HD = hc["N"], hc["HD"]
    if sp:
        zr = hc["zr"].astype(f32)
        hi, lo = split_planes(hc["dz"])
        dz = (hi + lo).astype(f32)
    else:
        zr, dz = bf16_round(hc["zr"]), bf16_round(hc["dz"])
    dva = hc["dva"].astype(f32)
    gw2 = np.zeros((1 + hc["A"], HD), f32)
    gb2, gb1 = np.zeros(1 + hc["A"], f32), np.zeros(2 * HD, f32)
    for r in range(N):
        gw2[0] += dva[r, 0] * zr[r, :HD]
        gw2[1:] += dva[r, 1:, None] * zr[r, None, HD:]
        gb2 += dva[r]
        gb1 += dz[r]
    return dict(gw2=gw2, gb2=gb2, gb1=gb1)


# ------------------------------------------------------------------------------------------
# fp32 emulation of the kernels (numpy float32 at the kernels' quantisation points)

def _sig32(x):
    one = np.float32(1)
    with np.errstate(over="ignore"):
        return (one / (one + np.exp(-x, dtype=np.float32))).astype(np.float32)


def _tanh32(x):
    one = np.float32(1)
    e = np.exp(np.float32(-2) * np.abs(x), dtype=np.float32)
    return np.copysign(((one - e) * (one / (one + e))).astype(np.float32), x)


def _mm32(a_hi, a_lo, b_hi, b_lo, kc):
    """sum_k a[., k] b[., k] in fp32, K chunks of ``kc``; three passes (lo.hi, hi.lo, hi.hi) per
    chunk when lo planes are given (csrc/split.h)."""
    acc = np.zeros((a_hi.shape[0], b_hi.shape[0]), np.float32)
    for k0 in range(0, a_hi.shape[1], kc):
        s = slice(k0, k0 + kc)
        if a_lo is not None:
            acc = acc + a_lo[:, s] @ b_hi[:, s].T
            acc = acc + a_hi[:, s] @ b_lo[:, s].T
        acc = acc + a_hi[:, s] @ b_hi[:, s].T
    return acc.astype(np.float32)


def emulate_forward(ch, sp: bool, T: int):
    """fp32 emulation of the tagged forward (bf16, or split precision with the 19-bit hand-off
    word).  Returns the ``out`` dict of check_forward (every optional output present)."""
    ops = forward_operands(ch, sp)
    B, H = ch["c0"].shape
    col = gate_cols(H)
    sf = int(ch["save_from"])
    c = ch["c0"].astype(np.float32)
    x = ch["xproj"].astype(np.float32)
    hseq, clist, h32, gates = [], [], [], []
    h = None
    for t in range(T):
        if sp:
            src = ops["h0"] if t == 0 else round19(h)
            a_hi, a_lo = split_planes(src)
        else:
            a_hi, a_lo = (ops["h0"] if t == 0 else bf16_round(h)), None
        pre = (_mm32(a_hi, a_lo, ops["w_hi"], ops["w_lo"], 32) + x[t]).astype(np.float32)
        gi, gf, gg, go = _sig32(pre[:, col[0]]), _sig32(pre[:, col[1]]), _tanh32(pre[:, col[2]]), _sig32(pre[:, col[3]])
        c = (gf * c + gi * gg).astype(np.float32)
        h = (go * _tanh32(c)).astype(np.float32)
        g = np.empty((B, 4 * H), np.float32)
        g[:, col[0]], g[:, col[1]], g[:, col[2]], g[:, col[3]] = gi, gf, gg, go
        clist.append(c), h32.append(h), gates.append(g)
    h32 = np.stack(h32)
    out = dict(c_seq=np.stack(clist), h32=h32, h_seq_bits=bf16_bits(h32), h_seq=bf16_round(h32),
               gates=np.stack(gates)[sf:] if sf < T else np.zeros((0, B, 4 * H), np.float32))
    if sp:
        lo = (h32 - out["h_seq"]).astype(np.float32)
        out["h_seq_lo_bits"], out["h_seq_lo"] = bf16_bits(lo), bf16_round(lo)
    return out


def emulate_backward(bw, sp: bool):
    """fp32 emulation of the tagged BPTT: 19-bit partials per source workgroup summed in source
    order, hi / lo gate-gradient images, per-tile bias sums added in tile order, and the in-BPTT
    dh_ext (dz path).  Returns the ``out`` dict of check_backward / check_bias_grad."""
    ops = backward_operands(bw, sp)
    T, t0, B = bw["T"], bw["t0"], bw["B"]
    K = T - t0
    H = ops["w_hi"].shape[1]
    nwg = H // UNITS
    col = gate_cols(H)
    f32 = np.float32
    one = f32(1)
    dz_on = bw.get("dz_hi") is not None
    gates, cs = bw["gates"].astype(f32), bw["c_seq"].astype(f32)
    dcr = np.zeros((B, H), f32)
    dg_hi, dg_lo = np.zeros((K, B, 4 * H), f32), np.zeros((K, B, 4 * H), f32)
    bsum = np.zeros((B, 4 * H), f32)
    parts = None
    for k, t in enumerate(range(T - 1, t0 - 1, -1)):
        tl = t - t0
        if dz_on:
            dh = np.zeros((B, H), f32)
            if k == 0:
                rows = slice(tl * B, tl * B + B)
                q = [_mm32(bw["dz_hi"][rows, 128 * w_:128 * w_ + 128], bw["dz_lo"][rows, 128 * w_:128 * w_ + 128],
                           bw["w1t_hi"][:, 128 * w_:128 * w_ + 128], bw["w1t_lo"][:, 128 * w_:128 * w_ + 128], 32)
                     for w_ in range(4)]
                dh = (((q[0] + q[1]) + q[2]) + q[3]).astype(f32)
        elif bw.get("dh_ext") is not None:
            dh = bw["dh_ext"][tl].astype(f32)
        else:
            dh = np.zeros((B, H), f32)
        if k > 0:
            quarter = []
            for w_ in range(4):
                s = np.zeros((B, H), f32)
                for i in range(nwg // 4):
                    s = s + parts[w_ * (nwg // 4) + i]
                quarter.append(s)
            dh = (dh + (((quarter[0] + quarter[1]) + quarter[2]) + quarter[3])).astype(f32)
        g = gates[tl]
        gi, gf, gg, go = (g[:, col[q]] for q in range(4))
        c_prev = cs[t - 1] if t > 0 else bw["c0"].astype(f32)
        tc = _tanh32(cs[t])
        dc = (dcr + dh * go * (one - tc * tc)).astype(f32)
        d_o = dh * tc
        dcr = (dc * gf).astype(f32)
        dg = np.empty((B, 4 * H), f32)
        dg[:, col[0]] = dc * gg * gi * (one - gi)
        dg[:, col[1]] = dc * c_prev * gf * (one - gf)
        dg[:, col[2]] = dc * gi * (one - gg * gg)
        dg[:, col[3]] = d_o * go * (one - go)
        bsum = (bsum + dg).astype(f32)
        dg_hi[tl] = bf16_round(dg)
        if sp:
            dg_lo[tl] = bf16_round((dg - dg_hi[tl]).astype(f32))
        if t > t0:
            parts = []
            for j in range(nwg):
                s = slice(j * GCOLS, (j + 1) * GCOLS)
                wt_hi = ops["w_hi"][s].T
                wt_lo = ops["w_lo"][s].T if sp else None
                acc = _mm32(dg_hi[tl][:, s], dg_lo[tl][:, s] if sp else None, wt_hi, wt_lo, 32)
                if dz_on:
                    rows, ks = slice((tl - 1) * B, (tl - 1) * B + B), slice(32 * j, 32 * j + 32)
                    acc = (acc + _mm32(bw["dz_hi"][rows, ks], bw["dz_lo"][rows, ks],
                                       bw["w1t_hi"][:, ks], bw["w1t_lo"][:, ks], 32)).astype(f32)
                parts.append(round19(acc))
    # per-tile column sums, tiles added in order; delivered through perm
    tot = np.zeros(4 * H, f32)
    for m in range((B + 15) // 16):
        tot = (tot + bsum[16 * m:16 * m + 16].sum(0, dtype=f32)).astype(f32)
    db = np.empty(4 * H, f32)
    db[gate_perm(H)] = tot
    out = dict(dgates=dg_hi, dgates_bits=bf16_bits(dg_hi), db1=db, db2=db.copy())
    if sp:
        out["dgates_lo"], out["dgates_lo_bits"] = dg_lo, bf16_bits(dg_lo)
    return out


# ------------------------------------------------------------------------------------------
# the cases (shared by the CPU and the GPU test)

FORWARD_CASES = {
    # name: H, B, T, save_from per chain, chains without h32, chains without gates, xproj scale
    "f_one":    dict(H=64, B=1, T=1, save_from=(0,)),
    "f_tail":   dict(H=64, B=17, T=3, save_from=(0, 2), no_h32=(1,), no_gates=(0,)),
    "f_map2":   dict(H=128, B=33, T=5, save_from=(0, 1, 4, 5)),
    "f_wrap":   dict(H=256, B=16, T=10, save_from=(0,)),
    "f_512":    dict(H=512, B=33, T=2, save_from=(0,)),
    "f_linear": dict(H=64, B=80, T=4, save_from=(0, 0, 0, 0)),
    "f_wide":   dict(H=64, B=144, T=3, save_from=(0,)),
    "f_sat":    dict(H=64, B=17, T=3, save_from=(0,), xscale=8.0),
}

BACKWARD_CASES = {
    "b_one":  dict(H=64, B=1, T=1, t0=0),
    "b_tail": dict(H=64, B=17, T=4, t0=0),
    "b_burn": dict(H=128, B=33, T=6, t0=2),
    "b_wrap": dict(H=256, B=16, T=12, t0=1),
    "b_last": dict(H=512, B=33, T=3, t0=2),
    "b_wpm2": dict(H=64, B=80, T=5, t0=1),
    "b_wide": dict(H=64, B=144, T=3, t0=0),
    "b_nodh": dict(H=64, B=17, T=3, t0=0, no_dh=True),
    "b_dz":   dict(H=256, B=17, T=4, t0=1, dz=True),
    "b_hg":   dict(H=256, B=16, T=4, t0=1),      # with the head-gradient job (head_case) beside it
}


def _rng(name: str, launch: int):
    return np.random.default_rng(zlib.crc32(name.encode()) + 7919 * launch)


def _weights(rng, H):
    """W_hh ~ 0.06 sqrt(256 / H) N(0, 1), generated directly in packed form ((4H, H) packed rows)."""
    return (0.06 * np.sqrt(256.0 / H) * rng.standard_normal((4 * H, H))).astype(np.float32)


def forward_case(name: str, launch: int = 0):
    """Operands of forward case ``name`` (``launch``: a second, different input set for the same
    launch site).  Returns (spec, [chain dict(w, xproj, h0, c0, save_from, h32, gates)])."""
    spec = FORWARD_CASES[name]
    rng = _rng(name, launch)
    H, B, T = spec["H"], spec["B"], spec["T"]
    chains = []
    for c, sf in enumerate(spec["save_from"]):
        chains.append(dict(
            w=_weights(rng, H),
            xproj=(spec.get("xscale", 1.0) * rng.standard_normal((T, B, 4 * H))).astype(np.float32),
            h0=(0.3 * rng.standard_normal((B, H))).astype(np.float32),
            c0=(0.5 * rng.standard_normal((B, H))).astype(np.float32),
            save_from=sf, h32=c not in spec.get("no_h32", ()), gates=c not in spec.get("no_gates", ())))
    return spec, chains


def backward_case(name: str, launch: int = 0):
    """Operands of backward case ``name``.  gates / c_seq come from the oracle's own float64 forward
    (free running, bf16 weights), rounded to fp32, so the backward is isolated from the forward
    kernels.  What must not influence the result is NaN: c0 when t0 > 0 (``c0_stale`` keeps the
    values for the mutation that reads it) and c_seq rows before t0 - 1."""
    spec = BACKWARD_CASES[name]
    rng = _rng(name, launch)
    H, B, T, t0 = spec["H"], spec["B"], spec["T"], spec["t0"]
    K = T - t0
    w = _weights(rng, H)
    xproj = rng.standard_normal((T, B, 4 * H))
    h0, c0 = 0.3 * rng.standard_normal((B, H)), 0.5 * rng.standard_normal((B, H))
    g, c, _ = free_forward(xproj, bf16_round(w).astype(np.float64), h0, c0)
    bw = dict(H=H, B=B, T=T, t0=t0, w=w, gates=g[t0:].astype(np.float32), c_seq=c.astype(np.float32),
              c0=c0.astype(np.float32), c0_stale=c0.astype(np.float32),
              dh_ext=None if spec.get("no_dh") else rng.standard_normal((K, B, H)).astype(np.float32))
    if t0 > 0:
        bw["c0"] = np.full((B, H), np.nan, np.float32)
        bw["c_seq"][:t0 - 1] = np.nan
    if spec.get("dz"):
        bw["dz_hi"], bw["dz_lo"] = split_planes((0.2 * rng.standard_normal((K * B, DZ_K))).astype(np.float32))
        bw["w1t_hi"], bw["w1t_lo"] = split_planes((0.2 * rng.standard_normal((H, DZ_K))).astype(np.float32))
        bw["dh_ext"] = None
    return spec, bw


def activation_grid():
    """8192 pre-activations: [-30, 30] linearly plus +-{0, 1e-8, 1e-4, 87, 88.5, 89, 104, 1e4}."""
    s = np.array([0, 1e-8, 1e-4, 87, 88.5, 89, 104, 1e4])
    return np.concatenate([np.linspace(-30, 30, 8192 - 16), s, -s]).astype(np.float32)


def check_activations(label, gates, grid):
    """Saved gates of the sweep (H 64, B 128, T 1, W_hh = 0, h0 = 0): gate q of (row b, unit n) is
    the activation of grid[64 b + n].  Within eps_act of float64, finite and inside [0, 1] /
    [-1, 1].  Returns (sigmoid use, tanh use)."""
    col = gate_cols(64)
    x = grid.astype(np.float64).reshape(128, 64)
    us, ut = 0.0, 0.0
    for q in range(4):
        got = gates[:, col[q]]
        lo = -1.0 if q == 2 else 0.0
        if not (np.isfinite(got).all() and (got >= lo).all() and (got <= 1.0).all()):
            raise AssertionError(f"{label}: gate {q} leaves [{lo}, 1] or is not finite")
        if q == 2:
            ut = compare(label, "tanh", got, np.tanh(x), np.full(x.shape, EPS_TANH), names=("b", "unit"))
        else:
            us = max(us, compare(label, f"sigmoid (gate {q})", got, _sig(x), np.full(x.shape, EPS_SIG),
                                  names=("b", "unit")))
    return us, ut


# ------------------------------------------------------------------------------------------
# the split-precision step kernel (csrc/kernels/lstm_step_sp.hip, r2_lstm_fwd_sp): its cases, shared
# by tests/test_lstm_step_sp_cpu.py and tests/test_lstm_step_sp_gpu.py.  The oracle is
# check_forward(sp=True) unchanged: its t > 0 bound also allows for the 19-bit hand-off word, which
# this kernel does not use (it reads the stored planes), so that bound is looser, not wrong.

STEP_SP_CASES = {
    # name: H, B (rows per chain), T, save_from per chain, chains without gates / h32; ``halves``:
    # the chains are nets x two row halves of 2 B-row buffers (pointer offsets, as PolicyInference.run calls it)
    "s_clamp":  dict(H=64, B=5, T=1, save_from=(0,)),                      # one partial M tile
    "s_tile2":  dict(H=64, B=33, T=3, save_from=(0, 1), no_gates=(1,)),    # second tile partial
    "s_full":   dict(H=64, B=128, T=1, save_from=(0,)),
    "s_h128":   dict(H=128, B=40, T=2, save_from=(2, 0), no_h32=(0,)),     # the H = 128 instance
    "s_halves": dict(H=256, B=65, T=1, save_from=(0, 0, 0, 0), no_gates=(1, 2, 3), halves=True),
}


def step_sp_case(name: str):
    """Operands of step case ``name``.  Returns (spec, chains); with ``halves`` chains 2n and 2n + 1
    are rows [0, B) and [B, 2B) of net n's operands (same w), and ``chain["net"]`` / ``["row0"]``
    say where the chain lives in its net's buffers."""
    spec = STEP_SP_CASES[name]
    rng = _rng(name, 0)
    H, B, T = spec["H"], spec["B"], spec["T"]
    per = 2 if spec.get("halves") else 1
    chains = []
    for c, sf in enumerate(spec["save_from"]):
        if c % per == 0:
            w = _weights(rng, H)
            x = rng.standard_normal((T, per * B, 4 * H)).astype(np.float32)
            h0 = (0.3 * rng.standard_normal((per * B, H))).astype(np.float32)
            c0 = (0.5 * rng.standard_normal((per * B, H))).astype(np.float32)
        r0 = (c % per) * B
        chains.append(dict(w=w, xproj=np.ascontiguousarray(x[:, r0:r0 + B]), h0=h0[r0:r0 + B].copy(),
                           c0=c0[r0:r0 + B].copy(), save_from=sf, net=c // per, row0=r0,
                           h32=c not in spec.get("no_h32", ()), gates=c not in spec.get("no_gates", ())))
    return spec, chains
