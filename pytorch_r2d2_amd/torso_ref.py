"""Float64 oracle of the conv torso kernels: the bf16 forward and backward (csrc/kernels/torso.hip,
torso_bwd.hip) and the split-precision forward and backward (torso_sp.hip).

Pure host code (numpy, no torch, no GPU), parametrised by the frame geometry (cin, h, w):
Conv(cin,32,8,s4)-ReLU-Conv(32,32,4,s2)-ReLU-Conv(32,32,3,s1)-ReLU on uint8 frames scaled by 1/255.

Forward: *teacher forced*.  conv1 is recomputed from the uint8 frame, conv2 from the ``save1`` the
kernel stored, conv3 from the stored ``save2``, so every check is a one-layer check whose bound can
be derived per element (``layer_reference``).

Backward: the operands (frames, act1, act2, out3, dx3, weights) are free inputs.  The intermediate
gradients g2 and g1 live only in LDS, so the oracle carries float64 values plus per-element error
intervals and propagates them linearly (``backward_frame``); each slab row (one per workgroup, the
partial sum over frames f = g mod grid) is referenced separately (``slab_reference``), and the
reduction is checked from the stored slab (``check_reduce``).

Also here: the packed layouts (plain indexing from (co, ci, kh, kw) weights, independent of
engine/layout.py), an fp32/bf16 emulation of the kernels' arithmetic (``emulate_*``: the roundings,
not the addressing -- the condition that the bounds are not too tight, checked on the CPU), the
``mutation=`` variants (deliberately wrong oracles the checks must reject -- the condition that they
are not too loose) and the case tables that tests/test_torso_ref_cpu.py and
tests/test_torso_oracle_gpu.py share.

The split-precision backward (torso_bwd_sp_kernel, torso_dw3_sp_kernel) shares the backward oracle
(``sp=True``: three passes, hi / lo planes, its own frame deal for dW3).
"""
from __future__ import annotations

import zlib
from typing import Optional

import numpy as np

from .lstm_ref import U
# the ownership checks are not used below: they stay part of this oracle's interface
from .refnum import (bf16_bits, bf16_round, bf16_val, check_ownership, check_untouched,  # noqa: F401
                     compare, compare_bf16, split_planes)

C = 32                      # channels of every conv layer
EPS_BF16 = 2.0 ** -8        # bf16 unit roundoff: 8 significand bits, so half an ulp is up to 2^-8 |x|
                            # (x = 1 + 2^-8 rounds to 1 or 1 + 2^-7); 2^-9 is exceeded by a correct rounding

MUTATIONS_FWD = ("c1_last_col", "pad_lanes_written", "c2_khkw_swapped", "s2d_dy_misordered",
                 "bias_wrong_half", "save1_late", "stale_frame")
MUTATIONS_SP = MUTATIONS_FWD + ("w1_digit3_dropped",)
MUTATIONS_BWD_SP = ("c3t_corner_tap", "s2_wrong_phase", "mask_neighbour", "no_255", "db2_before_mask",
                    "c3_pad_pixel_twice", "dx3_lo_dropped")
MUTATIONS_BWD = ("c3t_corner_tap", "s2_wrong_phase", "mask_neighbour", "no_255", "db2_before_mask",
                 "c3_pad_pixel_twice")


class Geo:
    """The layer extents of one frame geometry (TGeo / TBGeo of the kernels)."""

    def __init__(self, cin: int, h: int, w: int):
        self.cin, self.h, self.w = cin, h, w
        self.fb = cin * h * w
        self.H1, self.W1 = (h - 8) // 4 + 1, (w - 8) // 4 + 1
        self.H2, self.W2 = (self.H1 - 4) // 2 + 1, (self.W1 - 4) // 2 + 1
        self.H3, self.W3 = self.H2 - 2, self.W2 - 2
        self.P1, self.P2, self.P3 = self.H1 * self.W1, self.H2 * self.W2, self.H3 * self.W3
        self.OUT = C * self.P3
        self.K1 = 64 * cin
        # backward: K steps of 16 pixels (dW2, dW3) and 4x4 pixel blocks (dW1), slab offsets
        self.K2S, self.K3S = (self.P2 + 15) // 16, (self.P3 + 15) // 16
        self.NB1 = ((self.H1 + 3) // 4) * ((self.W1 + 3) // 4)
        self.OFF_W2 = C * self.K1
        self.OFF_W3 = self.OFF_W2 + C * 512
        self.OFF_B = self.OFF_W3 + C * 288
        self.SLAB = self.OFF_B + 3 * C

    @property
    def key(self):
        return (self.cin, self.h, self.w)


GEOMS = {"atari": Geo(4, 84, 84), "dmlab": Geo(3, 72, 96)}


# ------------------------------------------------------------------------------------------
# packed layouts

def pack_conv1(w) -> np.ndarray:
    """(co, ci, 8, 8) -> (co, 64 ci) in space-to-depth K order (by, bx, ci, dy, dx), kh = 4 by + dy,
    kw = 4 bx + dx: the 8x8/s4 conv as a 2x2/s1 conv on the (h/4, w/4, 16 ci) image."""
    co, ci = w.shape[:2]
    out = np.empty((co, 2, 2, ci, 4, 4), w.dtype)
    for by in range(2):
        for bx in range(2):
            for dy in range(4):
                for dx in range(4):
                    out[:, by, bx, :, dy, dx] = w[:, :, 4 * by + dy, 4 * bx + dx]
    return out.reshape(co, -1)


def pack_hwc(w) -> np.ndarray:
    """(co, ci, k, k) -> (co, (kh, kw, ci)): conv2 and conv3."""
    co, ci, k, _ = w.shape
    out = np.empty((co, k, k, ci), w.dtype)
    for kh in range(k):
        for kw in range(k):
            out[:, kh, kw, :] = w[:, :, kh, kw]
    return out.reshape(co, -1)


def pack_conv3_dg(w3) -> np.ndarray:
    """conv3_dg[ci][kh][kw][co] = W3[co][ci][kh][kw], (32, 288)."""
    co, ci = w3.shape[:2]
    out = np.empty((ci, 3, 3, co), w3.dtype)
    for kh in range(3):
        for kw in range(3):
            out[:, kh, kw, :] = w3[:, :, kh, kw].T
    return out.reshape(ci, -1)


def pack_conv2_dg(w2) -> np.ndarray:
    """conv2_dg[py, px][ci][khi][kwi][co] = W2[co][ci][py + 2 khi][px + 2 kwi], (4, 32, 128)."""
    co, ci = w2.shape[:2]
    out = np.empty((2, 2, ci, 2, 2, co), w2.dtype)
    for py in range(2):
        for px in range(2):
            for khi in range(2):
                for kwi in range(2):
                    out[py, px, :, khi, kwi, :] = w2[:, :, py + 2 * khi, px + 2 * kwi].T
    return out.reshape(4, ci, -1)


def slab_map(geo: Geo, off: dict):
    """(dst int32, scale float32) of the slab [dW1 (co, ci, kh, kw) | dW2 (co, kh, kw, ci) |
    dW3 (co, kh, kw, ci) | db1 | db2 | db3]: ``off`` holds the position of the torch-order tensors
    w1, b1, w2, b2, w3, b3 in the flat gradient.  dW1 is accumulated against the integer frame, so
    it alone carries the scale 1/255."""
    dst = np.empty(geo.SLAB, np.int64)
    scale = np.ones(geo.SLAB, np.float32)
    dst[:geo.OFF_W2] = off["w1"] + np.arange(C * geo.K1)
    scale[:geo.OFF_W2] = np.float32(1.0 / 255.0)
    for o, name, k in ((geo.OFF_W2, "w2", 4), (geo.OFF_W3, "w3", 3)):
        idx = np.empty((C, k, k, C), np.int64)
        for co in range(C):
            for kh in range(k):
                for kw in range(k):
                    idx[co, kh, kw, :] = off[name] + ((co * C + np.arange(C)) * k + kh) * k + kw
        dst[o:o + idx.size] = idx.reshape(-1)
    for i, name in enumerate(("b1", "b2", "b3")):
        dst[geo.OFF_B + C * i:geo.OFF_B + C * (i + 1)] = off[name] + np.arange(C)
    return dst.astype(np.int32), scale


def pack_slab(geo: Geo, dw1, dw2, dw3, db1, db2, db3) -> np.ndarray:
    """Torch-order gradients -> one slab row."""
    return np.concatenate([dw1.reshape(-1), pack_hwc(dw2).reshape(-1), pack_hwc(dw3).reshape(-1),
                           db1, db2, db3])


# ------------------------------------------------------------------------------------------
# operands

def _rng(name: str):
    return np.random.default_rng(zlib.crc32(name.encode()))


def make_weights(geo: Geo, seed: str) -> dict:
    """bf16-exact weights and fp32 biases; zero-mean weights on non-negative inputs leave about
    half of every layer's pre-activations negative, the biases move each channel's share."""
    r = _rng("w/" + seed)
    w = {"seed": seed}
    for name, shape, k, gain in (("w1", (C, geo.cin, 8, 8), geo.K1, 2.0), ("w2", (C, C, 4, 4), 512, 1.5),
                                 ("w3", (C, C, 3, 3), 288, 1.5)):
        w[name] = bf16_round(r.standard_normal(shape) * gain / np.sqrt(k))
    for name in ("b1", "b2", "b3"):
        w[name] = (0.3 * r.standard_normal(C)).astype(np.float32)
    w["w1_pk"], w["w2_pk"], w["w3_pk"] = pack_conv1(w["w1"]), pack_hwc(w["w2"]), pack_hwc(w["w3"])
    w["w3_dg"], w["w2_dg"] = pack_conv3_dg(w["w3"]), pack_conv2_dg(w["w2"])
    return w


def make_store(geo: Geo, seed: str, n_rows: int, row_pad: int, frames: str) -> np.ndarray:
    """(n_rows, frame bytes + row_pad) uint8 replay rows; the pad bytes are random in every mode."""
    r = _rng("s/" + seed)
    store = r.integers(0, 256, (n_rows, geo.fb + row_pad), dtype=np.uint8)
    if frames == "zeros":
        store[:, :geo.fb] = 0
    elif frames == "full":
        store[:, :geo.fb] = 255
    return store


def make_rows(seed: str, n: int, n_store: int, mode: str) -> Optional[np.ndarray]:
    if mode == "null":
        return None
    if mode == "identity":
        return np.arange(n, dtype=np.int32)
    r = _rng("r/" + seed)
    rows = r.integers(0, n_store, n).astype(np.int32)
    if mode == "dup_desc":
        rows = np.sort(rows)[::-1].copy()
        if n > 1:
            rows[1] = rows[0]
    return rows


def gather(geo: Geo, store, rows, n: int) -> np.ndarray:
    idx = np.arange(n) if rows is None else rows
    return store[idx, :geo.fb].reshape(n, geo.cin, geo.h, geo.w)


def deal_workers(ns, nw: int):
    """r2_torso_fwd_geom's worker deal: jobs with frames get workers in proportion to their frame
    counts, at least one and never more than their frames.  Returns [(job, wbegin, wcount)] of the
    live jobs, or None where the launcher refuses (-3: more jobs than workers)."""
    total, seen, wb, out = sum(n for n in ns if n > 0), 0, 0, []
    for j, n in enumerate(ns):
        if n <= 0:
            continue
        seen += n
        end = min((seen * nw + total - 1) // total, nw)
        cnt = min(max(end - wb, 1), n)
        out.append((j, wb, cnt))
        wb += cnt
    return None if wb > nw else out


def reserve_workers(reserve_xcds: int, reserve_slots: int) -> int:
    return (32 - reserve_slots) * 8 + reserve_slots * (8 - reserve_xcds)


# ------------------------------------------------------------------------------------------
# forward

def _windows(x, k: int, s: int) -> np.ndarray:
    """(n, H, W, ch) -> (n, Ho, Wo, kh, kw, ch)."""
    v = np.lib.stride_tricks.sliding_window_view(x, (k, k), axis=(1, 2))
    return v[:, ::s, ::s].transpose(0, 1, 2, 4, 5, 3)


def cols_conv1(geo: Geo, frames, mutation=None) -> np.ndarray:
    """uint8 (n, cin, h, w) -> (n, P1, 64 cin) im2col rows in the space-to-depth K order."""
    n = frames.shape[0]
    v = _windows(frames.transpose(0, 2, 3, 1), 8, 4)                    # n, H1, W1, kh, kw, ci
    v = v.reshape(n, geo.H1, geo.W1, 2, 4, 2, 4, geo.cin)               # .., by, dy, bx, dx, ci
    v = np.ascontiguousarray(v.transpose(0, 1, 2, 3, 5, 7, 4, 6))       # .., by, bx, ci, dy, dx
    if mutation == "s2d_dy_misordered":
        v[:, :, :, :, :, 0, [1, 2]] = v[:, :, :, :, :, 0, [2, 1]]
    return v.reshape(n, geo.P1, geo.K1)


def cols_hwc(act, Hi: int, Wi: int, k: int, s: int) -> np.ndarray:
    """(n, Hi Wi, 32) channels-last activations -> (n, Po, k k 32) rows in (kh, kw, ci) order."""
    n = act.shape[0]
    v = _windows(act.reshape(n, Hi, Wi, C), k, s)
    return v.reshape(n, v.shape[1] * v.shape[2], k * k * C)


def layer_reference(cols, wpk, b, scale: float):
    """One layer before ReLU and rounding, and its bound.

    The kernel forms acc = sum_k a_k w_k on the MFMA: each product is exact in fp32 (a is an integer
    <= 255 or a bf16 value, w is bf16: at most 16 significand bits), the K terms are accumulated in
    fp32 in some order: |acc - S| <= (K - 1) u T, T = sum |a_k||w_k|, u = 2^-24.  Then
    x = acc * fl(1/255) + b (conv1; the constant's representation, the product and the sum round
    once each, a contraction into one fma rounds less) or x = acc + b (one rounding): at most three
    further relative u of |S| scale + |b| <= T scale + |b|.  Hence
        |x - (S scale + b)| <= (K + 2) u (T scale + |b|),
    the project's (n + 2) u sum|a||w| convention with the bias as one more term.  ReLU is
    1-Lipschitz, so the same bound holds for max(x, 0) against max(ref, 0) with no exclusion near
    zero, and the stored value is the bf16 rounding of that (compared in the compare_bf16 sense)."""
    K = cols.shape[-1]
    a, w = cols.astype(np.float64), wpk.astype(np.float64)
    pre = a @ w.T * scale + b.astype(np.float64)
    T = np.abs(a) @ np.abs(w).T
    return pre, (K + 2) * U * (T * scale + np.abs(b.astype(np.float64)))


def forward_reference(geo: Geo, frames, wts, stored, stride: int = 1, mutation: Optional[str] = None):
    """{name: (relu(ref), bound)} for save1 (n, P1, 32), save2 (n, P2, 32), out (n, 32, P3);
    ``stored``: the kernel's save1 / save2 as bf16 bits (conv2 and conv3 are computed from them).
    ``stride``: the job's worker count (used by the stale-prefetch mutation only)."""
    n = frames.shape[0]
    w1, w2, w3, b2 = wts["w1_pk"], wts["w2_pk"], wts["w3_pk"], wts["b2"]
    if mutation == "stale_frame":       # conv1 of every iteration after the first reads the frame
        frames = frames.copy()          # the previous iteration left in LDS
        if n > stride:
            frames[stride:] = frames[:n - stride].copy()
    if mutation == "c2_khkw_swapped":
        w2 = pack_hwc(wts["w2"].transpose(0, 1, 3, 2))
    if mutation == "bias_wrong_half":   # the other lane half's accumulator rows: channel ^ 4
        b2 = b2[np.arange(C) ^ 4]
    p1, e1 = layer_reference(cols_conv1(geo, frames, mutation), w1, wts["b1"], 1.0 / 255.0)
    if mutation == "c1_last_col":
        p1 = p1.reshape(n, geo.H1, geo.W1, C).copy()
        p1[:, :, -1] = p1[:, :, -2]
        p1 = p1.reshape(n, geo.P1, C)
    if mutation == "save1_late":
        p1, e1 = np.roll(p1, 1, axis=1), np.roll(e1, 1, axis=1)
    s1 = bf16_val(stored["save1"]).reshape(n, geo.P1, C)
    p2, e2 = layer_reference(cols_hwc(s1, geo.H1, geo.W1, 4, 2), w2, b2, 1.0)
    s2 = bf16_val(stored["save2"]).reshape(n, geo.P2, C)
    p3, e3 = layer_reference(cols_hwc(s2, geo.H2, geo.W2, 3, 1), w3, wts["b3"], 1.0)
    relu = lambda x: np.maximum(x, 0.0)  # noqa: E731
    return dict(save1=(relu(p1), e1), save2=(relu(p2), e2),
                out=(relu(p3).transpose(0, 2, 1), e3.transpose(0, 2, 1)))


def check_forward(label, geo: Geo, frames, wts, stored, stride: int = 1, mutation=None) -> dict:
    """Every element of save1, save2 and out against the teacher-forced oracle; returns the largest
    use of each bound.  ``stored``: bf16 bits of save1 (n, P1, 32), save2 (n, P2, 32), out (n, 32, P3)."""
    ref = forward_reference(geo, frames, wts, stored, stride, mutation)
    names = dict(save1=("frame", "pixel", "channel"), save2=("frame", "pixel", "channel"),
                 out=("frame", "channel", "pixel"))
    return {k: compare_bf16(label, k, np.asarray(stored[k]).reshape(r.shape), r, e, names[k])
            for k, (r, e) in ref.items()}


def _layer32(cols, wpk, b, scale):
    acc = cols.astype(np.float32) @ wpk.astype(np.float32).T
    if scale is not None:
        acc = acc * np.float32(1.0 / 255.0)
    return bf16_bits(np.maximum((acc + b.astype(np.float32)).astype(np.float32), np.float32(0)))


def emulate_forward(geo: Geo, frames, wts) -> dict:
    """The forward kernel's arithmetic in fp32 with a bf16 rounding per stored element: bf16 bits
    of save1, save2, out."""
    n = frames.shape[0]
    s1 = _layer32(cols_conv1(geo, frames), wts["w1_pk"], wts["b1"], 1)
    s2 = _layer32(cols_hwc(bf16_val(s1), geo.H1, geo.W1, 4, 2), wts["w2_pk"], wts["b2"], None)
    o = _layer32(cols_hwc(bf16_val(s2), geo.H2, geo.W2, 3, 1), wts["w3_pk"], wts["b3"], None)
    return dict(save1=s1, save2=s2, out=np.ascontiguousarray(o.transpose(0, 2, 1)).reshape(n, C, geo.P3))


def guarded_image(bits, pad: int, spill: int = 0) -> np.ndarray:
    """What a NaN-poisoned, guard-banded buffer reads back as after a launch that wrote ``bits``
    (flat float view); ``spill`` elements past the end written too (tests: the padded lanes of the
    last pixel tile not dropped)."""
    v = bf16_val(np.asarray(bits).reshape(-1))
    full = np.full(v.size + 2 * pad, np.nan, np.float32)
    full[pad:pad + v.size] = v
    full[pad + v.size:pad + v.size + spill] = 0.0
    return full


# ------------------------------------------------------------------------------------------
# forward, split precision (torso_fwd_sp2_kernel; Atari geometry only)

def make_weights_sp(geo: Geo, seed: str, w1_mode: str = "random") -> dict:
    """fp32 weights carried as hi / lo bf16 planes (csrc/split.h); the kernel's operand is hi + lo.
    ``w1_mode``: "outlier" makes one element of W1 1000 x the rest (the digit scale is shared, so
    the conv1 bound grows with it), "zero" makes W1 all zero (act1 = ReLU(b1) exactly)."""
    r = _rng("wsp/" + seed)
    w = {"seed": f"{seed}/{w1_mode}"}
    for name, shape, k, gain in (("w1", (C, geo.cin, 8, 8), geo.K1, 2.0), ("w2", (C, C, 4, 4), 512, 1.5),
                                 ("w3", (C, C, 3, 3), 288, 1.5)):
        w[name] = (r.standard_normal(shape) * gain / np.sqrt(k)).astype(np.float32)
    if w1_mode == "outlier":
        w["w1"][17, 2, 5, 3] = np.float32(1000.0 * np.abs(w["w1"]).max())
    elif w1_mode == "zero":
        w["w1"][:] = 0
    for name in ("b1", "b2", "b3"):
        w[name] = (0.3 * r.standard_normal(C)).astype(np.float32)
    for name, pk in (("w1", pack_conv1), ("w2", pack_hwc), ("w3", pack_hwc)):
        hi, lo = split_planes(pk(w[name]))
        w[name + "_hi"], w[name + "_lo"] = hi, lo
        w[name + "_pk"] = hi.astype(np.float64) + lo          # the operand the kernel multiplies
    return w


def c1_digits(w32):
    """torso_sp.hip c1_digits in fp32: W1 (= hi + lo) -> three int8 digits under one scale.
    Returns (d0, d1, d2 int64 arrays, m = max|W1|, the epilogue scale fl(fl(m fl(1/127)) fl(1/255)))."""
    f = np.float32
    w32 = w32.astype(f)
    m = f(np.abs(w32).max())
    inv = f(127.0) / m if m > 0 else f(0)
    q = (w32 * inv).astype(f)
    d0 = np.rint(q)
    r1 = ((q - d0) * f(128)).astype(f)              # exact: |q - d0| <= 1/2 on q's grid
    d1 = np.rint(r1)
    d2 = np.rint(((r1 - d1) * f(128)).astype(f))
    scale = f(f(m * f(1.0 / 127.0)) * f(1.0 / 255.0))
    return d0.astype(np.int64), d1.astype(np.int64), d2.astype(np.int64), m, scale


def conv1_sp_reference(cols, wts, mutation=None):
    """conv1 of the split forward before ReLU, and its bound.

    The kernel multiplies the exact integer frame with W1 = hi + lo quantised to three int8 digits
    under one scale s = m / 127, m = max|W1|.  From c1_digits: q = fl(w fl(127 / m)); d0 = rint(q);
    r1 = 128 (q - d0) and d1 = rint(r1), d2 = rint(128 (r1 - d1)) are exact fp32 operations, so
    q = d0 + d1/128 + d2/16384 + eps with |eps| <= (1/2)/16384: per weight the digits represent
    w (1 + 2 roundings of q) to s / 32768, the figure of the kernel's comment.  The int32 sums are
    exact; t = fma(float(i12), 2^-14, float(i0)) rounds i12 (< 2^30) and the sum, v = fma(t, c, b)
    rounds once, and the scale c = fl(fl(m fl(1/127)) fl(1/255)) carries four roundings.  With
    T = sum x|w|:
        |v - ref| <= (s / 32768) (sum_k x_k) / 255 + 12 u (T / 255 + |b|)
    (2 (3 for a division that is not correctly rounded) + 4 + 3 relative roundings, 2 spare)."""
    w = wts["w1_pk"]
    if mutation == "w1_digit3_dropped":
        d0, d1, _, m, _ = c1_digits(w)
        w = (d0 + d1 / 128.0) * (float(m) / 127.0)
    a = cols.astype(np.float64)
    b = wts["b1"].astype(np.float64)
    pre = a @ w.T / 255.0 + b
    s = float(np.abs(wts["w1_pk"]).max()) / 127.0
    T = a @ np.abs(wts["w1_pk"]).T
    return pre, (s / 32768.0) * a.sum(-1, keepdims=True) / 255.0 + 12 * U * (T / 255.0 + np.abs(b))


def layer_sp_reference(a_hi, a_lo, wts, name, b):
    """conv2 / conv3 of the split forward: three bf16 passes lo.hi + hi.lo + hi.hi over exactly the
    stored planes, 3K products exact in fp32, accumulated in fp32, the lo.lo term dropped:
        |x - ref| <= (3K + 2) u (T + |b|) + sum |a_lo||w_lo|,
    T = sum (|a_lo||w_hi| + |a_hi||w_lo| + |a_hi||w_hi|); ref multiplies (a_hi + a_lo)(w_hi + w_lo)."""
    wh, wl = wts[name + "_hi"].astype(np.float64), wts[name + "_lo"].astype(np.float64)
    ah, al = a_hi.astype(np.float64), a_lo.astype(np.float64)
    b = b.astype(np.float64)
    pre = (ah + al) @ (wh + wl).T + b
    T = np.abs(al) @ np.abs(wh).T + np.abs(ah) @ np.abs(wl).T + np.abs(ah) @ np.abs(wh).T
    K = a_hi.shape[-1]
    return pre, (3 * K + 2) * U * (T + np.abs(b)) + np.abs(al) @ np.abs(wl).T


def forward_sp_reference(geo: Geo, frames, wts, stored, stride: int = 1, mutation: Optional[str] = None):
    """{name: (relu(ref), bound)} for s1, s2, out of the split forward; ``stored`` holds the bf16
    bits of both planes of s1 and s2 (``s1``, ``s1_lo``, ...), from which conv2 and conv3 are computed."""
    n = frames.shape[0]
    if mutation == "stale_frame" and n > stride:
        frames = frames.copy()
        frames[stride:] = frames[:n - stride].copy()
    w = dict(wts)
    if mutation == "c2_khkw_swapped":
        for pl in ("_hi", "_lo"):
            w["w2" + pl] = w["w2" + pl].reshape(C, 4, 4, C).transpose(0, 2, 1, 3).reshape(C, 512)
    b2 = wts["b2"][np.arange(C) ^ 4] if mutation == "bias_wrong_half" else wts["b2"]
    p1, e1 = conv1_sp_reference(cols_conv1(geo, frames, mutation), wts, mutation)
    if mutation == "c1_last_col":
        p1 = p1.reshape(n, geo.H1, geo.W1, C).copy()
        p1[:, :, -1] = p1[:, :, -2]
        p1 = p1.reshape(n, geo.P1, C)
    if mutation == "save1_late":
        p1, e1 = np.roll(p1, 1, axis=1), np.roll(e1, 1, axis=1)
    val = lambda k: bf16_val(stored[k])  # noqa: E731
    hwc = lambda k, P: val(k).reshape(n, P, C)  # noqa: E731
    p2, e2 = layer_sp_reference(cols_hwc(hwc("s1", geo.P1), geo.H1, geo.W1, 4, 2),
                                cols_hwc(hwc("s1_lo", geo.P1), geo.H1, geo.W1, 4, 2), w, "w2", b2)
    p3, e3 = layer_sp_reference(cols_hwc(hwc("s2", geo.P2), geo.H2, geo.W2, 3, 1),
                                cols_hwc(hwc("s2_lo", geo.P2), geo.H2, geo.W2, 3, 1), w, "w3", wts["b3"])
    relu = lambda x: np.maximum(x, 0.0)  # noqa: E731
    return dict(s1=(relu(p1), e1), s2=(relu(p2), e2), out=(relu(p3).transpose(0, 2, 1), e3.transpose(0, 2, 1)))


def check_forward_sp(label, geo: Geo, frames, wts, stored, stride: int = 1, mutation=None) -> dict:
    """Both planes of s1, s2 and out: hi = bf16(x) and lo = bf16(x - hi) for some x within the bound
    of the reference (x - hi is exact in fp32).  Returns the largest use per tensor."""
    ref = forward_sp_reference(geo, frames, wts, stored, stride, mutation)
    names = dict(s1=("frame", "pixel", "channel"), s2=("frame", "pixel", "channel"), out=("frame", "channel", "pixel"))
    uses = {}
    for k, (r, e) in ref.items():
        hi_bits = np.asarray(stored[k]).reshape(r.shape)
        hi = bf16_val(hi_bits).astype(np.float64)
        uses[k] = max(compare_bf16(label, k, hi_bits, r, e, names[k]),
                      compare_bf16(label, k + "_lo", np.asarray(stored[k + "_lo"]).reshape(r.shape), r - hi, e, names[k]))
    return uses


def _planes32(v):
    hi, lo = split_planes(v.astype(np.float32))
    return bf16_bits(hi), bf16_bits(lo)


def _layer_sp32(a_hi, a_lo, wts, name, b):
    f = np.float32
    wh, wl = wts[name + "_hi"].astype(f), wts[name + "_lo"].astype(f)
    acc = (a_lo.astype(f) @ wh.T + a_hi.astype(f) @ wl.T).astype(f) + a_hi.astype(f) @ wh.T
    return _planes32(np.maximum((acc + b.astype(f)).astype(f), f(0)))


def emulate_forward_sp(geo: Geo, frames, wts) -> dict:
    """The split forward's arithmetic: digit quantisation and exact integer sums with one fp32
    combine (conv1), three fp32-accumulated passes (conv2, conv3), a hi / lo split per stored value."""
    n = frames.shape[0]
    d0, d1, d2, _, scale = c1_digits(wts["w1_pk"])
    x = cols_conv1(geo, frames).astype(np.int64)
    i0, i12 = x @ d0.T, 128 * (x @ d1.T) + x @ d2.T
    t = (i12.astype(np.float32).astype(np.float64) / 16384.0 + i0).astype(np.float32)       # one fma
    v = (t.astype(np.float64) * float(scale) + wts["b1"].astype(np.float64)).astype(np.float32)
    out = {}
    out["s1"], out["s1_lo"] = _planes32(np.maximum(v, np.float32(0)))
    a = lambda k, H, W, kk, s: cols_hwc(bf16_val(out[k]), H, W, kk, s)  # noqa: E731
    out["s2"], out["s2_lo"] = _layer_sp32(a("s1", geo.H1, geo.W1, 4, 2), a("s1_lo", geo.H1, geo.W1, 4, 2),
                                          wts, "w2", wts["b2"])
    oh, ol = _layer_sp32(a("s2", geo.H2, geo.W2, 3, 1), a("s2_lo", geo.H2, geo.W2, 3, 1), wts, "w3", wts["b3"])
    out["out"] = np.ascontiguousarray(oh.transpose(0, 2, 1)).reshape(n, C, geo.P3)
    out["out_lo"] = np.ascontiguousarray(ol.transpose(0, 2, 1)).reshape(n, C, geo.P3)
    return out


def forward_sp_operands(case: dict) -> dict:
    """As forward_operands, with split weights (``w1`` of a job: the W1 mode of make_weights_sp)."""
    geo, name = GEOMS[case["geom"]], case["name"]
    n_store = sum(j["n"] for j in case["jobs"]) + 3
    store = make_store(geo, name, n_store, 0, case.get("frames", "random"))
    jobs = []
    for i, j in enumerate(case["jobs"]):
        rows = make_rows(f"{name}/{i}", j["n"], n_store, case.get("rows", "random"))
        jobs.append(dict(n=j["n"], saves=j.get("saves", True), rows=rows,
                         wts=make_weights_sp(geo, j.get("w", "a"), j.get("w1", "random")),
                         frames=gather(geo, store, rows, j["n"])))
    return dict(geo=geo, store=store, row_bytes=store.shape[1], jobs=jobs)


# ------------------------------------------------------------------------------------------
# backward

def _convT3(g3, w3, skip=None):
    """(H3, W3, co) x W3 (co, ci, 3, 3) -> (H3 + 2, W3 + 2, ci): g2[y + kh, x + kw] += g3[y, x] W3[.., kh, kw]."""
    H3, W3 = g3.shape[:2]
    out = np.zeros((H3 + 2, W3 + 2, C), g3.dtype)
    for kh in range(3):
        for kw in range(3):
            if (kh, kw) != skip:
                out[kh:kh + H3, kw:kw + W3] += g3 @ w3[:, :, kh, kw]
    return out


def _convT2(g2, w2, H1: int, W1: int):
    """(H2, W2, co) x W2 (co, ci, 4, 4) -> (H1, W1, ci), stride 2: g1[2y + kh, 2x + kw] += g2[y, x] W2[.., kh, kw]
    (the kernel's four output phases (kh % 2, kw % 2) of two taps each way)."""
    H2, W2 = g2.shape[:2]
    out = np.zeros((H1, W1, C), g2.dtype)
    for kh in range(4):
        for kw in range(4):
            out[kh:kh + 2 * H2:2, kw:kw + 2 * W2:2] += g2 @ w2[:, :, kh, kw]
    return out


def _dw_hwc(g, a, k: int, s: int):
    """dW[co, ci, kh, kw] = sum_p g[p, co] a[s p + (kh, kw), ci]."""
    Ho, Wo = g.shape[:2]
    out = np.empty((C, C, k, k), g.dtype)
    gt = g.reshape(-1, C).T
    for kh in range(k):
        for kw in range(k):
            out[:, :, kh, kw] = gt @ a[kh:kh + s * Ho:s, kw:kw + s * Wo:s].reshape(-1, C)
    return out


def _dw1(g1, fr):
    """dW1[co, ci, kh, kw] = sum_p g1[p, co] frame[ci, 4 y + kh, 4 x + kw] (integer frame)."""
    H1, W1 = g1.shape[:2]
    out = np.empty((C, fr.shape[0], 8, 8), g1.dtype)
    gt = g1.reshape(-1, C).T
    for kh in range(8):
        for kw in range(8):
            out[:, :, kh, kw] = gt @ fr[:, kh:kh + 4 * H1:4, kw:kw + 4 * W1:4].reshape(fr.shape[0], -1).T
    return out


def _frame_inputs(geo: Geo, ops, f: int, dt):
    g3 = (ops["dx3"][f] * (ops["out3"][f] > 0)).reshape(C, geo.H3, geo.W3).transpose(1, 2, 0).astype(dt)
    a1 = ops["act1"][f].reshape(geo.H1, geo.W1, C).astype(dt)
    a2 = ops["act2"][f].reshape(geo.H2, geo.W2, C).astype(dt)
    return g3, a1, a2, ops["frames"][f].astype(dt)


def backward_frame(geo: Geo, ops, f: int, mutation: Optional[str] = None, sp: bool = False):
    """One frame's slab contribution: (value, propagated interval, T = sum |g||a|), float64 (SLAB,).

    g3 = dx3 (out3 > 0) is exact.  g2pre = convT(g3, W3) has K = 288 exact products accumulated in
    fp32: E2 = (288 + 2) u sum|g3||W3|.  The kernel stores g2 = bf16(g2pre + d), |d| <= E2, times
    the exact mask (act2 > 0), so against the unrounded oracle value
        |dg2| <= E2 + 2^-8 (|g2pre| + E2) =: D2          (a rounding flipped by d stays inside it).
    g1pre = convT_s2(g2, W2) (K = 4 taps x 32 channels) inherits sum |dg2||W2| plus its own
    (128 + 2) u sum|g2||W2| =: E1, and g1 = bf16(g1pre) (act1 > 0) gives D1 = E1 + 2^-8 (|g1pre| + E1).
    A weight gradient dW[co, k] = sum_p g[p, co] a[p, k] with exact a then carries the interval
    sum_p |dg[p, co]||a[p, k]|; its own accumulation error is added per slab row (slab_reference).
    The bias gradients are sums of the rounded g: interval sum_p |dg[p, co]|.

    Split precision (``sp``, torso_bwd_sp_kernel): every operand is a hi + lo pair (ops[name] is the
    sum, ops[name + "_lo"] the lo plane) and every product takes three passes lo.hi + hi.lo + hi.hi
    (two for the integer frame), so the accumulation terms are (3K + 2) u T, and the dropped lo.lo
    term is added: exactly where both lo planes are inputs (g3 with W3 and with act2), else through
    |g_lo| <= 2^-8 (|g| + D) for the planes the kernel makes itself.  g2 and g1 are stored as hi / lo
    pairs, which represent the fp32 value to 2^-17 (lstm_ref.forward_reference), in place of the
    bf16 rounding's 2^-8; the bias gradients sum the fp32 values *before* the split, so their
    interval is the accumulation error alone."""
    dt = np.float64
    g3, a1, a2, fr = _frame_inputs(geo, ops, f, dt)
    w2, w3 = ops["w2"].astype(dt), ops["w3"].astype(dt)
    npass, eps = (3, 2.0 ** -17) if sp else (1, EPS_BF16)
    if sp:
        lo = lambda k, shape: np.abs(ops[k + "_lo"][f].reshape(shape).astype(dt))  # noqa: E731
        on = (ops["out3"][f] > 0).reshape(C, geo.H3, geo.W3).transpose(1, 2, 0)
        g3_lo = np.abs(ops["dx3_lo"][f].reshape(C, geo.H3, geo.W3).transpose(1, 2, 0).astype(dt)) * on
        a1_lo, a2_lo = lo("act1", (geo.H1, geo.W1, C)), lo("act2", (geo.H2, geo.W2, C))
        w2_lo, w3_lo = np.abs(ops["w2_lo"].astype(dt)), np.abs(ops["w3_lo"].astype(dt))
        if mutation == "dx3_lo_dropped":
            g3 = (ops["dx3_hi"][f] * (ops["out3"][f] > 0)).reshape(C, geo.H3, geo.W3).transpose(1, 2, 0).astype(dt)
    if mutation == "s2_wrong_phase":        # tap (0, 0) and tap (0, 1) exchanged: each lands in the
        w2 = w2.copy()                      # other column phase
        w2[:, :, 0, [0, 1]] = w2[:, :, 0, [1, 0]]
    skip = (2, 2) if mutation == "c3t_corner_tap" else None
    g2pre = _convT3(g3, w3, skip)
    E2 = (npass * 288 + 2) * U * _convT3(np.abs(g3), np.abs(w3))
    if sp:
        E2 = E2 + _convT3(g3_lo, w3_lo)
    m2 = a2 > 0
    g2, D2 = g2pre * m2, (E2 + eps * (np.abs(g2pre) + E2)) * m2
    g1pre = _convT2(g2, w2, geo.H1, geo.W1)
    E1 = _convT2(D2, np.abs(w2), geo.H1, geo.W1) + (npass * 128 + 2) * U * _convT2(np.abs(g2), np.abs(w2), geo.H1, geo.W1)
    if sp:
        E1 = E1 + 2.0 ** -8 * _convT2(np.abs(g2) + D2, w2_lo, geo.H1, geo.W1)
    m1 = a1 > 0
    if mutation == "mask_neighbour":
        m1 = np.roll(m1.reshape(-1, C), 1, axis=0).reshape(m1.shape)
    g1, D1 = g1pre * m1, (E1 + eps * (np.abs(g1pre) + E1)) * m1
    B1, B2 = (E1 * m1, E2 * m2) if sp else (D1, D2)      # what the bias sums inherit
    dw3 = _dw_hwc(g3, a2, 3, 1)
    if mutation == "c3_pad_pixel_twice":    # the clamped address of a padded K-step pixel meeting a
        dw3 = dw3 + np.einsum("o,hwi->oihw", g3[-1, -1], a2[-3:, -3:])      # non-zero g3 column
    s = lambda x: x.reshape(-1, C).sum(0)  # noqa: E731
    val = pack_slab(geo, _dw1(g1, fr), _dw_hwc(g2, a1, 4, 2), dw3, s(g1),
                    s(g2pre if mutation == "db2_before_mask" else g2), s(g3))
    z = np.zeros(C)
    p2, p3 = _dw_hwc(D2, np.abs(a1), 4, 2), np.zeros((C, C, 3, 3))
    if sp:
        p2 = p2 + 2.0 ** -8 * _dw_hwc(np.abs(g2) + D2, a1_lo, 4, 2)
        p3 = _dw_hwc(g3_lo, a2_lo, 3, 1)
    prop = pack_slab(geo, _dw1(D1, fr), p2, p3, s(B1), s(B2), z)
    T = pack_slab(geo, _dw1(np.abs(g1), fr), _dw_hwc(np.abs(g2), np.abs(a1), 4, 2),
                  _dw_hwc(np.abs(g3), np.abs(a2), 3, 1), s(np.abs(g1)), s(np.abs(g2)), s(np.abs(g3)))
    return val, prop, T


def slab_terms(geo: Geo) -> np.ndarray:
    """Terms one frame adds to the fp32 accumulator of each slab element: the pixels of the layer
    padded to the kernels' K steps (dW1: 4x4 blocks), for the bias sums the same pixel counts."""
    t = np.empty(geo.SLAB)
    t[:geo.OFF_W2], t[geo.OFF_W2:geo.OFF_W3], t[geo.OFF_W3:geo.OFF_B] = 16 * geo.NB1, 16 * geo.K2S, 16 * geo.K3S
    t[geo.OFF_B:geo.OFF_B + C], t[geo.OFF_B + C:geo.OFF_B + 2 * C], t[geo.OFF_B + 2 * C:] = 16 * geo.NB1, 16 * geo.K2S, 16 * geo.K3S
    return t


def effective_grid(grid: int, n: int) -> int:
    """The launchers' clamp: grid <= 0 or grid > n runs one workgroup per frame (at most 256)."""
    return min(n, 256) if grid <= 0 or grid > n else grid


def slab_rows(geo: Geo, n: int, G: int, sp: bool) -> np.ndarray:
    """(n, SLAB) int: the slab row that holds frame f's share of each element.  Workgroup g takes the
    frames f = g (mod G); the split path's dW3 / db3 kernel (torso_dw3_sp_kernel) runs two frames
    per workgroup instead: frames 2g and 2g + 1 (mod 2G)."""
    rows = np.repeat((np.arange(n) % G)[:, None], geo.SLAB, axis=1)
    if sp:
        r3 = (np.arange(n) % (2 * G)) // 2
        rows[:, geo.OFF_W3:geo.OFF_B] = r3[:, None]
        rows[:, geo.OFF_B + 2 * C:] = r3[:, None]
    return rows


def slab_reference(geo: Geo, ops, grid: int, mutation: Optional[str] = None, sp: bool = False):
    """(ref, bound), each (G, SLAB): a slab row is the sum over its frames (slab_rows) of
    backward_frame's values, accumulated in one fp32 register across those frames:
        bound = sum_f interval_f + (m + 2) u sum_f T_f,   m = passes x frames x slab_terms (+ 16 for
    the fixed-order sums that finish the bias partials and join the dW3 kernel's two halves);
    passes = 1 (bf16), 3 (split; counted for dW1's two as well)."""
    n = ops["frames"].shape[0]
    G = effective_grid(grid, n)
    ref, prop, T, cnt = (np.zeros((G, geo.SLAB)) for _ in range(4))
    rows, col = slab_rows(geo, n, G, sp), np.arange(geo.SLAB)
    for f in range(n):
        v, p, t = backward_frame(geo, ops, f, mutation, sp)
        ref[rows[f], col] += v
        prop[rows[f], col] += p
        T[rows[f], col] += t
        cnt[rows[f], col] += 1
    m = (3 if sp else 1) * cnt * slab_terms(geo)[None, :] + 16
    return ref, prop + (m + 2) * U * T


def check_slab(label, geo: Geo, ops, grid: int, slab, mutation=None, sp: bool = False) -> float:
    ref, bound = slab_reference(geo, ops, grid, mutation, sp)
    return compare(label, "slab", np.asarray(slab).reshape(ref.shape), ref, bound, ("row", "element"))


def check_reduce(label, slab, dst, scale, grad, mutation=None) -> float:
    """grad[dst[e]] = scale[e] sum_g slab[g][e] from the *stored* slab: G - 1 fp32 additions in a
    fixed order, the product, and the representation of 1/255 in scale: (G + 2) u scale sum_g |slab|."""
    slab = np.asarray(slab, np.float64)
    sc = np.ones_like(scale, np.float64) if mutation == "no_255" else np.where(scale == 1.0, 1.0, 1.0 / 255.0)
    ref = slab.sum(0) * sc
    bound = (slab.shape[0] + 2) * U * np.abs(slab).sum(0) * sc
    return compare(label, "grad", np.asarray(grad)[dst], ref, bound, ("element",))


def emulate_backward(geo: Geo, ops, grid: int) -> np.ndarray:
    """The backward kernels' arithmetic in fp32 with bf16 roundings of g2 and g1: the slab (G, SLAB)."""
    n, dt = ops["frames"].shape[0], np.float32
    G = effective_grid(grid, n)
    slab = np.zeros((G, geo.SLAB), dt)
    w2, w3 = ops["w2"].astype(dt), ops["w3"].astype(dt)
    s = lambda x: x.reshape(-1, C).sum(0, dtype=dt)  # noqa: E731
    for f in range(n):
        g3, a1, a2, fr = _frame_inputs(geo, ops, f, dt)
        g2 = bf16_round(_convT3(g3, w3)) * (a2 > 0)
        g1 = bf16_round(_convT2(g2, w2, geo.H1, geo.W1)) * (a1 > 0)
        slab[f % G] += pack_slab(geo, _dw1(g1, fr), _dw_hwc(g2, a1, 4, 2), _dw_hwc(g3, a2, 3, 1),
                                 s(g1), s(g2), s(g3)).astype(dt)
    return slab


def emulate_reduce(slab, dst, scale, grad) -> np.ndarray:
    out = np.array(grad, np.float32)
    out[dst] = slab.astype(np.float32).sum(0, dtype=np.float32) * scale
    return out


def emulate_backward_sp(geo: Geo, ops, grid: int) -> np.ndarray:
    """The split backward's arithmetic: three fp32-accumulated passes per product (two against the
    integer frame), g2 and g1 split into hi / lo planes, the bias sums taken before the split."""
    n, dt = ops["frames"].shape[0], np.float32
    G = effective_grid(grid, n)
    slab = np.zeros((G, geo.SLAB), dt)
    rows, col = slab_rows(geo, n, G, True), np.arange(geo.SLAB)
    pl = lambda k: (ops[k + "_hi"].astype(dt), ops[k + "_lo"].astype(dt))  # noqa: E731
    (w2h, w2l), (w3h, w3l) = pl("w2"), pl("w3")
    s = lambda x: x.reshape(-1, C).sum(0, dtype=dt)  # noqa: E731
    x3 = lambda fn, ah, al, bh, bl, *a: ((fn(al, bh, *a) + fn(ah, bl, *a)).astype(dt) + fn(ah, bh, *a)).astype(dt)  # noqa: E731
    for f in range(n):
        on = (ops["out3"][f] > 0).reshape(C, geo.H3, geo.W3).transpose(1, 2, 0)
        hwc3 = lambda v: v[f].reshape(C, geo.H3, geo.W3).transpose(1, 2, 0).astype(dt) * on  # noqa: E731
        g3h, g3l = hwc3(ops["dx3_hi"]), hwc3(ops["dx3_lo"])
        a1h, a1l = (ops["act1" + k][f].reshape(geo.H1, geo.W1, C).astype(dt) for k in ("_hi", "_lo"))
        a2h, a2l = (ops["act2" + k][f].reshape(geo.H2, geo.W2, C).astype(dt) for k in ("_hi", "_lo"))
        fr = ops["frames"][f].astype(dt)
        g2 = x3(_convT3, g3h, g3l, w3h, w3l) * (a2h > 0)
        g2h, g2l = split_planes(g2)
        g1 = x3(_convT2, g2h, g2l, w2h, w2l, geo.H1, geo.W1) * (a1h > 0)
        g1h, g1l = split_planes(g1)
        v = pack_slab(geo, (_dw1(g1l, fr) + _dw1(g1h, fr)).astype(dt), x3(_dw_hwc, g2h, g2l, a1h, a1l, 4, 2),
                      x3(_dw_hwc, g3h, g3l, a2h, a2l, 3, 1), s(g1), s(g2), s((g3h + g3l).astype(dt))).astype(dt)
        slab[rows[f], col] += v
    return slab


def backward_sp_operands(case: dict) -> dict:
    """backward_operands with fp32 act1 / act2 / dx3 / W2 / W3 carried as hi / lo planes (the masks
    are unchanged: a plane pair is zero exactly where the value is); out3 stays one bf16 plane."""
    ops = backward_operands(case)
    geo, r = ops["geo"], _rng("bsp/" + case["name"])
    for k in ("act1", "act2", "dx3"):
        v = (ops[k] * (1.0 + 2.0 ** -9 * r.uniform(-1, 1, ops[k].shape))).astype(np.float32)
        hi, lo = split_planes(v)
        ops[k + "_hi"], ops[k + "_lo"], ops[k] = hi, lo, hi.astype(np.float64) + lo
    wts = make_weights_sp(geo, "bwd")
    for k in ("w2", "w3"):
        hi, lo = split_planes(wts[k])
        ops[k + "_hi"], ops[k + "_lo"], ops[k] = hi, lo, hi.astype(np.float64) + lo
    for k, pk in (("w3", pack_conv3_dg), ("w2", pack_conv2_dg)):
        ops[k + "_dg"], ops[k + "_dg_lo"] = pk(ops[k + "_hi"]), pk(ops[k + "_lo"])
    return ops


def grad_layout(geo: Geo, head: int = 40, tail: int = 24):
    """A flat gradient of the test: ``head`` foreign elements, the six torso tensors in torch order
    (w1, b1, w2, b2, w3, b3), ``tail`` foreign elements.  Returns (numel, offsets)."""
    off, cur = {}, head
    for name, size in (("w1", C * geo.K1), ("b1", C), ("w2", C * 512), ("b2", C), ("w3", C * 288), ("b3", C)):
        off[name] = cur
        cur += size
    return cur + tail, off


def backward_operands(case: dict) -> dict:
    """Free operands of a backward case: nothing here comes from a forward pass."""
    geo, n, name = GEOMS[case["geom"]], case["n"], case["name"]
    r = _rng("b/" + name)
    wts = make_weights(geo, "bwd/" + case["geom"])
    store = make_store(geo, name, n + 3, case.get("row_pad", 0), case.get("frames", "random"))
    rows = make_rows(name, n, n + 3, "random")

    def act(P, H, W):
        v = bf16_round(np.abs(r.standard_normal((n, P, C))) + 0.01)
        mode = case.get("masks", "random")
        if mode == "random":
            v = v * (r.random((n, P, C)) < 0.5)
        elif mode == "checker":
            y, x = np.divmod(np.arange(P), W)
            v = v * (((y + x)[None, :, None] + np.arange(C)[None, None, :] + np.arange(n)[:, None, None]) % 2 == 0)
        return v.astype(np.float32)

    act1, act2 = act(geo.P1, geo.H1, geo.W1), act(geo.P2, geo.H2, geo.W2)
    out3 = act(geo.P3, geo.H3, geo.W3).transpose(0, 2, 1).reshape(n, geo.OUT).copy()
    hot = case.get("onehot")
    if hot is None:
        dx3 = bf16_round(r.standard_normal((n, geo.OUT)))
    else:           # one conv3 pixel, every channel: the transposed convolutions' border paths
        y, x = {"tl": (0, 0), "tr": (0, geo.W3 - 1), "bl": (geo.H3 - 1, 0), "br": (geo.H3 - 1, geo.W3 - 1),
                "c": (geo.H3 // 2, geo.W3 // 2)}[hot]
        dx3 = np.zeros((n, C, geo.H3, geo.W3), np.float32)
        dx3[:, :, y, x] = bf16_round(r.standard_normal((n, C)) + 2.0)
        dx3 = dx3.reshape(n, geo.OUT)
    numel, off = grad_layout(geo)
    dst, scale = slab_map(geo, off)
    return dict(geo=geo, store=store, rows=rows, row_bytes=store.shape[1], frames=gather(geo, store, rows, n),
                act1=act1, act2=act2, out3=out3, dx3=dx3.astype(np.float32), w2=wts["w2"], w3=wts["w3"],
                w3_dg=wts["w3_dg"], w2_dg=wts["w2_dg"], dst=dst, scale=scale, grad_numel=numel)


def forward_operands(case: dict) -> dict:
    """The replay store and, per job, rows / weights / gathered frames of a forward case."""
    geo, name = GEOMS[case["geom"]], case["name"]
    total = sum(j["n"] for j in case["jobs"])
    n_store = total + 3
    store = make_store(geo, name, n_store, case.get("row_pad", 0), case.get("frames", "random"))
    jobs = []
    for i, j in enumerate(case["jobs"]):
        rows = make_rows(f"{name}/{i}", j["n"], n_store, case.get("rows", "random"))
        jobs.append(dict(n=j["n"], saves=j.get("saves", True), rows=rows, wts=make_weights(geo, j.get("w", "a")),
                         frames=gather(geo, store, rows, j["n"])))
    return dict(geo=geo, store=store, row_bytes=store.shape[1], jobs=jobs)


def forward_strides(case: dict):
    """Per job of the case: its worker count (the frame stride of its workgroups), 0 for a job
    without frames."""
    res = case.get("reserve", (0, 0))
    nw = reserve_workers(*res) if res[1] > 0 else (case["grid"] if case["grid"] > 0 else 256)
    out = [0] * len(case["jobs"])
    for j, _, cnt in deal_workers([j["n"] for j in case["jobs"]], nw):
        out[j] = cnt
    return out


# ------------------------------------------------------------------------------------------
# case tables (shared by the CPU and the GPU tests)

def _fwd_cases():
    out = []
    for g in GEOMS:
        one = lambda name, n, grid, **kw: out.append(dict(name=f"{g}/{name}", geom=g, grid=grid,  # noqa: E731
                                                          jobs=[dict(n=n)], **kw))
        for n, grid in ((1, 1), (2, 2), (3, 2), (5, 2), (3, 8)):    # no loop; prefetch edge true and
            one(f"n{n}g{grid}", n, grid)                            # false; row_nn used; grid > frames
        one("rows_dup_desc", 3, 2, rows="dup_desc")
        one("rows_null", 3, 2, rows="null")
        one("rows_identity", 3, 2, rows="identity")
        one("row_pad16", 3, 2, row_pad=16)
        one("row_pad64", 3, 2, row_pad=64)
        one("frames_zeros", 2, 2, frames="zeros")
        one("frames_full", 2, 2, frames="full")
        multi = lambda name, grid, jobs, **kw: out.append(dict(name=f"{g}/{name}", geom=g, grid=grid,  # noqa: E731
                                                               jobs=jobs, **kw))
        multi("two_jobs", 4, [dict(n=3, w="a"), dict(n=2, w="b", saves=False)])
        multi("four_jobs", 4, [dict(n=1, w=w) for w in "abcd"])
        multi("zero_mid", 4, [dict(n=2, w="a"), dict(n=0, w="b"), dict(n=2, w="c")])
        multi("reserve", 256, [dict(n=4, w="a"), dict(n=3, w="b")], reserve=(2, 4))
    return out


def _bwd_cases():
    out = []
    for g in GEOMS:
        add = lambda name, n, grid, **kw: out.append(dict(name=f"{g}/{name}", geom=g, n=n, grid=grid, **kw))  # noqa: E731
        for n, grid in ((1, 1), (2, 2), (3, 2), (5, 2), (3, 3), (3, 0), (3, 9)):
            add(f"n{n}g{grid}", n, grid)
        add("open", 2, 2, masks="open")
        for hot in ("tl", "tr", "bl", "br", "c"):
            add(f"onehot_{hot}", 1, 1, masks="open", onehot=hot)
        add("checker", 2, 1, masks="checker")
        add("frames_zeros", 2, 2, frames="zeros")
        add("frames_full", 2, 2, frames="full", row_pad=16)
    return out


def _sp_cases():
    """The forward table on the Atari geometry, less what r2_torso_fwd_sp_multi has no argument for
    (row stride, reserve), plus the W1 edges."""
    out = [dict(c, name="sp/" + c["name"]) for c in _fwd_cases()
           if c["geom"] == "atari" and "row_pad" not in c and "reserve" not in c]
    out.append(dict(name="sp/atari/w1_outlier", geom="atari", grid=2, jobs=[dict(n=2, w1="outlier")]))
    out.append(dict(name="sp/atari/w1_zero", geom="atari", grid=2, jobs=[dict(n=2, w1="zero")]))
    return out


FWD_CASES = _fwd_cases()
SP_CASES = _sp_cases()
BWD_CASES = _bwd_cases()
# (r2_torso_bwd_sp has no row stride argument: replay rows are exactly one frame)
SP_BWD_CASES = [dict(c, name="sp/" + c["name"], row_pad=0) for c in BWD_CASES if c["geom"] == "atari"]
