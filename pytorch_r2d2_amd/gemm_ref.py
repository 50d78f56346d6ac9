"""Float64 oracle of the dense GEMM kernels (csrc/kernels/gemm.hip, gemm_sp.hip, csrc/gemm_tile.h).

Pure host code (numpy, no torch, no GPU).  Contents: the contract, the per-element bound, the
comparison (``check_problem``: write ownership, bound or bit identity, split output planes), an
fp32 / bf16 emulation of the kernels' arithmetic with named mutations (``emulate``,
``MUTATIONS``), and the case table ``CASES`` that tests/test_gemm_ref_cpu.py and
tests/test_gemm_oracle_gpu.py share.

Contract.  Operands enter as bf16 planes with given bits (nothing is split on the device); the
reference is computed in float64 from their exact values:

    ref[crow[m]][n] = alpha * P[m][n] + bias[n] (+ C_old[crow[m]][n])

    P = A.B                                  plain operands           (mode "hh")
    P = A_lo.B_hi + A_hi.B_lo + A_hi.B_hi    both operands split      (mode "x3", csrc/split.h)
    P = A_lo.B + A_hi.B                      only A split             (mode "a")
    P = A.B_lo + A.B_hi                      only B split             (mode "b")

The lo.lo term that the split product drops belongs to the number format, not to a kernel: it is
left out of the reference too, so the bound below measures arithmetic only.

Bound.  A product of two bf16 values has 16 significant bits and is exact in fp32.  The kernels
sum n_add of them (K per pass; 3K, 2K or K in all) in fp32 in some order: whatever the order (MFMA
blocks of 16 or 32, K tiles, passes, K-split partial tiles summed by the last arriver), every
product passes through at most n_add - 1 additions, each of relative error u = 2^-24, so with
S = sum |a||b| over all products taken the accumulator is off by at most (n_add - 1) u S to first
order.  alpha, the bias and the accumulate each add one rounding of a value of magnitude at most
|alpha| S + |bias| + |C_old|.  As in lstm_ref.py's MFMA sums, (n + 2) u (S + |x|), two more units
absorb the second-order terms (n u << 1 here: n <= 768), and one unit is counted for the K-split
partial sums, which the table runs on the same cases:

    bound = (n_add + c) u (|alpha| S + |bias| + |C_old|),  c = 3 + [alpha != 1] + [bias] + [accumulate]

The internal adder of the bf16 matrix instruction is not documented as correctly rounded; the
bound's slack against a sum in round-to-nearest is its factor n_add against the typical
sqrt(n_add).  The uses measured on the GPU are committed in profiles/gemm_oracle_errors.txt.

Exact cases (``data == "int"``): both planes hold integers of magnitude <= 8 and K <= 256, alpha
is a power of two, bias and C_old are small integers: every partial sum in every order is an
integer below 2^24, so fp32 output equals the oracle bit for bit, and bf16 / split output equals
its rounding bit for bit, on every kernel and every K split.

Cancellation cases (``data == "cancel"``): rows of +-x pairs with exponents from 2^-6 to 2^6, so
|C| << S; the bound stays relative to S, and a missing cross term of the split product (2^-9 of S)
cannot hide behind it.

Operand geometry: every operand has a leading dimension larger than its extent and the gap holds
NaN, so a read past K (or past M / N of an mn-major operand) that reaches an MFMA poisons a named
element (0 * NaN = NaN).  Outputs are NaN poison outside the elements the problem owns.
"""
from __future__ import annotations

import zlib
from typing import Optional

import numpy as np

from .refnum import (bf16_bits, bf16_round, bf16_val, bits_equal, check_ownership, compare,
                     compare_bf16, split_planes)

U = 2.0 ** -24
TILE_ROWS, TILE_COLS, TILE_K = (128, 192, 256), (64, 128, 256), (32, 64)
# the tiles the kernels cut a problem into: gemm / gemm2 / gemm3 / group 128 x 128, gemm4 256 x 256
# and 256 x 128, the split GEMM's configurations
TILINGS = ((128, 128), (256, 256), (256, 128), (192, 128), (256, 64), (128, 64), (192, 256))
NAN16 = np.uint16(0x7FC0)
EMU_PAD = 1024              # guard elements of the emulation's output buffers

MODES = ("hh", "x3", "a", "b")
# deliberately wrong variants of the emulation (tests only): a check that accepts one tests nothing
MUTATIONS = {
    "k_tail_dropped": "the K tile that K does not fill is not multiplied",
    "k_tail_from_gap": "the K tail is read past K from the operand's leading-dimension gap",
    "cross_term_dropped": "the split product without A_lo.B_hi",
    "alpha_after_bias": "alpha (acc + bias)",
    "accumulate_ignored": "C = v where C += v was asked for",
    "accumulate_bf16_narrow": "bf16 output: v rounded to bf16 before C_old is added",
    "crow_inverse": "the row map applied as its inverse",
    "vec_store_across_n": "the 4-column chunk that straddles N stored whole",
    "edge_rows_stored": "the tile's row M stored as row M of C",
    "lo_from_truncated": "split output: lo taken from v minus its truncation while hi is rounded",
    "k_chunks_swapped": "two 8-element k chunks exchanged in A only",
    "partial_twice": "K split: the first partial sum counted twice",
    "partial_missing": "K split: the last partial sum not counted",
}


# ------------------------------------------------------------------------------------------
# the case table

def _p(M, N, K, out="f32", alpha=1.0, bias=False, acc=False, crow="none", ga=8, gb=8, gc=0, coff=0):
    """One problem.  out: f32 / bf16 / split; crow: none / id / perm / inject (into M + 5 rows);
    ga / gb: elements by which lda / ldb exceed the extent (multiples of 8); gc: ldc - N; coff:
    elements by which the base of C (and C_lo) is offset from a 16-byte boundary."""
    assert out in ("f32", "bf16", "split") and not (out == "split" and acc)
    assert crow in ("none", "id", "perm", "inject") and ga % 8 == 0 and gb % 8 == 0
    return dict(M=M, N=N, K=K, out=out, alpha=alpha, bias=bias, acc=acc, crow=crow, ga=ga, gb=gb,
                gc=gc, coff=coff)


def _c(name, probs, data="rand", splits=None):
    """splits: the K split of each problem on the kernels that split K (one of them larger than the
    number of K tiles where the case says so); default 2, 3, 2, 3."""
    probs = list(probs)
    return dict(name=name, probs=probs, data=data, splits=list(splits or [2, 3, 2, 3][:len(probs)]))


CASES = [
    # ---- one problem: the M / N / K edges, each with another epilogue
    _c("m1n1k8", [_p(1, 1, 8, coff=1)], splits=[3]),                      # 3 splits of 1 K tile
    _c("m8n8k24", [_p(8, 8, 24, out="bf16", bias=True, gc=3)]),
    _c("m16n50k40", [_p(16, 50, 40, bias=True, alpha=0.5, gc=1, crow="inject")]),
    _c("m56n130k72", [_p(56, 130, 72, acc=True, gc=2, crow="perm")]),     # vec store, col + 4 > N
    _c("m120n257k136", [_p(120, 257, 136, out="bf16", acc=True, gc=3, alpha=-2.0)]),
    _c("m128n128k64", [_p(128, 128, 64, alpha=0.5, bias=True, crow="perm")], splits=[4]),
    _c("m136n136k128", [_p(136, 136, 128, out="split", bias=True, gc=4)]),
    _c("m184n56k32", [_p(184, 56, 32, out="bf16", coff=1, crow="id")], splits=[2]),
    _c("m192n64k96", [_p(192, 64, 96, acc=True, bias=True, alpha=0.25)]),
    _c("m200n72k200", [_p(200, 72, 200, out="split", coff=1, gc=1, crow="inject")]),
    _c("m248n120k256", [_p(248, 120, 256, bias=True, ga=16, gb=24)], splits=[5]),
    _c("m256n256k64", [_p(256, 256, 64, out="bf16", bias=True, alpha=2.0)], splits=[2]),
    _c("m264n248k24", [_p(264, 248, 24, acc=True, coff=1, gc=5)]),
    _c("m392n392k256", [_p(392, 392, 256, crow="perm", gc=8)], splits=[3]),
    _c("m392n8k8", [_p(392, 8, 8, out="split", crow="inject")]),
    _c("m8n392k128", [_p(8, 392, 128, out="bf16", acc=True, bias=True, gc=4)], splits=[2]),
    _c("m1n257k64", [_p(1, 257, 64, bias=True, gc=3)], splits=[2]),
    _c("m200n1k96", [_p(200, 1, 96, out="bf16", gc=2, coff=1)]),
    _c("m16n16k192", [_p(16, 16, 192, out="split")], splits=[3]),        # acting: M below one tile
    _c("m56n50k64", [_p(56, 50, 64, out="split", bias=True, gc=2)]),      # split output, col + 4 > N
    # ---- several problems per launch, different shapes and epilogues
    _c("two_k64", [_p(136, 200, 64, bias=True, crow="perm"), _p(56, 264, 128, out="bf16", acc=True)],
       splits=[2, 1]),
    _c("three_mixed", [_p(120, 136, 40, coff=1), _p(264, 8, 72, out="bf16", bias=True, gc=1),
                       _p(16, 120, 8, acc=True, alpha=0.5, crow="inject")]),
    _c("four_k64", [_p(128, 256, 64, out="split"), _p(8, 8, 128, acc=True), _p(392, 56, 192, bias=True, gc=4),
                    _p(200, 136, 64, out="bf16", crow="id", coff=1)], splits=[1, 3, 2, 2]),
    _c("four_tails", [_p(1, 50, 24), _p(184, 130, 136, out="bf16", gc=2), _p(256, 1, 40, bias=True),
                      _p(120, 257, 200, acc=True, crow="perm", gc=3)], splits=[2, 3, 1, 4]),
    # (tile counts 6, 7 and 8 of the 256 x 256 kernel, 15, 16 and 21 of the 128 x 128 ones)
    _c("tiles6", [_p(392, 264, 64, bias=True, gc=4), _p(264, 120, 64, out="bf16", crow="perm")], splits=[2, 1]),
    _c("tiles7", [_p(392, 264, 40, acc=True), _p(264, 8, 8, out="bf16", gc=1), _p(8, 8, 24, alpha=2.0)]),
    _c("m392n264k72", [_p(392, 264, 72, bias=True, alpha=-0.5, gc=2)]),
    _c("tiles8", [_p(392, 264, 128, out="bf16", acc=True, coff=1), _p(264, 264, 64, crow="inject")],
       splits=[3, 2]),
    # ---- bound-free: integer planes, every sum exact
    _c("int_m1n1k8", [_p(1, 1, 8, alpha=2.0, bias=True)], data="int", splits=[2]),
    _c("int_m136n130k40", [_p(136, 130, 40, alpha=0.5, bias=True, acc=True, gc=2, crow="perm")], data="int"),
    _c("int_m200n264k256", [_p(200, 264, 256, alpha=-4.0, bias=True, coff=1)], data="int", splits=[3]),
    _c("int_m264n72k64_bf16", [_p(264, 72, 64, out="bf16", acc=True, bias=True, gc=4)], data="int", splits=[2]),
    _c("int_m120n200k128_split", [_p(120, 200, 128, out="split", bias=True, alpha=2.0, crow="inject")],
       data="int", splits=[5]),
    _c("int_three", [_p(256, 128, 192, acc=True), _p(56, 56, 64, out="split", coff=1),
                     _p(8, 392, 128, out="bf16", alpha=0.125, crow="id")], data="int", splits=[2, 2, 3]),
    _c("int_tails", [_p(16, 257, 72, out="bf16", gc=3), _p(392, 16, 24, acc=True, alpha=0.5)], data="int"),
    # ---- cancellation: |C| << S
    _c("cancel_m136n72k256", [_p(136, 72, 256, bias=True)], data="cancel", splits=[4]),
    _c("cancel_m56n130k40", [_p(56, 130, 40, acc=True, gc=2)], data="cancel"),
    _c("cancel_two", [_p(264, 136, 128, out="split"), _p(120, 8, 64, alpha=0.5, crow="perm")],
       data="cancel", splits=[2, 2]),
]
CASE_BY_NAME = {c["name"]: c for c in CASES}


def tiles(case, bm, bn) -> int:
    return sum(-(-p["M"] // bm) * -(-p["N"] // bn) for p in case["probs"])


def layout_ok(p, ak, bk) -> bool:
    """mn-major operands need an extent that is a multiple of 8."""
    return (ak or p["M"] % 8 == 0) and (bk or p["N"] % 8 == 0)


def m_out(p) -> int:
    return p["M"] + 5 if p["crow"] == "inject" else p["M"]


def ldc(p) -> int:
    return p["N"] + p["gc"]


# ------------------------------------------------------------------------------------------
# operands

def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def make_problem(case, pi) -> dict:
    """The operands of problem ``pi`` of ``case`` by value: a_hi, a_lo (M, K), b_hi, b_lo (K, N) as
    fp32 arrays exact in bf16, bias (N) fp32 or None, crow (M) int32 or None, c_old (M, N) values
    at the owned elements (exact in the output type) or None."""
    p = case["probs"][pi]
    M, N, K = p["M"], p["N"], p["K"]
    r = _rng("%s/%d" % (case["name"], pi))
    data = case["data"]
    if data == "int":
        a_hi, a_lo, b_hi, b_lo = (r.integers(-8, 9, size=s).astype(np.float32)
                                  for s in ((M, K), (M, K), (K, N), (K, N)))
        bias = r.integers(-64, 65, size=N).astype(np.float32)
        c_old = r.integers(-64, 65, size=(M, N)).astype(np.float32)
    else:
        if data == "cancel":
            # A_hi: +-x pairs against nearly equal positive pairs of B_hi, so A_hi.B_hi cancels to
            # about 2^-6 of its S; the lo planes are given bits of their own (2^-9 of the hi
            # plane's magnitude, A_lo positive), so the cross term A_lo.B_hi does not cancel
            h = K // 2
            x = np.ldexp(1.0 + r.random((M, h)), r.integers(-6, 7, size=(M, h))) * r.choice([-1.0, 1.0], (M, h))
            a = np.empty((M, K))
            a[:, 0::2], a[:, 1::2] = x, -x
            y = np.ldexp(1.0 + r.random((h, N)), r.integers(-6, 7, size=(h, N)))
            b = np.empty((K, N))
            b[0::2], b[1::2] = y, y * (1.0 + 2.0 ** -6 * r.standard_normal((h, N)))
            a_hi, b_hi = bf16_round(a.astype(np.float32)), bf16_round(b.astype(np.float32))
            a_lo = bf16_round((np.abs(a_hi) * 2.0 ** -9 * (0.5 + 0.5 * r.random((M, K)))).astype(np.float32))
            b_lo = bf16_round((b_hi * 2.0 ** -9 * r.uniform(-1, 1, (K, N))).astype(np.float32))
        else:
            a, b = r.standard_normal((M, K)), r.standard_normal((K, N))
            a_hi, a_lo = split_planes(a.astype(np.float32))
            b_hi, b_lo = split_planes(b.astype(np.float32))
        bias = r.standard_normal(N).astype(np.float32)
        c_old = (3.0 * r.standard_normal((M, N))).astype(np.float32)
    if p["out"] != "f32":
        c_old = bf16_round(c_old)
    crow = None
    if p["crow"] == "id":
        crow = np.arange(M, dtype=np.int32)
    elif p["crow"] == "perm":
        crow = r.permutation(M).astype(np.int32)
    elif p["crow"] == "inject":
        crow = np.sort(r.permutation(M + 5)[:M]).astype(np.int32)
        if M > 1:
            crow[[0, M - 1]] = crow[[M - 1, 0]]
    return dict(p=p, label="%s/%d" % (case["name"], pi), exact=data == "int", a_hi=a_hi, a_lo=a_lo,
                b_hi=b_hi, b_lo=b_lo, bias=bias if p["bias"] else None, crow=crow,
                c_old=c_old if p["acc"] else None)


def lay_operand(x, kmajor: bool, gap: int):
    """bf16 bits of X[i][k] (values exact in bf16) laid out k-major (X[i][k] at i * ld + k) or
    mn-major (at k * ld + i) with ``gap`` NaN elements at the end of every row.  Returns (flat
    uint16 array, ld)."""
    v = bf16_bits(x if kmajor else x.T)
    full = np.full((v.shape[0], v.shape[1] + gap), NAN16, dtype=np.uint16)
    full[:, :v.shape[1]] = v
    return full.reshape(-1), v.shape[1] + gap


def rows_of(pd) -> np.ndarray:
    return pd["crow"].astype(np.int64) if pd["crow"] is not None else np.arange(pd["p"]["M"])


def owned_mask(pd) -> np.ndarray:
    """(coff + M_out * ldc) bools: the elements of the output body the problem writes."""
    p = pd["p"]
    v = np.zeros((m_out(p), ldc(p)), bool)
    v[rows_of(pd), :p["N"]] = True
    return np.concatenate([np.zeros(p["coff"], bool), v.reshape(-1)])


def initial_body(pd) -> np.ndarray:
    """The output body before the launch (fp32 values): NaN poison, C_old at the owned elements of
    an accumulating problem."""
    p = pd["p"]
    body = np.full((m_out(p), ldc(p)), np.nan, dtype=np.float32)
    if pd["c_old"] is not None:
        body[rows_of(pd), :p["N"]] = pd["c_old"]
    return np.concatenate([np.full(p["coff"], np.nan, np.float32), body.reshape(-1)])


# ------------------------------------------------------------------------------------------
# reference and bound

def products(pd, mode, mutation: Optional[str] = None):
    """The (A plane, B plane) pairs the mode multiplies, small terms first."""
    ah, al, bh, bl = pd["a_hi"], pd["a_lo"], pd["b_hi"], pd["b_lo"]
    out = {"hh": [(ah, bh)], "x3": [(al, bh), (ah, bl), (ah, bh)], "a": [(al, bh), (ah, bh)],
           "b": [(ah, bl), (ah, bh)]}[mode]
    if mutation == "cross_term_dropped" and len(out) > 1:
        out = out[1:]
    return out


_REF = {}


def reference(pd, mode):
    """(ref, bound): (M, N) float64, by product row (row m is stored at crow[m]).  Cached: the
    kernel variants share it."""
    key = (pd["label"], mode)
    if key not in _REF:
        p = pd["p"]
        P = np.zeros((p["M"], p["N"]))
        S = np.zeros((p["M"], p["N"]))
        pr = products(pd, mode)
        for a, b in pr:
            P += a.astype(np.float64) @ b.astype(np.float64)
            S += np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64)
        ref = p["alpha"] * P
        mag = abs(p["alpha"]) * S
        c = 3 + (p["alpha"] != 1.0)
        if pd["bias"] is not None:
            ref, mag, c = ref + pd["bias"].astype(np.float64), mag + np.abs(pd["bias"]), c + 1
        if pd["c_old"] is not None:
            ref, mag, c = ref + pd["c_old"].astype(np.float64), mag + np.abs(pd["c_old"]), c + 1
        bound = (len(pr) * p["K"] + c) * U * mag
        _REF[key] = (ref + 0.0, bound)
    return _REF[key]


# ------------------------------------------------------------------------------------------
# comparison

def check_problem(pd, mode, full, pad, full_lo=None, label=""):
    """Everything one launch must have left in the output of one problem.  ``full``: the output
    buffer as fp32 values (bf16 output widened), ``pad`` guard elements at each end of it, NaN
    poison before the launch except C_old; ``full_lo``: the lo plane's buffer (split output).
    Ownership first (guards, the offset before C, the ldc gap, rows outside crow's image), then every
    element against its bound, bit for bit in the exact cases.  Returns the largest use."""
    p = pd["p"]
    label = "%s %s [%s]" % (label, pd["label"], mode)
    M, N = p["M"], p["N"]
    valid = owned_mask(pd)
    names = ("m", "n")

    def view(f, what):
        f = np.asarray(f, np.float32).reshape(-1)
        assert f.size == valid.size + 2 * pad, (label, f.size, valid.size, pad)
        check_ownership(label, what, f, pad, valid)
        body = f[pad + p["coff"]: f.size - pad].reshape(m_out(p), ldc(p))
        return body[rows_of(pd), :N]

    got = view(full, "C")
    ref, bound = reference(pd, mode)
    if p["out"] == "f32":
        if pd["exact"]:
            bits_equal(label, "C", got.view(np.uint32), ref.astype(np.float32).view(np.uint32), names)
            return 0.0
        return compare(label, "C", got, ref, bound, names)
    hi_bits = bf16_bits(got)
    if p["out"] == "bf16":
        if pd["exact"]:
            bits_equal(label, "C", hi_bits, bf16_bits(ref.astype(np.float32)), names)
            return 0.0
        return compare_bf16(label, "C", hi_bits, ref, bound, names)
    lo = view(full_lo, "C_lo")
    lo_bits = bf16_bits(lo)
    if pd["exact"]:      # v = ref exactly: hi = bf16(v), lo = bf16(v - hi)
        v = ref.astype(np.float32)
        bits_equal(label, "C", hi_bits, bf16_bits(v), names)
        bits_equal(label, "C_lo vs bf16(v - hi)", lo_bits, bf16_bits((v - bf16_round(v)).astype(np.float32)), names)
        return 0.0
    # hi = bf16(v) and lo = bf16(v - hi) for some v within the bound of the reference (v - hi is exact)
    return max(compare_bf16(label, "C", hi_bits, ref, bound, names),
               compare_bf16(label, "C_lo", lo_bits, ref - got.astype(np.float64), bound, names))


def check_split_of(label, c32, hi_bits, lo_bits):
    """Bound-free: the planes of a split output are the split of the fp32 output that the same
    kernel gives for the same problem: hi == bf16(v), lo == bf16(v - hi)."""
    v = np.asarray(c32, np.float32)
    bits_equal(label, "C vs bf16(C32)", hi_bits, bf16_bits(v), ("m", "n"))
    bits_equal(label, "C_lo vs bf16(C32 - C)", lo_bits, bf16_bits((v - bf16_round(v)).astype(np.float32)),
               ("m", "n"))


# ------------------------------------------------------------------------------------------
# fp32 / bf16 emulation of the kernels' arithmetic

def _trunc_bf16(x):
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def emulate(pd, mode, split: int = 1, order: int = 0, bk: int = 32, mutation: Optional[str] = None):
    """One problem as the kernels compute it: fp32 accumulation of exact bf16 products in K tiles
    of ``bk``, the K tiles dealt to ``split`` partial sums that are added in split order, then the
    epilogue in fp32 and the store into a poisoned buffer.  order 0: K tiles ascending and the
    products of a tile together (the split GEMM); order 1: one pass over K per product, K tiles
    descending (the multi-pass kernels read them ascending: any order is allowed).  Returns
    dict(full, full_lo or None, pad)."""
    p = pd["p"]
    M, N, K = p["M"], p["N"], p["K"]
    f32 = np.float32
    pr = [(a.astype(f32), b.astype(f32)) for a, b in products(pd, mode, mutation)]
    if mutation == "k_chunks_swapped" and K >= 16:
        sw = np.arange(K)
        sw[:8], sw[8:16] = np.arange(8, 16), np.arange(8)
        pr = [(a[:, sw], b) for a, b in pr]
    nk = -(-K // bk)
    kend = K
    if mutation == "k_tail_dropped":
        nk, kend = K // bk, K // bk * bk
    if mutation == "k_tail_from_gap" and K % bk:   # the gap of A holds NaN; B's rows past K whatever
        kend = nk * bk
        pr = [(np.concatenate([a, np.full((M, kend - K), np.nan, f32)], 1),
               np.concatenate([b, np.ones((kend - K, N), f32)], 0)) for a, b in pr]
    per = -(-nk // split) if nk else 0
    partial = []
    for s in range(split):
        kt0, kt1 = min(nk, s * per), min(nk, s * per + per)
        acc = np.zeros((M, N), f32)
        kts = list(range(kt0, kt1))
        with np.errstate(invalid="ignore"):
            if order == 0:
                for kt in kts:
                    sl = slice(kt * bk, min(kend, kt * bk + bk))
                    for a, b in pr:
                        acc = acc + a[:, sl] @ b[sl]
            else:
                for a, b in pr:
                    for kt in reversed(kts):
                        sl = slice(kt * bk, min(kend, kt * bk + bk))
                        acc = acc + a[:, sl] @ b[sl]
        partial.append(acc)
    if mutation == "partial_twice" and split > 1:
        partial.append(partial[0])
    if mutation == "partial_missing" and split > 1:
        partial = partial[:-1]
    acc = np.zeros((M, N), f32)
    with np.errstate(invalid="ignore"):
        for x in partial:
            acc = acc + x
        bias = pd["bias"] if pd["bias"] is not None else f32(0)
        if mutation == "alpha_after_bias":
            v = (f32(p["alpha"]) * (acc + bias)).astype(f32)
        else:
            v = (f32(p["alpha"]) * acc + bias).astype(f32)
    rows = rows_of(pd)
    if mutation == "crow_inverse" and p["crow"] == "perm":
        rows = np.argsort(rows)
    body = initial_body(pd)
    body_lo = body.copy() if p["out"] == "split" else None
    ld, coff = ldc(p), p["coff"]
    C = body[coff:].reshape(m_out(p), ld)
    with np.errstate(invalid="ignore"):
        if p["acc"] and mutation != "accumulate_ignored":
            old = C[rows, :N]
            if p["out"] == "bf16" and mutation == "accumulate_bf16_narrow":
                v = bf16_round(v) + old
            else:
                v = (old + v).astype(f32)
    hi = v if p["out"] == "f32" else bf16_round(v)
    C[rows, :N] = hi
    if body_lo is not None:
        base = _trunc_bf16(v) if mutation == "lo_from_truncated" else hi
        body_lo[coff:].reshape(m_out(p), ld)[rows, :N] = bf16_round((v - base).astype(f32))
    full = np.concatenate([np.full(EMU_PAD, np.nan, f32), body, np.full(EMU_PAD, np.nan, f32)])
    if mutation == "vec_store_across_n" and N % 4:       # the last 4-column chunk stored whole
        for m in range(M):
            o = EMU_PAD + coff + int(rows[m]) * ld + N
            full[o: o + 4 - N % 4] = 0.0
    if mutation == "edge_rows_stored" and M % 16:        # the tile's row M stored as row M of C
        o = EMU_PAD + coff + M * ld
        full[o: o + N] = hi[M - 1]
    full_lo = None
    if body_lo is not None:
        full_lo = np.concatenate([np.full(EMU_PAD, np.nan, f32), body_lo, np.full(EMU_PAD, np.nan, f32)])
    return dict(full=full, full_lo=full_lo, pad=EMU_PAD)


def emulate_check(pd, mode, **kw):
    out = emulate(pd, mode, **kw)
    return check_problem(pd, mode, out["full"], out["pad"], out["full_lo"], label="emulation")


__all__ = ["CASES", "CASE_BY_NAME", "MODES", "MUTATIONS", "TILINGS", "make_problem", "lay_operand",
           "reference", "check_problem", "check_split_of", "emulate", "emulate_check", "tiles",
           "layout_ok", "m_out", "ldc", "owned_mask", "initial_body", "rows_of", "bf16_val"]
