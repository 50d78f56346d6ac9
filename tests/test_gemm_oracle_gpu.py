"""The dense GEMM kernels (csrc/kernels/gemm.hip, gemm_sp.hip, csrc/gemm_tile.h) against the float64
oracle of pytorch_r2d2_amd/gemm_ref.py: every element within its derived bound (bit for bit in the
exact cases), write ownership in NaN-poisoned guard-banded buffers (output, its ldc gap, rows
outside the row map, K-split workspace, tickets), read ownership by NaN injection, bound-free bit
identities and the launchers' refusals.  The cases are the ones tests/test_gemm_ref_cpu.py runs
through the fp32 / bf16 emulation; operands have NaN-filled leading-dimension gaps."""
import struct

import numpy as np
import pytest
import torch

from gpu_support import DEV, Buf, Guarded, buf_from_host, report_fixture
from gpu_support import stop_after_a_gpu_error  # noqa: F401
from pytorch_r2d2_amd import gemm_ref as R
from pytorch_r2d2_amd import refnum as rn
from pytorch_r2d2_amd.ops._lib import kernels, stream_handle
from pytorch_r2d2_amd.ops.gemm import G5_CFGS

pytestmark = pytest.mark.gpu
PAD = 512                       # guard elements at each end of an output / workspace buffer
LAYOUTS = [(1, 1), (1, 0), (0, 1), (0, 0)]

HEADER = """\
# The dense GEMM kernels against the float64 oracle (pytorch_r2d2_amd/gemm_ref.py), measured on an
# MI355X by tests/test_gemm_oracle_gpu.py: one line per kernel and case, the largest use of the
# per-element bound (n_add + c) u (|alpha| S + |bias| + |C_old|) over the case's problems, operand
# layouts and K splits (1.0 = at the bound; bf16 and split output: the share of the bound a value
# needs before it rounds to the stored bits).  The int_* cases are bit identities: 0 by construction.
#   r2_gemm v<N>        plain operands, r2_gemm_set_version(N): 1 register staged, 2 LDS-DMA (K % 64
#                       == 0), 5-8 the 8-wave tiles, 9 / 10 the 3- / 4-stage ring
#   r2_gemm <route>/<mode>   the multi-pass split route: v5 (256 x 256), ktail (K % 64 != 0: 256 x
#                       128), gemm2; mode x3 both operands split, a / b one of them, hh split output only
#   group <mode> A=..   r2_gemm_group, plain (hh) or split (x3) operands, A k-major / mn-major / alternating;
#                       K splits 1 / as the case / more than there are K tiles
#   gemm5 cfg<N> bk=..  r2_gemm5, every tile configuration, B k-major (1) / mn-major (0), A k-major and
#                       mn-major, K splits 1 / as the case
#   gemm5 auto cus=..   r2_gemm5 with splits = 0 for that many CUs, tiles 1, 3, 6, 7 and cfg = -1
"""
lines, report = report_fixture("R2D2_GEMM_ORACLE_REPORT", HEADER)
_AGG = {}

FIELDS = ("A", "B", "C", "bias", "crow", "M", "N", "K", "lda", "ldb", "ldc", "ak", "bk", "f32", "acc",
          "alpha", "A_lo", "B_lo", "C_lo", "pad")


def _flush():
    for (kernel, case), use in _AGG.items():
        lines.append("%-22s %-24s use %.3f" % (kernel, case, use))
    _AGG.clear()


# ---- device buffers ---------------------------------------------------------------------------------

_PD, _OPS = {}, {}


def pd_of(case, pi):
    key = (case["name"], pi)
    if key not in _PD:
        _PD[key] = R.make_problem(case, pi)
    return _PD[key]


class Operands:
    """The planes of one problem in one layout pair, each in a guard-banded buffer with NaN-filled
    leading-dimension gaps; ``poke`` = (plane, i, k): one NaN at X[i][k]."""

    def __init__(self, pd, ak, bk, poke=None):
        p = pd["p"]
        self.ak, self.bk = ak, bk
        for name, x, km, gap in (("a_hi", pd["a_hi"], ak, p["ga"]), ("a_lo", pd["a_lo"], ak, p["ga"]),
                                 ("b_hi", pd["b_hi"].T, bk, p["gb"]), ("b_lo", pd["b_lo"].T, bk, p["gb"])):
            flat, ld = R.lay_operand(x, bool(km), gap)
            if poke and poke[0] == name:
                i, k = poke[1:]
                flat[i * ld + k if km else k * ld + i] = R.NAN16
            setattr(self, name, buf_from_host(flat))
            setattr(self, "ld" + name[0], ld)
        self.bias = buf_from_host(pd["bias"]) if pd["bias"] is not None else None
        self.crow = buf_from_host(pd["crow"]) if pd["crow"] is not None else None


def ops_of(pd, ak, bk):
    key = (pd["label"], ak, bk)
    if key not in _OPS:
        _OPS[key] = Operands(pd, ak, bk)
    return _OPS[key]


class Out:
    """The output of one problem: NaN poison between guard bands, C_old at the owned elements of an
    accumulating problem; the lo plane of a split output beside it."""

    def __init__(self, pd):
        p = pd["p"]
        self.pd = pd
        dtype = torch.float32 if p["out"] == "f32" else torch.bfloat16
        self.init = torch.from_numpy(R.initial_body(pd)).to(DEV).to(dtype)
        self.c = Guarded((self.init.numel(),), dtype, PAD)
        self.lo = Guarded((self.init.numel(),), dtype, PAD) if p["out"] == "split" else None
        self.reset()

    def reset(self):
        self.c.body.copy_(self.init)
        if self.lo is not None:
            self.lo.body.fill_(float("nan"))

    def bits(self):
        return [g.bits().copy() for g in (self.c, self.lo) if g is not None]

    def values(self):
        """(M, N) fp32 values by product row."""
        p = self.pd["p"]
        body = self.c.host()[p["coff"]:].reshape(R.m_out(p), R.ldc(p))
        return body[R.rows_of(self.pd), :p["N"]]

    def check(self, mode, label):
        return R.check_problem(self.pd, mode, self.c.host_full(), self.c.pad,
                               self.lo.host_full() if self.lo is not None else None, label=label)

    def untouched(self, label):
        full = self.c.host_full()
        init = np.concatenate([np.full(self.c.pad, np.nan, np.float32), self.init.float().cpu().numpy(),
                               np.full(self.c.pad, np.nan, np.float32)])
        assert np.array_equal(full.view(np.uint32), init.view(np.uint32)), label + ": C was written"
        if self.lo is not None:
            self.lo.untouched(label, "C_lo")


def desc(pd, ops, out, mode, **over):
    p = pd["p"]
    coff = p["coff"]
    d = dict(A=ops.a_hi.p, B=ops.b_hi.p, C=out.c.ptr(coff),
             bias=ops.bias.p if ops.bias is not None else 0, crow=ops.crow.p if ops.crow is not None else 0,
             M=p["M"], N=p["N"], K=p["K"], lda=ops.lda, ldb=ops.ldb, ldc=R.ldc(p), ak=ops.ak, bk=ops.bk,
             f32=int(p["out"] == "f32"), acc=int(p["acc"]),
             alpha=struct.unpack("<I", struct.pack("<f", p["alpha"]))[0],
             A_lo=ops.a_lo.p if mode in ("x3", "a") else 0, B_lo=ops.b_lo.p if mode in ("x3", "b") else 0,
             C_lo=out.lo.ptr(coff) if out.lo is not None else 0, pad=0)
    assert tuple(d) == FIELDS
    d.update(over)
    return [d[f] for f in FIELDS]


def tiles_of(pd, bm, bn):
    p = pd["p"]
    return -(-p["M"] // bm) * -(-p["N"] // bn)


class Aux:
    """K-split workspace (poisoned, exactly ``nbytes``) and tickets (zero, exactly ``ntk``)."""

    def __init__(self, nbytes, ntk):
        assert nbytes >= 0 and nbytes % 4 == 0
        self.nbytes, self.ntk = int(nbytes), int(ntk)
        self.ws = Guarded((self.nbytes // 4,), torch.float32, PAD)
        self.tk = Buf(torch.zeros(self.ntk, dtype=torch.int32), -1)

    def check(self, label):
        full = self.ws.host_full()
        assert np.isnan(full[:PAD]).all() and np.isnan(full[full.size - PAD:]).all(), label + ": workspace guards written"
        assert (self.tk.body() == 0).all(), label + ": tickets not back to zero"
        self.tk.assert_guards(label + " tickets")

    def untouched(self, label):
        self.ws.untouched(label, "workspace")
        self.tk.assert_untouched(label + " tickets")


# ---- launchers: f(descs, pds, state) -> return code --------------------------------------------------

def gemm_launch(version):
    def f(descs, pds, state):
        k = kernels()
        k.r2_gemm_set_version(version)
        try:
            return k.r2_gemm(descs.ctypes.data, len(pds), stream_handle())
        finally:
            k.r2_gemm_set_version(2)
    return f


def group_launch(splits):
    def f(descs, pds, state):
        k = kernels()
        sp = np.asarray(splits, dtype=np.int32)
        if "aux" not in state:
            nb = k.r2_gemm_group_ws_bytes(descs.ctypes.data, sp.ctypes.data, len(pds))
            state["aux"] = Aux(nb, sum(tiles_of(pd, 128, 128) for pd, s in zip(pds, splits) if s > 1))
        a = state["aux"]
        return k.r2_gemm_group(descs.ctypes.data, sp.ctypes.data, len(pds), a.ws.ptr(), a.nbytes, a.tk.p,
                               a.ntk, stream_handle())
    return f


def g5_launch(splits, cfg, n_cus=0):
    def f(descs, pds, state):
        k = kernels()
        sp = np.asarray(splits, dtype=np.int32)
        cfgs = [cfg] if cfg >= 0 else range(len(G5_CFGS))
        if "aux" not in state:
            nb = max(k.r2_gemm5_ws_bytes_nc(descs.ctypes.data, sp.ctypes.data, len(pds), c, n_cus) for c in cfgs)
            fixed = cfg >= 0 and all(s >= 1 for s in splits)     # else: which problems split is the launcher's choice
            ntk = max(sum(tiles_of(pd, *G5_CFGS[c][:2]) for pd, s in zip(pds, splits) if s > 1 or not fixed)
                      for c in cfgs)
            state["aux"] = Aux(nb, ntk)
        a = state["aux"]
        rc = k.r2_gemm5(descs.ctypes.data, sp.ctypes.data, len(pds), cfg, a.ws.ptr(), a.nbytes, a.tk.p, a.ntk,
                        n_cus, stream_handle())
        if cfg >= 0:
            assert rc == cfg, rc
        return rc
    return f


def run_case(kernel, case, mode, aks, bk, launch, sel=None, note=True):
    """One launch of (the selected problems of) a case: ownership, bounds / bit identity, tickets and
    workspace guards, then the same launch again on the same buffers: same bits.  Returns the
    output bits of every problem."""
    sel = list(range(len(case["probs"]))) if sel is None else sel
    pds = [pd_of(case, i) for i in sel]
    ops = [ops_of(pd, aks[i], bk) for pd, i in zip(pds, sel)]
    outs = [Out(pd) for pd in pds]
    descs = np.asarray([v for pd, o, out in zip(pds, ops, outs) for v in desc(pd, o, out, mode)], dtype=np.int64)
    label = "%s ak=%s bk=%d" % (kernel, "".join(str(aks[i]) for i in sel), bk)
    state = {}
    rc = launch(descs, pds, state)
    assert rc >= 0, (label, case["name"], rc)
    torch.cuda.synchronize()
    use = max(out.check(mode, label) for out in outs)
    if "aux" in state:
        state["aux"].check(label + " " + case["name"])
    first = [out.bits() for out in outs]
    for out in outs:
        out.reset()
    assert launch(descs, pds, state) >= 0
    torch.cuda.synchronize()
    for out, b in zip(outs, first):
        for x, y in zip(out.bits(), b):
            assert np.array_equal(x, y), "%s %s: a second launch gives other bits" % (label, out.pd["label"])
    if "aux" in state:
        state["aux"].check(label + " " + case["name"] + " (second launch)")
    if note:
        key = (kernel, case["name"])
        _AGG[key] = max(_AGG.get(key, 0.0), use)
    return first


def legal(case, aks, bk, sel=None):
    return all(R.layout_ok(p, aks[i], bk) for i, p in enumerate(case["probs"]) if sel is None or i in sel)


def has_split_out(case):
    return any(p["out"] == "split" for p in case["probs"])


def k64(case):
    return all(p["K"] % 64 == 0 for p in case["probs"])


# ---- r2_gemm ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("version", [1, 2, 5, 6, 7, 8, 9, 10])
def test_r2_gemm_plain_operands(version):
    """gemm_kernel (1), gemm2_kernel (2), gemm4_kernel's four tiles (5-8), gemm3_kernel's two rings
    (9, 10); 2, 9 and 10 where K % 64 == 0."""
    n = 0
    for case in R.CASES:
        if has_split_out(case) or (version in (2, 9, 10) and not k64(case)):
            continue
        for ak, bk in LAYOUTS:
            aks = [ak] * len(case["probs"])
            if legal(case, aks, bk):
                run_case("r2_gemm v%d" % version, case, "hh", aks, bk, gemm_launch(version))
                n += 1
    _flush()
    assert n >= 20


@pytest.mark.parametrize("route", ["v5", "ktail", "gemm2"])
def test_r2_gemm_split_routes(route):
    """The multi-pass split route of r2_gemm: the 256 x 256 tile (version 5), the 256 x 128 tile that
    takes K % 64 != 0, and gemm2_kernel; both operands split, one of them, and split output alone."""
    n = 0
    for case in R.CASES:
        if (route == "ktail" and k64(case)) or (route == "gemm2" and not k64(case)):
            continue
        for mode in ("x3", "a", "b") + (("hh",) if has_split_out(case) else ()):
            for ak, bk in LAYOUTS:
                aks = [ak] * len(case["probs"])
                if legal(case, aks, bk):
                    run_case("r2_gemm %s/%s" % (route, mode), case, mode, aks, bk, gemm_launch(5 if route == "v5" else 2))
                    n += 1
    _flush()
    assert n >= 20


# ---- r2_gemm_group ------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["hh", "x3"])
@pytest.mark.parametrize("a_layout", ["k", "mn", "mixed"])
def test_r2_gemm_group(mode, a_layout):
    """Plain and split operands, A k-major / mn-major / alternating, B mn-major; K unsplit, split as
    the case says, and split into more parts than there are K tiles."""
    n = 0
    for case in R.CASES:
        np_ = len(case["probs"])
        aks = {"k": [1] * np_, "mn": [0] * np_, "mixed": [i % 2 for i in range(np_)]}[a_layout]
        if not k64(case) or not legal(case, aks, 0) or (a_layout == "mixed" and np_ == 1):
            continue
        big = [p["K"] // 64 * (1 if mode == "hh" else 3) + 1 + i for i, p in enumerate(case["probs"])]
        for splits in ([1] * np_, case["splits"], big):
            run_case("group %s A=%s" % (mode, a_layout), case, mode, aks, 0, group_launch(splits))
            n += 1
    _flush()
    assert n >= 6


# ---- r2_gemm5 -----------------------------------------------------------------------------------------

def _g5_layouts(case, cfg, bk):
    bm = G5_CFGS[cfg][0]
    np_ = len(case["probs"])
    yield [1] * np_
    if bm % 128 == 0:
        yield [0 if p["M"] % 8 == 0 and i % 2 == 0 else 1 for i, p in enumerate(case["probs"])]


@pytest.mark.parametrize("cfg,bk", [(c, b) for c in range(len(G5_CFGS)) for b in (1, 0) if b or G5_CFGS[c][1] % 128 == 0])
def test_r2_gemm5(cfg, bk):
    """Every tile configuration the layout permits, A k-major and (where the tile permits) mn-major;
    K % 32 == 0 (the fixed-offset staging) and not; K unsplit and split as the case says."""
    n = 0
    for case in R.CASES:
        seen = []
        for aks in _g5_layouts(case, cfg, bk):
            if not legal(case, aks, bk) or aks in seen:
                continue
            seen.append(aks)
            for splits in ([1] * len(aks), case["splits"]):
                run_case("gemm5 cfg%d bk=%d" % (cfg, bk), case, "x3", aks, bk, g5_launch(splits, cfg))
                n += 1
    _flush()
    assert n >= 20


@pytest.mark.parametrize("n_cus", [8, 64, 256])
def test_r2_gemm5_auto_split_and_auto_tile(n_cus):
    """splits = 0: the K split the launcher chooses for n_cus CUs (what every learner call site
    passes), on fixed tiles and with cfg = -1."""
    n = 0
    for case in R.CASES:
        for bk in (1, 0):
            aks = [1] * len(case["probs"])
            if not legal(case, aks, bk):
                continue
            for cfg in (-1, 1, 3, 6, 7):
                run_case("gemm5 auto cus=%d" % n_cus, case, "x3", aks, bk, g5_launch([0] * len(aks), cfg, n_cus))
                n += 1
    _flush()
    assert n >= 100


# ---- read ownership -----------------------------------------------------------------------------------

FAMILIES = [("r2_gemm v1", "hh", lambda: gemm_launch(1)), ("r2_gemm v2", "hh", lambda: gemm_launch(2)),
            ("r2_gemm v6", "hh", lambda: gemm_launch(6)), ("r2_gemm v10", "hh", lambda: gemm_launch(10)),
            ("r2_gemm v5/x3", "x3", lambda: gemm_launch(5)), ("group", "x3", lambda: group_launch([3])),
            ("gemm5 cfg0", "x3", lambda: g5_launch([1], 0)), ("gemm5 cfg3", "x3", lambda: g5_launch([2], 3))]


@pytest.mark.parametrize("family", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_one_nan_poisons_exactly_its_row_or_column(family):
    """One NaN at A[m0][k0] makes exactly row m0 of C NaN, one at B[k0][n0] exactly column n0: the
    kernel multiplies each operand element into the elements that own it and no other.  First and
    last row / column, first and last K chunk."""
    kernel, mode, launch = family
    case = R.CASE_BY_NAME["m248n120k256"]
    pd = pd_of(case, 0)
    M, N, K = (pd["p"][k] for k in "MNK")
    for ak, bk in ((1, 1), (0, 0), (1, 0)):
        if (kernel == "group" and bk) or (kernel == "gemm5 cfg0" and not ak):
            continue
        for plane, i, k in (("a_hi", 0, 0), ("a_hi", M - 1, K - 1), ("b_hi", 0, K - 1), ("b_hi", N - 1, 0)):
            ops = Operands(pd, ak, bk, poke=(plane, i, k))
            out = Out(pd)
            descs = np.asarray(desc(pd, ops, out, mode), dtype=np.int64)
            assert launch()(descs, [pd], {}) >= 0
            torch.cuda.synchronize()
            v = out.values()
            want = np.zeros((M, N), bool)
            if plane == "a_hi":
                want[i, :] = True
            else:
                want[:, i] = True
            bad = np.argwhere(np.isnan(v) != want)
            assert bad.size == 0, "%s ak=%d bk=%d NaN at %s[%d][%d]: C[%d][%d] is %r" % (
                kernel, ak, bk, plane, i, k, bad[0][0], bad[0][1], v[tuple(bad[0])])


# ---- agreement that needs no bound --------------------------------------------------------------------

def test_k_split_result_does_not_depend_on_the_item_order():
    """r2_gemm5's two item orders (K-split-major and tile-major) give the same bits on an edge shape."""
    k = kernels()
    case = R.CASE_BY_NAME["four_tails"]
    got = []
    try:
        for m in (0, 1 << 6):
            k.r2_gemm5_set_mode(m)
            got.append(run_case("gemm5 order", case, "x3", [1] * 4, 1, g5_launch(case["splits"], 5), note=False))
    finally:
        k.r2_gemm5_set_mode(0)
    for a, b in zip(*got):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)


ALONE = [("r2_gemm v2", "hh", 0, "gemm", 2), ("r2_gemm v5", "hh", 1, "gemm", 5), ("r2_gemm v9", "hh", 1, "gemm", 9),
         ("r2_gemm gemm2/x3", "x3", 0, "gemm", 2), ("group", "x3", 0, "group", [2, 3, 1, 2]),
         ("gemm5 cfg1", "x3", 0, "g5", (1, [2, 1, 3, 2])), ("gemm5 cfg7", "x3", 1, "g5", (7, [1, 2, 2, 3]))]


def _alone_launch(kind, arg, sel):
    if kind == "gemm":
        return gemm_launch(arg)
    if kind == "group":
        return group_launch([arg[i] for i in sel])
    return g5_launch([arg[1][i] for i in sel], arg[0])


@pytest.mark.parametrize("family", ALONE, ids=[f[0] for f in ALONE])
def test_one_problem_alone_or_as_one_of_four(family):
    """The tile a problem's element falls in, and so its bits, do not depend on the other problems of
    the launch (each keeps its K split)."""
    kernel, mode, bk, kind, arg = family
    case = R.CASE_BY_NAME["four_k64"]
    if mode == "hh":         # plain kernels take no split output: the same shapes without it
        case = dict(case, name="four_k64_plain", probs=[dict(p, out="bf16" if p["out"] == "split" else p["out"])
                                                        for p in case["probs"]])
    aks = [1, 1, 1, 1]
    together = run_case(kernel, case, mode, aks, bk, _alone_launch(kind, arg, range(4)), note=False)
    for i in range(4):
        alone = run_case(kernel, case, mode, aks, bk, _alone_launch(kind, arg, [i]), sel=[i], note=False)
        for x, y in zip(alone[0], together[i]):
            assert np.array_equal(x, y), "%s: problem %d alone differs from the launch of four" % (kernel, i)


@pytest.mark.parametrize("family", ["r2_gemm gemm2", "r2_gemm v5", "r2_gemm ktail", "group", "gemm5 cfg2", "gemm5 cfg5"])
def test_split_output_is_the_split_of_the_fp32_output(family):
    """Bound-free: hi == bf16(v) and lo == bf16(v - hi) with v the fp32 output of the same kernel for
    the same problem; vector and scalar epilogue."""
    for name in ("m136n136k128", "m200n72k200"):
        case = R.CASE_BY_NAME[name]
        if (family in ("r2_gemm gemm2", "group") and not k64(case)) or (family == "r2_gemm ktail" and k64(case)):
            continue
        split = pd_of(case, 0)
        twin = dict(split, p=dict(split["p"], out="f32"), label=split["label"] + "_f32")
        ops = ops_of(split, 1, 0 if family == "group" else 1)
        outs = []
        for pd in (split, twin):
            out = Out(pd)
            descs = np.asarray(desc(pd, ops, out, "x3"), dtype=np.int64)
            ln = {"r2_gemm gemm2": lambda: gemm_launch(2), "r2_gemm v5": lambda: gemm_launch(5),
                  "r2_gemm ktail": lambda: gemm_launch(2), "group": lambda: group_launch([2]),
                  "gemm5 cfg2": lambda: g5_launch([2], 2), "gemm5 cfg5": lambda: g5_launch([1], 5)}[family]()
            assert ln(descs, [pd], {}) >= 0
            torch.cuda.synchronize()
            outs.append(out)
        sp, f32 = outs
        p = sp.pd["p"]
        lo = sp.lo.host()[p["coff"]:].reshape(R.m_out(p), R.ldc(p))[R.rows_of(sp.pd), :p["N"]]
        R.check_split_of("%s %s" % (family, name), f32.values(), rn.bf16_bits(sp.values()), rn.bf16_bits(lo))


# ---- refusals -----------------------------------------------------------------------------------------

def _refusal_setup(mode="x3", bk=0, n=1):
    case = R.CASE_BY_NAME["two_k64"]
    pds = [pd_of(case, i) for i in range(n)]
    ops = [ops_of(pd, 1, bk) for pd in pds]
    outs = [Out(pd) for pd in pds]
    return pds, ops, outs


def _descs(pds, ops, outs, mode, over=None):
    rows = [desc(pd, o, out, mode, **((over or {}).get(i, {}))) for i, (pd, o, out) in enumerate(zip(pds, ops, outs))]
    return np.asarray([v for r in rows for v in r], dtype=np.int64)


PARSE = [(-2, dict(K=4)), (-2, dict(K=68)), (-2, dict(M=0)), (-2, dict(N=0)), (-3, dict(bk=0, N=130)),
         (-3, dict(ak=0, M=131)), (-4, dict(lda=76)), (-4, dict(ldb=132)), (-12, dict(C_lo=1, f32=1)),
         (-12, dict(C_lo=1, f32=0, acc=1))]


@pytest.mark.parametrize("entry", ["r2_gemm", "r2_gemm_group", "r2_gemm5"])
def test_descriptor_refusals(entry):
    """gemm_parse_desc's codes through every launcher; a refused launch writes nothing."""
    k = kernels()
    for code, over in PARSE:
        pds, ops, outs = _refusal_setup(bk=0 if "bk" in over or entry != "r2_gemm" else 1)
        if "C_lo" in over:
            over = dict(over, C_lo=outs[0].c.ptr())
        descs = _descs(pds, ops, outs, "x3", {0: over})
        aux = Aux(4 << 20, 64)
        sp = np.asarray([2], dtype=np.int32)
        if entry == "r2_gemm":
            rc = k.r2_gemm(descs.ctypes.data, 1, stream_handle())
        elif entry == "r2_gemm_group":
            rc = k.r2_gemm_group(descs.ctypes.data, sp.ctypes.data, 1, aux.ws.ptr(), aux.nbytes, aux.tk.p, aux.ntk,
                                 stream_handle())
        else:
            rc = k.r2_gemm5(descs.ctypes.data, sp.ctypes.data, 1, 1, aux.ws.ptr(), aux.nbytes, aux.tk.p, aux.ntk, 0,
                            stream_handle())
        torch.cuda.synchronize()
        assert rc == code, (entry, over, rc)
        outs[0].untouched("%s %r" % (entry, over))
        aux.untouched("%s %r" % (entry, over))


def test_r2_gemm_refusals():
    k = kernels()
    pds, ops, outs = _refusal_setup("hh", bk=0, n=2)
    descs = _descs(pds, ops, outs, "hh")
    for n in (0, 5):
        assert k.r2_gemm(descs.ctypes.data, n, stream_handle()) == -1
    # two problems with different layouts: B of the second k-major
    other = ops_of(pds[1], 1, 1)
    mixed = np.concatenate([descs[:20], np.asarray(desc(pds[1], other, outs[1], "hh"), dtype=np.int64)])
    assert k.r2_gemm(mixed.ctypes.data, 2, stream_handle()) == -5
    torch.cuda.synchronize()
    for out in outs:
        out.untouched("r2_gemm")


def test_r2_gemm_group_refusals():
    """-6: a shape the group kernel does not take; -7: the workspace one byte short, one ticket short."""
    k = kernels()
    pds, ops, outs = _refusal_setup("hh", bk=0, n=2)
    descs = _descs(pds, ops, outs, "hh")
    sp = np.asarray([2, 3], dtype=np.int32)
    nb = k.r2_gemm_group_ws_bytes(descs.ctypes.data, sp.ctypes.data, 2)
    ntk = sum(tiles_of(pd, 128, 128) for pd in pds)
    assert nb == ntk_bytes(pds, sp, 128, 128)
    aux = Aux(nb, ntk)

    def go(d, n=2, nbytes=nb, ntk_=ntk):
        return k.r2_gemm_group(d.ctypes.data, sp.ctypes.data, n, aux.ws.ptr(), nbytes, aux.tk.p, ntk_, stream_handle())

    assert go(descs, n=0) == -1 and go(descs, n=5) == -1
    assert go(_descs(pds, ops, outs, "hh", {1: dict(K=72)})) == -6
    kmaj = ops_of(pds[0], 1, 1)
    assert go(np.asarray(desc(pds[0], kmaj, outs[0], "hh"), dtype=np.int64), n=1) == -6
    assert go(descs, nbytes=nb - 1) == -7
    assert go(descs, ntk_=ntk - 1) == -7
    torch.cuda.synchronize()
    for out in outs:
        out.untouched("r2_gemm_group")
    aux.untouched("r2_gemm_group")
    assert go(descs) == 0          # and with exactly what was asked for it runs
    torch.cuda.synchronize()
    for out in outs:
        out.check("hh", "group after the refusals")
    aux.check("group after the refusals")


def ntk_bytes(pds, sp, bm, bn):
    return sum(tiles_of(pd, bm, bn) * int(s) * bm * bn * 4 for pd, s in zip(pds, sp) if s > 1)


def test_r2_gemm5_refusals():
    """-5: two B layouts; -7: workspace one byte / one ticket short; -8: no such tile, or a tile the
    layout does not permit; -10: an operand without its lo plane."""
    k = kernels()
    pds, ops, outs = _refusal_setup("x3", bk=0, n=2)
    descs = _descs(pds, ops, outs, "x3")
    sp = np.asarray([2, 3], dtype=np.int32)
    cfg = 1
    nb = k.r2_gemm5_ws_bytes_nc(descs.ctypes.data, sp.ctypes.data, 2, cfg, 0)
    assert nb == ntk_bytes(pds, sp, 128, 128)
    ntk = sum(tiles_of(pd, 128, 128) for pd in pds)
    aux = Aux(nb, ntk)

    def go(d, n=2, c=cfg, nbytes=nb, ntk_=ntk):
        return k.r2_gemm5(d.ctypes.data, sp.ctypes.data, n, c, aux.ws.ptr(), nbytes, aux.tk.p, ntk_, 0, stream_handle())

    assert go(descs, n=0) == -1 and go(descs, n=5) == -1
    other = ops_of(pds[1], 1, 1)
    mixed = np.concatenate([descs[:20], np.asarray(desc(pds[1], other, outs[1], "x3"), dtype=np.int64)])
    assert go(mixed) == -5
    assert go(descs, nbytes=nb - 1) == -7
    assert go(descs, ntk_=ntk - 1) == -7
    assert go(descs, c=len(G5_CFGS)) == -8
    assert go(descs, c=4) == -8                       # 256 x 64 needs a k-major B
    mn_a = ops_of(pds[0], 0, 0)
    assert go(np.asarray(desc(pds[0], mn_a, outs[0], "x3"), dtype=np.int64), n=1, c=0) == -8   # 192 rows: k-major A
    for mode in ("hh", "a", "b"):
        assert go(_descs(pds, ops, outs, mode)) == -10
    assert k.r2_gemm5_ws_bytes_nc(descs.ctypes.data, sp.ctypes.data, 2, len(G5_CFGS), 0) == -1
    torch.cuda.synchronize()
    for out in outs:
        out.untouched("r2_gemm5")
    aux.untouched("r2_gemm5")
    assert go(descs) == cfg
    torch.cuda.synchronize()
    for out in outs:
        out.check("x3", "gemm5 after the refusals")
    aux.check("gemm5 after the refusals")
