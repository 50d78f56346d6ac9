"""r2_state_refresh (csrc/kernels/state_refresh.hip) against the float64 / integer oracle
(pytorch_r2d2_amd/state_refresh_ref.py), launched directly on guarded buffers: written rows equal
the oracle bit for bit (the values are copies or one exact fp32 add), every other byte of hs_cs /
target_hs_cs and every guard keeps its bits, "measure" writes nothing, the drift sums stay inside the
oracle's a-priori bound, two launches give the same drift bits and the ticket is back at zero."""
import numpy as np
import pytest
import torch

from gpu_support import Buf, buf_from_host, stop_after_a_gpu_error  # noqa: F401
from pytorch_r2d2_amd import refnum
from pytorch_r2d2_amd import state_refresh_ref as sr
from pytorch_r2d2_amd.ops._lib import kernels, stream_handle

pytestmark = pytest.mark.gpu

# B 6, burn-in 3 + learn 5, n 2, two sub-rings of 16 rows: slots 0 / 1 overlap (rows 1..8, 4..11),
# slots 2 / 3 are the same start, slot 4 wraps its sub-ring's end (13, 14, 15, 0, ..) and meets
# slots 0, 2 and 3, slot 5 sits alone in the second sub-ring
STARTS = (1, 4, 11, 11, 13, 18)
BURN, LEARN, N, CAP_E, N_SUB = 3, 5, 2, 16, 2


class Case:
    def __init__(self, spec, starts, H, split, n_sub, seed=0):
        self.spec, self.H, self.split = spec, H, split
        self.starts = np.asarray(starts, dtype=np.int32)
        rng = np.random.default_rng(seed)
        f = lambda *s: rng.standard_normal(s).astype(np.float32)   # noqa: E731
        T, n = spec.T, spec.n_step
        shifted = spec.target_mode == "shifted"
        self.steps = {"on": T + n if shifted else T, "tg": T + n if shifted else T}
        self.cap = spec.cap_e * n_sub
        self.hi, self.lo, self.c, self.h = {}, {}, {}, {}
        for ch in sr.CHAINS:
            x = f(self.steps[ch], spec.B, H)
            hi, lo = refnum.split_planes(x)
            self.hi[ch], self.lo[ch] = refnum.bf16_bits(hi), (refnum.bf16_bits(lo) if split else None)
            self.h[ch] = sr.combine_h(self.hi[ch], self.lo[ch])
            self.c[ch] = f(self.steps[ch], spec.B, H)
        self.hs0, self.ths0 = f(self.cap, 2 * H), f(self.cap, 2 * H)
        # device side
        self.d_starts = buf_from_host(self.starts)
        self.d_hi = {ch: buf_from_host(self.hi[ch]) for ch in sr.CHAINS}
        self.d_lo = {ch: buf_from_host(self.lo[ch]) if split else None for ch in sr.CHAINS}
        self.d_c = {ch: buf_from_host(self.c[ch]) for ch in sr.CHAINS}
        self.d_hs, self.d_ths = buf_from_host(self.hs0), buf_from_host(self.ths0)
        self.d_out = Buf.poisoned(12, torch.float32, float("nan"))
        self.d_part = Buf(torch.zeros(int(kernels().r2_state_refresh_partials())), float("nan"))
        self.d_ticket = Buf(torch.zeros(1, dtype=torch.int32), -1)

    def ref(self, mode):
        return sr.refresh_ref(self.starts, self.spec, self.h, self.c, self.hs0, self.ths0, mode)

    def launch(self, write, **over):
        sp = self.spec
        a = dict(T=sp.T, cap_e=sp.cap_e, capacity=self.cap, steps_on=self.steps["on"],
                 steps_tg=self.steps["tg"], hs=self.d_hs.p, ths=self.d_ths.p, c_on=self.d_c["on"].p,
                 o_tg=sr.chain_offset("tg", sp.target_mode, sp.n_step), ctx=sp.ctx)
        a.update(over)
        lo = lambda ch: self.d_lo[ch].p if self.split else 0   # noqa: E731
        rc = kernels().r2_state_refresh(
            self.d_starts.p, sp.B, self.H, a["T"], a["cap_e"], a["capacity"],
            self.d_hi["on"].p, lo("on"), a["c_on"], a["steps_on"],
            self.d_hi["tg"].p, lo("tg"), self.d_c["tg"].p, a["steps_tg"],
            a["hs"], a["ths"], a["o_tg"], sr.row_shift(sp.stored_state), a["ctx"], int(write),
            self.d_out.p, self.d_part.p, self.d_ticket.p, stream_handle())
        torch.cuda.synchronize()
        return rc

    def drift(self):
        """(bits of the ten drift words, sums per chain, rows per chain); the pad stays poison."""
        o = self.d_out.body()
        assert np.isnan(o[10:]).all(), "the drift words' padding was written"
        return (o[:10].view(np.uint32).copy(), {"on": o[0:4], "tg": o[4:8]},
                {"on": int(o[8]), "tg": int(o[9])})

    def check_plumbing(self, what):
        for name, b in [("starts", self.d_starts), ("c_on", self.d_c["on"]), ("c_tg", self.d_c["tg"]),
                        ("h_on", self.d_hi["on"]), ("h_tg", self.d_hi["tg"])] + \
                       ([("lo_on", self.d_lo["on"]), ("lo_tg", self.d_lo["tg"])] if self.split else []):
            b.assert_untouched(f"{what}: {name}")
        for name, b in (("out", self.d_out), ("partials", self.d_part), ("ticket", self.d_ticket),
                        ("hs_cs", self.d_hs), ("target_hs_cs", self.d_ths)):
            b.assert_guards(f"{what}: {name}")
        assert int(self.d_ticket.body()[0]) == 0, f"{what}: the ticket is not back at zero"


def run_case(case):
    H = case.H
    ref_m, ref_w = case.ref("measure"), case.ref("write")
    assert ref_w.rows["on"] > 0
    # measure: nothing written, sums inside the bound
    assert case.launch(write=0) == 0
    case.check_plumbing("measure")
    case.d_hs.assert_untouched("measure: hs_cs")
    case.d_ths.assert_untouched("measure: target_hs_cs")
    bits_m, sums, rows = case.drift()
    use = sr.check_drift(ref_m, H, sums, rows)
    # again: the same bits
    assert case.launch(write=0) == 0
    case.check_plumbing("measure twice")
    assert np.array_equal(case.drift()[0], bits_m), "two launches gave different drift bits"
    # write: every byte equals the oracle's array (written rows and all others), guards kept; the
    # drift comes from the values it overwrites, so it is the measure launch's, bit for bit
    assert case.launch(write=1) == 0
    case.check_plumbing("write")
    for name, buf, want in (("hs_cs", case.d_hs, ref_w.hs_cs), ("target_hs_cs", case.d_ths, ref_w.target_hs_cs)):
        got = buf.body().view(np.uint32).reshape(-1, 2 * H)
        refnum.bits_equal("write", name, got, want.view(np.uint32), names=("row", "col"))
    assert np.array_equal(case.drift()[0], bits_m), "write and measure report different drift bits"
    return use


CASES = [pytest.param(split, stored, tmode, ctx, id=f"{'fp32' if split else 'bf16'}-{stored}-{tmode}-ctx{ctx}")
         for split in (True, False) for stored in ("post", "pre") for tmode in ("shifted", "fixed")
         for ctx in (0, -1)]


@pytest.mark.parametrize("split,stored,tmode,ctx", CASES)
def test_kernel_matches_oracle(split, stored, tmode, ctx):
    spec = sr.Spec(B=len(STARTS), burn_in=BURN, learn=LEARN, n_step=N, cap_e=CAP_E, target_mode=tmode,
                   stored_state=stored, context=ctx)
    case = Case(spec, STARTS, 64, split, N_SUB)
    # the case table does what it says: rows shared between slots, a wrapped window, a lone slot
    rows, b, _ = sr.entries(case.starts, spec, "on")
    assert rows.size > np.unique(rows).size and (rows[b == 4] < 13).any() and (rows[b == 5] >= 16).all()
    run_case(case)


def test_kernel_hidden_256():
    spec = sr.Spec(B=len(STARTS), burn_in=BURN, learn=LEARN, n_step=N, cap_e=CAP_E, target_mode="fixed",
                   stored_state="pre", context=-1)
    run_case(Case(spec, STARTS, 256, True, N_SUB, seed=1))


def test_kernel_grid_stride():
    """More items than the launch has waves (64 slots x 75 steps > 4 x 1024): every wave takes
    several items, and the final sum runs over the full grid's partials."""
    spec = sr.Spec(B=64, burn_in=0, learn=40, n_step=5, cap_e=64, target_mode="fixed",
                   stored_state="post", context=0)
    rng = np.random.default_rng(7)
    starts = rng.integers(0, 64 * 8, 64)
    starts[10] = starts[3]
    case = Case(spec, starts, 64, True, 8, seed=2)
    assert spec.B * (40 + 35) > 4096
    run_case(case)


def test_launcher_refusals_write_nothing():
    spec = sr.Spec(B=len(STARTS), burn_in=BURN, learn=LEARN, n_step=N, cap_e=CAP_E, target_mode="fixed",
                   stored_state="post", context=-1)
    case = Case(spec, STARTS, 64, True, N_SUB)
    bad = [dict(cap_e=spec.T - 1, capacity=2 * (spec.T - 1)),      # a window longer than its sub-ring
           dict(capacity=case.cap + 1),                            # not whole sub-rings
           dict(ctx=spec.T), dict(ctx=-1), dict(o_tg=-1),
           dict(steps_on=spec.T - 1),                              # a chain shorter than its eligible steps
           dict(hs=case.d_hs.p + 4), dict(c_on=case.d_c["on"].p + 4),   # not 16-byte aligned
           dict(ths=case.d_hs.p), dict(hs=0)]
    for over in bad:
        assert case.launch(write=1, **over) == -1, over
    case.check_plumbing("refused")
    for b in (case.d_hs, case.d_ths, case.d_out, case.d_part):
        b.assert_untouched("refused")
