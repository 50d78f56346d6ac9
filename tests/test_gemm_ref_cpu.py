"""The GEMM oracle (pytorch_r2d2_amd/gemm_ref.py) on the CPU: the fp32 / bf16 emulation of the
kernels passes every case within the derived bounds, the exact cases are exact in any summation
order, every named mutation of the emulation is caught by a named case, and the case table covers
the kernels' edges it claims to cover."""
import numpy as np
import pytest

from pytorch_r2d2_amd import gemm_ref as R
from pytorch_r2d2_amd import refnum as rn

_PD = {}


def _pd(case, pi):
    key = (case["name"], pi)
    if key not in _PD:
        _PD[key] = R.make_problem(case, pi)
    return _PD[key]


@pytest.mark.parametrize("case", R.CASES, ids=[c["name"] for c in R.CASES])
def test_emulation_within_bounds(case):
    """The reference alone: both summation orders, both K tiles, unsplit and the case's K split, all
    four operand modes.  The exact cases report 0 (bit identity inside check_problem)."""
    worst = 0.0
    for pi, sp in enumerate(case["splits"]):
        pd = _pd(case, pi)
        for mode in R.MODES:
            for split, order, bk in ((1, 0, 32), (sp, 0, 64), (1, 1, 64), (sp, 1, 32)):
                use = R.emulate_check(pd, mode, split=split, order=order, bk=bk)
                assert use <= 1.0
                assert not pd["exact"] or use == 0.0
                worst = max(worst, use)
    print("%-26s largest use of the bound %.3f" % (case["name"], worst))
    # the bound leaves the emulation (round to nearest, n additions) its sqrt(n) against n
    assert worst < 0.5


def test_exact_cases_are_exact_in_any_order():
    """Integer planes: two summation orders, two K tiles and a K split give the same bits, and
    they are the bits of the float64 oracle."""
    n = 0
    for case in R.CASES:
        if case["data"] != "int":
            continue
        for pi, sp in enumerate(case["splits"]):
            pd = _pd(case, pi)
            for mode in R.MODES:
                a = R.emulate(pd, mode, split=1, order=0, bk=32)
                b = R.emulate(pd, mode, split=sp, order=1, bk=64)
                assert np.array_equal(a["full"].view(np.uint32), b["full"].view(np.uint32))
                if a["full_lo"] is not None:
                    assert np.array_equal(a["full_lo"].view(np.uint32), b["full_lo"].view(np.uint32))
                ref, _ = R.reference(pd, mode)
                assert np.all(ref == np.rint(ref * 8) / 8) and np.abs(ref).max() < 2 ** 24
                n += 1
    assert n >= 8 * len(R.MODES)


def _catches(mutation):
    """The first (case, problem, mode) whose check rejects the mutated emulation, with the message."""
    for case in R.CASES:
        for pi, sp in enumerate(case["splits"]):
            pd = _pd(case, pi)
            for mode in ("x3", "hh"):
                out = R.emulate(pd, mode, split=sp, mutation=mutation)
                try:
                    R.check_problem(pd, mode, out["full"], out["pad"], out["full_lo"])
                except AssertionError as e:
                    return "%s/%d [%s]" % (case["name"], pi, mode), str(e)
    return None, None


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_mutation_is_caught(mutation):
    where, msg = _catches(mutation)
    assert where is not None, "no case rejects the mutation %s" % mutation
    print("%-24s caught by %-32s %s" % (mutation, where, msg.split(";")[0][:150]))


def test_cross_term_cannot_hide_in_a_cancellation_case():
    """|C| << S there: an error relative to |C| would pass a dropped cross term, the bound relative
    to S does not."""
    case = R.CASE_BY_NAME["cancel_m136n72k256"]
    pd = _pd(case, 0)
    ref, bound = R.reference(pd, "x3")
    S = bound / ((3 * 256 + 4) * R.U)
    assert np.median(np.abs(ref - pd["bias"]) / S) < 0.05
    out = R.emulate(pd, "x3", mutation="cross_term_dropped")
    with pytest.raises(AssertionError, match=r"C\[m=\d+, n=\d+\]"):
        R.check_problem(pd, "x3", out["full"], out["pad"], out["full_lo"])


def test_case_table_covers_what_it_claims():
    probs = [p for c in R.CASES for p in c["probs"]]
    Ms, Ns, Ks = ({p[k] for p in probs} for k in "MNK")
    for t in R.TILE_ROWS:
        assert {t - 8, t, t + 8} <= Ms, t
    for t in R.TILE_COLS:
        assert {t - 8, t, t + 8} <= Ns, t
    for bk in R.TILE_K:
        assert any(k % bk for k in Ks) and any(k < bk for k in Ks), bk
    # K shorter than the rings: one and two K tiles (of 32 and of 64) against NS = 3 and 4
    assert {32, 64, 128} <= Ks and {8, 24, 40, 72, 136, 200} <= Ks
    # the XCD remap of a launch depends on its tile count mod 8
    # (over the cases each remapping kernel takes with plain operands: no split output; gemm3 K % 64)
    plain = [c for c in R.CASES if all(p["out"] != "split" for p in c["probs"])]
    k64 = [c for c in plain if all(p["K"] % 64 == 0 for p in c["probs"])]
    for bm, bn, cases in ((128, 128, k64), (256, 256, plain), (256, 128, plain)):
        assert {R.tiles(c, bm, bn) % 8 for c in cases} == set(range(8)), (bm, bn)
    # the scalar epilogue: N % 4, ldc % 4, an offset C; the straddle of a vector store
    assert any(p["N"] % 4 and R.ldc(p) % 4 for p in probs)
    assert any(p["N"] % 4 and R.ldc(p) % 4 == 0 and p["coff"] == 0 for p in probs)
    for out in ("f32", "bf16", "split"):
        assert any(p["out"] == out and p["coff"] for p in probs), out
        assert any(p["out"] == out and p["coff"] == 0 and R.ldc(p) % 4 == 0 and p["N"] % 4 for p in probs), out
    for out in ("f32", "bf16"):
        assert {p["acc"] for p in probs if p["out"] == out} == {True, False}
    assert {p["crow"] for p in probs} == {"none", "id", "perm", "inject"}
    assert {len(c["probs"]) for c in R.CASES} == {1, 2, 3, 4}
    # a K split with more splits than K tiles (of 64 and of 32)
    assert any(s > -(-p["K"] // 32) for c in R.CASES for p, s in zip(c["probs"], c["splits"]))
    assert any(s > -(-p["K"] // 64) and p["K"] % 64 == 0 and p["N"] % 8 == 0
               for c in R.CASES for p, s in zip(c["probs"], c["splits"]))
    assert max(p["M"] * p["N"] * p["K"] for p in probs) <= 400 * 400 * 256
    assert len(R.CASES) <= 48


def test_operand_layout_and_ownership_helpers():
    case = R.CASE_BY_NAME["m16n50k40"]
    pd = _pd(case, 0)
    flat, ld = R.lay_operand(pd["a_hi"], True, 8)
    assert ld == 48 and np.array_equal(rn.bf16_val(flat.reshape(16, 48)[:, :40]), pd["a_hi"])
    assert (flat.reshape(16, 48)[:, 40:] == R.NAN16).all()
    flat, ld = R.lay_operand(pd["a_hi"], False, 8)
    assert ld == 24 and np.array_equal(rn.bf16_val(flat.reshape(40, 24)[:, :16]).T, pd["a_hi"])
    own = R.owned_mask(pd)
    assert own.size == 21 * 51 and own.sum() == 16 * 50
    body = R.initial_body(pd)
    assert np.isnan(body).all()
    acc = _pd(R.CASE_BY_NAME["m56n130k72"], 0)
    assert np.isfinite(R.initial_body(acc)[R.owned_mask(acc)]).all()
    assert np.isnan(R.initial_body(acc)[~R.owned_mask(acc)]).all()
