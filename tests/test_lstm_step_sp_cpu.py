"""The oracle's own control for the split-precision step kernel (csrc/kernels/lstm_step_sp.hip):
on the chain shapes of tests/test_lstm_step_sp_gpu.py the fp32 emulation of three-pass products
(lstm_ref.emulate_forward) passes lstm_ref.check_forward(sp=True) inside every bound, and two
emulations of the bf16 path's shortcuts -- the lo planes dropped, h0 rounded to bf16 -- are
rejected: the bounds tell split precision from bf16 operands."""
import numpy as np
import pytest

from pytorch_r2d2_amd import lstm_ref as R
from pytorch_r2d2_amd import refnum as rn


def _emulate(ch, T, drop_lo=False):
    """lstm_ref.emulate_forward(sp=True) re-stated with the stored planes as the recurrent operand
    (no 19-bit word) and, with ``drop_lo``, the hi.hi pass alone."""
    ops = R.forward_operands(ch, True)
    B, H = ch["c0"].shape
    col = R.gate_cols(H)
    sf = int(ch["save_from"])
    c = ch["c0"].astype(np.float32)
    x = ch["xproj"].astype(np.float32)
    cs, hs, gs = [], [], []
    h = ops["h0"]
    for t in range(T):
        a_hi, a_lo = rn.split_planes(h)
        if drop_lo:
            pre = R._mm32(a_hi, None, ops["w_hi"], None, 64)
        else:
            pre = R._mm32(a_hi, a_lo, ops["w_hi"], ops["w_lo"], 64)
        pre = (pre + x[t]).astype(np.float32)
        gi, gf = R._sig32(pre[:, col[0]]), R._sig32(pre[:, col[1]])
        gg, go = R._tanh32(pre[:, col[2]]), R._sig32(pre[:, col[3]])
        c = (gf * c + gi * gg).astype(np.float32)
        h = (go * R._tanh32(c)).astype(np.float32)
        g = np.empty((B, 4 * H), np.float32)
        g[:, col[0]], g[:, col[1]], g[:, col[2]], g[:, col[3]] = gi, gf, gg, go
        cs.append(c), hs.append(h), gs.append(g)
    h32 = np.stack(hs)
    hi = rn.bf16_round(h32)
    lo = (h32 - hi).astype(np.float32)
    return dict(c_seq=np.stack(cs), h32=h32, h_seq_bits=rn.bf16_bits(h32), h_seq=hi,
                h_seq_lo_bits=rn.bf16_bits(lo), h_seq_lo=rn.bf16_round(lo),
                gates=np.stack(gs)[sf:] if sf < T else np.zeros((0, B, 4 * H), np.float32))


@pytest.mark.parametrize("name", list(R.STEP_SP_CASES))
def test_emulation_is_inside_every_bound(name):
    spec, chains = R.step_sp_case(name)
    for c, ch in enumerate(chains):
        for label, out in (("tagged emulation", R.emulate_forward(ch, True, spec["T"])),
                           ("step emulation", _emulate(ch, spec["T"]))):
            uses = R.check_forward(f"{name}/chain{c}/{label}", ch, out, sp=True)
            print(f"lstm-step-sp: {name}/chain{c} {label}: " +
                  "  ".join(f"{k} {v:.3f}" for k, v in uses.items()))
            assert max(uses.values()) < 1.0


@pytest.mark.parametrize("name", list(R.STEP_SP_CASES))
def test_bf16_shortcuts_are_rejected(name):
    spec, chains = R.step_sp_case(name)
    ch = chains[0]
    with pytest.raises(AssertionError):          # hi.hi only
        R.check_forward(f"{name}/drop_lo", ch, _emulate(ch, spec["T"], drop_lo=True), sp=True)
    rounded = dict(ch, h0=rn.bf16_round(ch["h0"]))
    with pytest.raises(AssertionError):          # h0 through bf16, as the bf16 path carries it
        R.check_forward(f"{name}/h0_bf16", ch, R.emulate_forward(rounded, True, spec["T"]), sp=True)


def test_halves_are_rows_of_one_net():
    """s_halves: chains 2n, 2n + 1 share net n's weights and are its two row halves."""
    spec, chains = R.step_sp_case("s_halves")
    assert len(chains) == 4 and [c["net"] for c in chains] == [0, 0, 1, 1]
    assert [c["row0"] for c in chains] == [0, spec["B"], 0, spec["B"]]
    assert chains[0]["w"] is chains[1]["w"] and chains[0]["w"] is not chains[2]["w"]
    assert not np.array_equal(chains[0]["h0"], chains[1]["h0"])
