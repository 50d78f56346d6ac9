"""The LSTM oracle (pytorch_r2d2_amd/lstm_ref.py) on the CPU: it is the float64 LSTM, its bounds
admit an fp32 emulation of the kernels on every case of the GPU test, and every listed mutation
is rejected."""
import numpy as np
import pytest
import torch

from pytorch_r2d2_amd import lstm_ref as R
from pytorch_r2d2_amd import refnum as rn

FWD = list(R.FORWARD_CASES)
BWD = list(R.BACKWARD_CASES)


def _sp_ok(H):
    return H <= 256


# ---- 1. the untied oracle is the float64 LSTM ------------------------------------------------

def test_untied_oracle_is_float64_lstmcell_and_autograd():
    """Free-running step references == torch.nn.LSTMCell in float64 over 6 steps (1e-12); the
    backward loop == float64 autograd through it with the burn-in steps detached, bias gradient
    included.  Weights go through pack_whh / gate_perm / unpack_cols, so the helpers are checked
    against plain indexing on the way."""
    torch.manual_seed(0)
    H, B, T, t0, D = 32, 5, 6, 2, 7
    cell = torch.nn.LSTMCell(D, H).double()
    x = torch.randn(T, B, D, dtype=torch.float64)
    h0, c0 = torch.randn(B, H, dtype=torch.float64) * 0.3, torch.randn(B, H, dtype=torch.float64) * 0.5
    perm = R.gate_perm(H)
    # plain-indexing definition of the packed order
    for p in (0, 17, 63, 64, 100, 4 * H - 1):
        j, g, u = p // 64, (p % 64) // 16, p % 16
        assert perm[p] == g * H + 16 * j + u
    whh = cell.weight_hh.detach().numpy()
    wpk = R.pack_whh(whh)
    assert wpk.shape == (H // 16, 64, H) and np.array_equal(wpk.reshape(4 * H, H), whh[perm])
    wt = R.pack_whh_t(wpk)
    assert wt.shape == (H // 16, H, 64) and wt[1, 5, 40] == wpk[1, 40, 5]
    bias = (cell.bias_ih + cell.bias_hh).detach()
    xproj = ((x.reshape(T * B, D) @ cell.weight_ih.detach().T + bias).numpy()[:, perm]).reshape(T, B, 4 * H)
    g, c, h = R.free_forward(xproj, wpk.reshape(4 * H, H), h0.numpy(), c0.numpy())
    # torch: burn-in detached, pre-activations kept for their gradients
    hh, cc = h0, c0
    pre, hs = [], []
    for t in range(T):
        if t == t0:
            hh, cc = hh.detach(), cc.detach()
        a = x[t] @ cell.weight_ih.T + cell.bias_ih + cell.bias_hh + hh @ cell.weight_hh.T
        if t >= t0:
            a.retain_grad()
            pre.append(a)
        i, f, gg, o = a.chunk(4, 1)
        cc = torch.sigmoid(f) * cc + torch.sigmoid(i) * torch.tanh(gg)
        hh = torch.sigmoid(o) * torch.tanh(cc)
        hs.append(hh)
        h_ref, c_ref = cell(x[t], (torch.from_numpy(h[t - 1]) if t else h0, torch.from_numpy(c[t - 1]) if t else c0))
        assert np.abs(h_ref.detach().numpy() - h[t]).max() < 1e-12
        assert np.abs(c_ref.detach().numpy() - c[t]).max() < 1e-12
    act = torch.cat([torch.sigmoid(pre[-1][:, :2 * H]), torch.tanh(pre[-1][:, 2 * H:3 * H]),
                     torch.sigmoid(pre[-1][:, 3 * H:])], 1).detach().numpy()
    assert np.abs(R.unpack_cols(g[-1]) - act).max() < 1e-12
    dh_ext = torch.randn(T - t0, B, H, dtype=torch.float64)
    cell.zero_grad()
    sum((hs[t0 + k] * dh_ext[k]).sum() for k in range(T - t0)).backward()
    ref = torch.stack([p.grad for p in pre]).numpy()
    dg = R.free_backward(dh_ext.numpy(), g[t0:], c, c0.numpy(), wpk.reshape(4 * H, H), t0)
    assert np.abs(R.unpack_cols(dg) - ref).max() < 1e-12
    db = np.empty(4 * H)
    db[perm] = dg.sum((0, 1))
    assert np.abs(db - cell.bias_hh.grad.numpy()).max() < 1e-12


def test_number_formats_match_torch():
    x = torch.randn(4096) * torch.logspace(-6, 4, 4096)
    bits = rn.bf16_bits(x.numpy())
    assert np.array_equal(bits.view(np.int16), x.bfloat16().view(torch.int16).numpy())
    hi, lo = rn.split_planes(x.numpy())
    assert np.array_equal(lo, (x - x.bfloat16().float()).bfloat16().float().numpy())
    assert (np.abs(hi.astype(np.float64) + lo - x.numpy()) <= 2.0 ** -17 * x.abs().numpy()).all()
    r = R.round19(x.numpy())
    assert (np.abs(r - x.numpy()) <= 2.0 ** -20 * np.abs(x.numpy())).all()
    assert ((r.view(np.uint32) & 15) == 0).all()


# ---- 2. the fp32 emulation passes every check on every case ----------------------------------

_EMU = {}


def _emu_fwd(name, sp):
    if (name, sp) not in _EMU:
        spec, chains = R.forward_case(name)
        _EMU[(name, sp)] = (spec, chains, [R.emulate_forward(ch, sp, spec["T"]) for ch in chains])
    return _EMU[(name, sp)]


def _emu_bwd(name, sp):
    if (name, sp) not in _EMU:
        spec, bw = R.backward_case(name)
        _EMU[(name, sp)] = (spec, bw, R.emulate_backward(bw, sp))
    return _EMU[(name, sp)]


def _fwd_modes(name):
    return [False, True] if _sp_ok(R.FORWARD_CASES[name]["H"]) else [False]


def _bwd_modes(name):
    spec = R.BACKWARD_CASES[name]
    if spec.get("dz"):
        return [True]
    return [False, True] if _sp_ok(spec["H"]) else [False]


def _view(out, ch):
    """What the entry point would have left for this chain (optional outputs dropped)."""
    o = dict(out)
    if not ch["h32"]:
        o.pop("h32")
    if not ch["gates"]:
        o.pop("gates")
    return o


@pytest.mark.parametrize("name", FWD)
def test_emulated_forward_is_inside_every_bound(name):
    for sp in _fwd_modes(name):
        spec, chains, outs = _emu_fwd(name, sp)
        for c, (ch, out) in enumerate(zip(chains, outs)):
            uses = R.check_forward(f"{name}/{'sp' if sp else 'bf16'}/chain{c}", ch, _view(out, ch), sp)
            print(f"emulation {name} {'sp' if sp else 'bf16'} chain {c}: "
                  + "  ".join(f"{k} {v:.3f}" for k, v in uses.items()))
            assert max(uses.values()) < 1.0


@pytest.mark.parametrize("name", BWD)
def test_emulated_backward_is_inside_every_bound(name):
    for sp in _bwd_modes(name):
        spec, bw, out = _emu_bwd(name, sp)
        label = f"{name}/{'sp' if sp else 'bf16'}"
        use, ref = R.check_backward(label, bw, out, sp)
        ub = R.check_bias_grad(label, bw, out, ref)
        print(f"emulation {label}: dgates {use:.3f}  db {ub:.3f}")
        assert use < 1.0 and ub < 1.0
        if spec.get("no_dh"):
            assert not out["dgates"].any() and not out["db1"].any()


def test_emulated_activations_are_inside_eps_act():
    grid = R.activation_grid()
    col = R.gate_cols(64)
    x = grid.reshape(128, 64)
    gates = np.empty((128, 256), np.float32)
    for q in range(4):
        gates[:, col[q]] = R._tanh32(x) if q == 2 else R._sig32(x)
    us, ut = R.check_activations("sweep", gates, grid)
    print(f"emulation sweep: sigmoid {us:.3f} tanh {ut:.3f}")
    assert us < 1.0 and ut < 1.0
    bad = gates.copy()
    bad[3, col[2][5]] += 2 * R.EPS_TANH
    with pytest.raises(AssertionError, match="tanh"):
        R.check_activations("sweep", bad, grid)


# ---- 3. mutations: the bounds are not too loose ----------------------------------------------

def _fwd_can_show(mut, name, sp):
    s = R.FORWARD_CASES[name]
    T, B, sfs = s["T"], s["B"], s["save_from"]
    saved = [T - sf for c, sf in enumerate(sfs) if c not in s.get("no_gates", ())]
    if mut in ("swap_if", "c_in_t", "slices_swapped", "c_elem_8x", "h32_bf16"):
        return True
    if mut in ("gates_preact", "g_sigmoid"):
        return max(saved) >= 1
    if mut == "save_from_off":
        return max(saved) >= 2
    if mut == "last_row_copy":
        return B > 1
    if mut == "stale_h":
        return T >= 3
    if mut == "chain_c0":
        return len(sfs) >= 2
    if mut == "h_seq_lo_zero":
        return sp
    raise KeyError(mut)


FWD_MUTATIONS = ("swap_if", "c_in_t", "c_elem_8x", "last_row_copy", "slices_swapped", "save_from_off",
                 "gates_preact", "g_sigmoid", "h32_bf16", "h_seq_lo_zero", "chain_c0", "stale_h")


def _check_all_chains(name, sp, chains, outs, mutation=None):
    for c, (ch, out) in enumerate(zip(chains, outs)):
        R.check_forward(f"{name}/chain{c}", ch, _view(out, ch), sp, mutation=mutation)


@pytest.mark.parametrize("mut", FWD_MUTATIONS)
def test_forward_mutation_is_rejected(mut):
    shown = 0
    for name in FWD:
        for sp in _fwd_modes(name):
            if not _fwd_can_show(mut, name, sp):
                continue
            spec, chains, outs = _emu_fwd(name, sp)
            chains = [dict(ch) for ch in chains]
            outs = [{k: v.copy() for k, v in o.items()} for o in outs]
            oracle_mut = mut if mut in R.MUTATIONS_FWD else None
            if mut == "c_elem_8x":     # last valid row of the last batch tile, last step, last unit
                ch, out = chains[-1], outs[-1]
                ref = R.forward_reference(ch, R.forward_operands(ch, sp), out, sp)
                out["c_seq"][-1, -1, -1] += np.float32(8 * ref["e_c"][-1, -1, -1])
            elif mut == "last_row_copy":
                for out in outs:
                    for k in out:
                        out[k][:, -1] = out[k][:, -2]
            elif mut == "h32_bf16":
                for out in outs:
                    out["h32"] = rn.bf16_round(out["h32"])
            elif mut == "h_seq_lo_zero":
                for out in outs:
                    out["h_seq_lo"][:] = 0
                    out["h_seq_lo_bits"][:] = 0
            elif mut == "chain_c0":
                chains[1]["c0"] = chains[0]["c0"]
            with pytest.raises(AssertionError, match=name):
                _check_all_chains(name, sp, chains, outs, oracle_mut)
            shown += 1
    assert shown >= 2


BWD_MUTATIONS = R.MUTATIONS_BWD + R.MUTATIONS_BIAS + ("dgates_lo_zero",)


def _bwd_can_show(mut, name, sp):
    s = R.BACKWARD_CASES[name]
    K, B = s["T"] - s["t0"], s["B"]
    if s.get("no_dh"):
        return False       # every gradient is zero
    if mut in ("tanh_prev", "fgrad_ct"):
        return True
    if mut == "perm_inverse":      # at H 64 (4 slices x 4 gates) the permutation is its own inverse
        return s["H"] != 64
    if mut in ("drop_dc", "no_rec_step", "no_rec_wg"):
        return K >= 2
    if mut == "dh_ext_next":
        return K >= 2
    if mut == "cprev_c0":
        return s["t0"] > 0
    if mut == "dz_first_omitted":
        return bool(s.get("dz"))
    if mut == "dgates_lo_zero":
        return sp
    if mut == "bias_tail_row":
        return B % 16 != 0
    if mut == "bias_no_last_tile":
        return B > 16
    raise KeyError(mut)


@pytest.mark.parametrize("mut", BWD_MUTATIONS)
def test_backward_mutation_is_rejected(mut):
    shown = 0
    for name in BWD:
        for sp in _bwd_modes(name):
            if not _bwd_can_show(mut, name, sp):
                continue
            spec, bw, out = _emu_bwd(name, sp)
            label = f"{name}/{'sp' if sp else 'bf16'}"
            with pytest.raises(AssertionError, match=name):
                if mut in R.MUTATIONS_BIAS:
                    _, ref = R.check_backward(label, bw, out, sp)
                    R.check_bias_grad(label, bw, out, ref, mutation=mut)
                elif mut == "dgates_lo_zero":
                    o = dict(out, dgates_lo=np.zeros_like(out["dgates_lo"]),
                             dgates_lo_bits=np.zeros_like(out["dgates_lo_bits"]))
                    R.check_backward(label, bw, o, sp)
                else:
                    R.check_backward(label, bw, out, sp, mutation=mut)
            shown += 1
    assert shown >= 1


def test_ownership_check_has_teeth():
    pad, n = 8, 24
    buf = np.full(pad + n + pad, np.nan, np.float32)
    valid = np.arange(n) < 16
    buf[pad:pad + 16] = 1.0
    rn.check_ownership("own", "gates", buf, pad, valid)
    for i, what in ((pad - 1, "guard before"), (pad + n, "guard after"), (pad + 20, "does not own")):
        b = buf.copy()
        b[i] = 0.0
        with pytest.raises(AssertionError, match=what):
            rn.check_ownership("own", "gates", b, pad, valid)
    b = buf.copy()
    b[pad + 3] = np.nan
    with pytest.raises(AssertionError, match="not written"):
        rn.check_ownership("own", "gates", b, pad, valid)
    with pytest.raises(AssertionError):
        rn.check_untouched("own", "gates", buf)


@pytest.mark.parametrize("A", [1, 9])
def test_head_grads_emulation_and_mutations(A):
    hc = R.head_case(A)
    for sp in (False, True):
        out = R.emulate_head_grads(hc, sp)
        use = R.check_head_grads(f"b_hg/A{A}", hc, out, sp)
        print(f"emulation b_hg A {A} {'sp' if sp else 'bf16'}: head {use:.3f}")
        assert use < 1.0
        for mut in ("head_halves_swapped", "head_last_row_missing"):
            with pytest.raises(AssertionError, match="b_hg"):
                R.check_head_grads(f"b_hg/A{A}", hc, out, sp, mutation=mut)
    # float64 autograd of the dueling head's last layer gives the same sums
    dva, zr = torch.from_numpy(hc["dva"]).double(), torch.from_numpy(hc["zr"]).double()
    w = torch.zeros(1 + A, hc["HD"], dtype=torch.float64, requires_grad=True)
    b = torch.zeros(1 + A, dtype=torch.float64, requires_grad=True)
    va = torch.cat([zr[:, :hc["HD"]] @ w[:1].T, zr[:, hc["HD"]:] @ w[1:].T], 1) + b
    (va * dva).sum().backward()
    ref = R.head_grads_reference(hc, True)
    assert np.abs(ref["gw2"][0] - w.grad.numpy()).max() < 1e-12
    assert np.abs(ref["gb2"][0] - b.grad.numpy()).max() < 1e-12
