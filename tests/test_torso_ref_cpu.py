"""The conv torso oracle (pytorch_r2d2_amd/torso_ref.py) on the CPU: it is the float64 conv stack
and its autograd, its layouts are ParamLayout's, its bounds admit an fp32/bf16 emulation of the
kernels on every case of the GPU test with no element excluded, and every listed mutation is
rejected."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pytorch_r2d2_amd import refnum as rn
from pytorch_r2d2_amd import torso_ref as R
from pytorch_r2d2_amd.config import get_config
from pytorch_r2d2_amd.engine.layout import ParamLayout

FWD = {c["name"]: c for c in R.FWD_CASES}
BWD = {c["name"]: c for c in R.BWD_CASES}
SP = {c["name"]: c for c in R.SP_CASES}
SPB = {c["name"]: c for c in R.SP_BWD_CASES}
PAD = 64


# ---- 1. the unrounded oracle is the float64 conv stack and its autograd -----------------------

@pytest.mark.parametrize("geom", list(R.GEOMS))
def test_unrounded_oracle_is_float64_conv_stack_and_autograd(geom):
    """layer_reference chained without rounding == F.conv2d in float64 (n = 2); backward_frame's
    values from that forward's activations == autograd's weight and bias gradients."""
    geo, n = R.GEOMS[geom], 2
    wts = R.make_weights(geo, "cpu")
    r = np.random.default_rng(5)
    frames = r.integers(0, 256, (n, geo.cin, geo.h, geo.w), dtype=np.uint8)
    t = {k: torch.tensor(np.asarray(wts[k], np.float64), requires_grad=True) for k in ("w1", "b1", "w2", "b2", "w3", "b3")}
    x = torch.tensor(frames.astype(np.float64) / 255.0)
    r1 = torch.relu(F.conv2d(x, t["w1"], t["b1"], stride=4))
    r2 = torch.relu(F.conv2d(r1, t["w2"], t["b2"], stride=2))
    r3 = torch.relu(F.conv2d(r2, t["w3"], t["b3"]))
    # forward, free running in float64
    p1, _ = R.layer_reference(R.cols_conv1(geo, frames), wts["w1_pk"], wts["b1"], 1.0 / 255.0)
    a1 = np.maximum(p1, 0)
    p2, _ = R.layer_reference(R.cols_hwc(a1, geo.H1, geo.W1, 4, 2), wts["w2_pk"], wts["b2"], 1.0)
    a2 = np.maximum(p2, 0)
    p3, _ = R.layer_reference(R.cols_hwc(a2, geo.H2, geo.W2, 3, 1), wts["w3_pk"], wts["b3"], 1.0)
    o3 = np.maximum(p3, 0).transpose(0, 2, 1)
    hwc = lambda v: v.detach().numpy().transpose(0, 2, 3, 1).reshape(n, -1, 32)  # noqa: E731
    assert np.abs(hwc(r1) - a1).max() < 1e-12
    assert np.abs(hwc(r2) - a2).max() < 1e-12
    assert np.abs(r3.detach().numpy().reshape(n, 32, -1) - o3).max() < 1e-12
    # backward
    dx3 = r.standard_normal((n, geo.OUT))
    (r3.reshape(n, -1) * torch.tensor(dx3)).sum().backward()
    ops = dict(frames=frames, act1=a1, act2=a2, out3=o3.reshape(n, -1), dx3=dx3, w2=wts["w2"], w3=wts["w3"])
    val = sum(R.backward_frame(geo, ops, f)[0] for f in range(n))
    ref = R.pack_slab(geo, t["w1"].grad.numpy() * 255.0, t["w2"].grad.numpy(), t["w3"].grad.numpy(),
                      t["b1"].grad.numpy(), t["b2"].grad.numpy(), t["b3"].grad.numpy())
    assert np.abs(val - ref).max() < 1e-9 * max(1.0, np.abs(ref).max())


# ---- 2. the layouts are ParamLayout's ---------------------------------------------------------

@pytest.mark.parametrize("preset,geom", [("atari57", "atari"), ("dmlab30", "dmlab")])
def test_layouts_match_param_layout(preset, geom):
    """pack_* applied to the master indices of the weights == ParamLayout.bf_index, and slab_map ==
    torso_grad_map(), element for element."""
    cfg = get_config(preset)
    L, geo = ParamLayout(cfg.model, cfg.env), R.GEOMS[geom]
    assert L.cin == geo.cin and L.D == geo.OUT
    idx = {}
    for k, name in (("w1", "vis_layers.0.weight"), ("w2", "vis_layers.2.weight"), ("w3", "vis_layers.4.weight"),
                    ("b1", "vis_layers.0.bias"), ("b2", "vis_layers.2.bias"), ("b3", "vis_layers.4.bias")):
        s = L.segs[name]
        idx[k] = s.offset + np.arange(s.numel, dtype=np.int64).reshape(s.shape)
    bf = L.bf_index.numpy()
    for name, mine in (("conv1", R.pack_conv1(idx["w1"])), ("conv2", R.pack_hwc(idx["w2"])),
                       ("conv3", R.pack_hwc(idx["w3"])), ("conv3_dg", R.pack_conv3_dg(idx["w3"])),
                       ("conv2_dg", R.pack_conv2_dg(idx["w2"]))):
        o, shp = L.bf_offsets[name]
        assert mine.shape == shp, name
        assert np.array_equal(bf[o:o + mine.size], mine.reshape(-1)), name
    dst, scale = L.torso_grad_map()
    mdst, mscale = R.slab_map(geo, {k: int(v.reshape(-1)[0]) for k, v in idx.items()})
    assert dst.numel() == geo.SLAB
    assert np.array_equal(dst.numpy(), mdst) and np.array_equal(scale.numpy(), mscale)


def test_dmlab_odd_extent_rows_carry_no_gradient():
    """DMLab's 17 x 23 conv1 map: conv2 (4 x 4, stride 2) reads rows 0..15 and columns 0..21 only, so
    the last row and column of g1 -- and the phase pixels one past them, which the backward kernel's
    odd-phase-valid bits zero -- are exactly zero whatever g2 and W2 are.  A kernel that did not zero
    those phase pixels would store the same zeros, so no oracle case can tell the two apart, and
    torso_ref has no mutation for it."""
    geo = R.GEOMS["dmlab"]
    r = np.random.default_rng(1)
    g2, w2 = r.standard_normal((geo.H2, geo.W2, 32)), r.standard_normal((32, 32, 4, 4))
    g1 = R._convT2(g2, w2, geo.H1 + 1, geo.W1 + 1)       # one phantom row and column appended
    assert (g1[geo.H1 - 1:] == 0).all() and (g1[:, geo.W1 - 1:] == 0).all()
    assert np.abs(g1[geo.H1 - 2, :geo.W1 - 1]).min() > 0 and np.abs(g1[:geo.H1 - 1, geo.W1 - 2]).min() > 0


def test_worker_deal_and_grid_clamp():
    assert R.deal_workers([3, 2], 4) == [(0, 0, 3), (1, 3, 1)]
    assert R.deal_workers([1, 1], 1) is None                         # the launcher's -3
    assert R.deal_workers([2, 0, 2], 4) == [(0, 0, 2), (2, 2, 2)]
    assert R.deal_workers([4, 3], R.reserve_workers(2, 4)) == [(0, 0, 4), (1, 4, 3)]
    assert [R.effective_grid(g, 3) for g in (0, 9, 3, 2)] == [3, 3, 3, 2]


# ---- 3. the emulation stays within every bound, no element excluded ---------------------------

_EMU = {}


def _emu_fwd(name):
    name = "fwd/" + name
    if name not in _EMU:
        ops = R.forward_operands(FWD[name[4:]])
        _EMU[name] = (ops, [R.emulate_forward(ops["geo"], j["frames"], j["wts"]) if j["n"] else None
                            for j in ops["jobs"]])
    return _EMU[name]


def _emu_bwd(name):
    name = "bwd/" + name
    if name not in _EMU:
        ops = R.backward_operands(BWD[name[4:]])
        slab = R.emulate_backward(ops["geo"], ops, BWD[name[4:]]["grid"])
        grad0 = np.full(ops["grad_numel"], np.nan, np.float32)
        _EMU[name] = (ops, slab, R.emulate_reduce(slab, ops["dst"], ops["scale"], grad0))
    return _EMU[name]


@pytest.mark.parametrize("name", list(FWD))
def test_forward_emulation_within_bounds(name):
    ops, emu = _emu_fwd(name)
    strides = R.forward_strides(FWD[name])
    for j, (job, out) in enumerate(zip(ops["jobs"], emu)):
        if out is None:
            continue
        uses = R.check_forward(f"{name}/job{j}", ops["geo"], job["frames"], job["wts"], out, strides[j])
        for k in ("save1", "save2", "out"):
            rn.check_ownership(name, k, R.guarded_image(out[k], PAD), PAD)
        print(f"torso-oracle: fwd {name}/job{j} " + " ".join(f"{k} {v:.3f}" for k, v in uses.items()))
        assert max(uses.values()) <= 1.0


def _emu_sp(name):
    if name not in _EMU:
        ops = R.forward_sp_operands(SP[name])
        _EMU[name] = (ops, [R.emulate_forward_sp(ops["geo"], j["frames"], j["wts"]) if j["n"] else None
                            for j in ops["jobs"]])
    return _EMU[name]


@pytest.mark.parametrize("name", list(SP))
def test_split_forward_emulation_within_bounds(name):
    ops, emu = _emu_sp(name)
    strides = R.forward_strides(SP[name])
    for j, (job, out) in enumerate(zip(ops["jobs"], emu)):
        if out is None:
            continue
        uses = R.check_forward_sp(f"{name}/job{j}", ops["geo"], job["frames"], job["wts"], out, strides[j])
        print(f"torso-oracle: fwd {name}/job{j} " + " ".join(f"{k} {v:.3f}" for k, v in uses.items()))
        assert max(uses.values()) <= 1.0
        if SP[name]["jobs"][j].get("w1") == "zero":       # act1 = ReLU(b1) exactly, lo plane included
            hi, lo = rn.split_planes(np.maximum(job["wts"]["b1"], 0))
            assert (rn.bf16_val(out["s1"]) == hi).all() and (rn.bf16_val(out["s1_lo"]) == lo).all()


def test_digit_quantisation_error_is_at_most_s_over_32768():
    """The claim of c1_digits' comment, on the emulated digits: |w - s D| <= s / 32768 + 2u|w|."""
    for mode in ("random", "outlier"):
        w = R.make_weights_sp(R.GEOMS["atari"], "digits", mode)["w1_pk"]
        d0, d1, d2, m, _ = R.c1_digits(w)
        s = float(m) / 127.0
        err = np.abs(w - s * (d0 + d1 / 128.0 + d2 / 16384.0))
        assert (err <= s / 32768.0 + 2 * R.U * np.abs(w)).all()
        assert max(np.abs(d0).max(), 2 * np.abs(d1).max(), 2 * np.abs(d2).max()) <= 128


@pytest.mark.parametrize("name", list(BWD))
def test_backward_emulation_within_bounds(name):
    ops, slab, grad = _emu_bwd(name)
    u_slab = R.check_slab(name, ops["geo"], ops, BWD[name]["grid"], slab)
    u_grad = R.check_reduce(name, slab, ops["dst"], ops["scale"], grad)
    torso = np.zeros(grad.size, bool)
    torso[ops["dst"]] = True
    rn.check_ownership(name, "grad", grad, 0, valid=torso)
    print(f"torso-oracle: bwd {name} slab {u_slab:.3f} grad {u_grad:.3f}")
    assert u_slab <= 1.0 and u_grad <= 1.0


def _emu_bwd_sp(name):
    if ("bwd", name) not in _EMU:
        ops = R.backward_sp_operands(SPB[name])
        slab = R.emulate_backward_sp(ops["geo"], ops, SPB[name]["grid"])
        grad0 = np.full(ops["grad_numel"], np.nan, np.float32)
        _EMU[("bwd", name)] = (ops, slab, R.emulate_reduce(slab, ops["dst"], ops["scale"], grad0))
    return _EMU[("bwd", name)]


@pytest.mark.parametrize("name", list(SPB))
def test_split_backward_emulation_within_bounds(name):
    ops, slab, grad = _emu_bwd_sp(name)
    u_slab = R.check_slab(name, ops["geo"], ops, SPB[name]["grid"], slab, sp=True)
    u_grad = R.check_reduce(name, slab, ops["dst"], ops["scale"], grad)
    print(f"torso-oracle: bwd {name} slab {u_slab:.3f} grad {u_grad:.3f}")
    assert u_slab <= 1.0 and u_grad <= 1.0


@pytest.mark.parametrize("mutation", R.MUTATIONS_BWD_SP)
def test_split_backward_mutation_rejected(mutation):
    hit, dense1 = False, False
    for name, case in SPB.items():
        ops, slab, grad = _emu_bwd_sp(name)
        if mutation == "no_255":
            h = _rejects(lambda: R.check_reduce(name, slab, ops["dst"], ops["scale"], grad, mutation))
        else:
            h = _rejects(lambda: R.check_slab(name, ops["geo"], ops, case["grid"], slab, mutation, sp=True))
        hit |= h
        if name.endswith("/n1g1"):
            dense1 = h
    assert hit and dense1, f"{mutation}: rejected by some case {hit}, by the dense n = 1 case {dense1}"


# ---- 4. every mutation is rejected ------------------------------------------------------------

def _rejects(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("mutation", R.MUTATIONS_FWD)
def test_forward_mutation_rejected(mutation):
    geoms = {}
    for name in FWD:
        ops, emu = _emu_fwd(name)
        strides = R.forward_strides(FWD[name])
        for j, (job, out) in enumerate(zip(ops["jobs"], emu)):
            if out is None:
                continue
            if mutation == "pad_lanes_written":     # the padded lanes of conv1's last pixel tile stored
                spill = (-ops["geo"].P1) % 32 * 32
                hit = _rejects(lambda: rn.check_ownership(name, "save1", R.guarded_image(out["save1"], PAD, spill), PAD))
            else:
                hit = _rejects(lambda: R.check_forward(name, ops["geo"], job["frames"], job["wts"], out,
                                                       strides[j], mutation))
            geoms[FWD[name]["geom"]] = geoms.get(FWD[name]["geom"], False) or hit
    assert geoms == {g: True for g in R.GEOMS}, f"{mutation}: no case rejects it on {geoms}"


@pytest.mark.parametrize("mutation", R.MUTATIONS_SP)
def test_split_forward_mutation_rejected(mutation):
    hit = False
    for name in SP:
        ops, emu = _emu_sp(name)
        strides = R.forward_strides(SP[name])
        for j, (job, out) in enumerate(zip(ops["jobs"], emu)):
            if out is None:
                continue
            if mutation == "pad_lanes_written":
                spill = (-ops["geo"].P1) % 32 * 32
                for k in ("s1", "s1_lo"):
                    hit |= _rejects(lambda: rn.check_ownership(name, k, R.guarded_image(out[k], PAD, spill), PAD))
            else:
                hit |= _rejects(lambda: R.check_forward_sp(name, ops["geo"], job["frames"], job["wts"], out,
                                                           strides[j], mutation))
    assert hit, f"{mutation}: no case rejects it"


@pytest.mark.parametrize("mutation", R.MUTATIONS_BWD)
def test_backward_mutation_rejected(mutation):
    geoms, dense1 = {}, {}
    for name, case in BWD.items():
        ops, slab, grad = _emu_bwd(name)
        if mutation == "no_255":
            hit = _rejects(lambda: R.check_reduce(name, slab, ops["dst"], ops["scale"], grad, mutation))
        else:
            hit = _rejects(lambda: R.check_slab(name, ops["geo"], ops, case["grid"], slab, mutation))
        geoms[case["geom"]] = geoms.get(case["geom"], False) or hit
        if name.endswith("/n1g1"):
            dense1[case["geom"]] = hit
    assert geoms == {g: True for g in R.GEOMS}, f"{mutation}: no case rejects it on {geoms}"
    # the dense random case at n = 1: one missing or misplaced tap must exceed the interval bound
    assert dense1 == {g: True for g in R.GEOMS}, f"{mutation}: the dense n = 1 case accepts it ({dense1})"
