"""pytorch_r2d2_amd/optim_ref.py (the float64 reference the GPU optimizer tests compare against)
against torch's own float64 Adam, centered RMSprop and clip_grad_norm_, and proof that the
comparison would catch a wrong reference."""
import numpy as np
import pytest
import torch

from pytorch_r2d2_amd import optim_ref

TOL = 1e-12
LR, EPS, B1, B2, ALPHA, RMS_LR, RMS_EPS = 1e-4, 1e-3, 0.9, 0.999, 0.95, 6.25e-5, 1.5e-7


def _data(n, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n), [rng.standard_normal(n) for _ in range(3)]


def _close(a, b):
    return np.allclose(np.asarray(a), np.asarray(b), rtol=TOL, atol=TOL)


def _max_norm(gs, where):
    """A clip value below every step's norm ('above': clipping active) or above them all."""
    norms = [float(np.sqrt((g * g).sum())) for g in gs]
    return {"above": 0.5 * min(norms), "below": 2.0 * max(norms), "off": 0.0}[where]


def _torch_run(kind, p0, gs, max_norm):
    p = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    if kind == "adam":
        opt = torch.optim.Adam([p], lr=LR, betas=(B1, B2), eps=EPS)
    else:
        opt = torch.optim.RMSprop([p], lr=RMS_LR, alpha=ALPHA, eps=RMS_EPS, centered=True)
    out = []
    for g in gs:
        p.grad = torch.tensor(g, dtype=torch.float64)
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_([p], max_norm)
        opt.step()
        out.append(p.detach().numpy().copy())
    return out


def _ref_run(kind, p0, gs, max_norm, adam=optim_ref.adam_step, rms=optim_ref.rmsprop_centered_step):
    p, a, b = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    out = []
    for t, g in enumerate(gs, 1):
        if kind == "adam":
            p, a, b = adam(p, g, a, b, t, LR, B1, B2, EPS, max_norm)
        else:
            p, a, b = rms(p, g, a, b, RMS_LR, ALPHA, RMS_EPS, max_norm)
        out.append(p)
    return out


@pytest.mark.parametrize("where", ["off", "below", "above"])
@pytest.mark.parametrize("n", [1, 7, 4099])
@pytest.mark.parametrize("kind", ["adam", "rmsprop_centered"])
def test_optim_ref_matches_torch_float64(kind, n, where):
    """3 steps, the norm below and above the clip value (and no clipping)."""
    p0, gs = _data(n)
    mx = _max_norm(gs, where)
    want, got = _torch_run(kind, p0, gs, mx), _ref_run(kind, p0, gs, mx)
    for t in range(3):
        assert _close(got[t], want[t]), (t, np.abs(got[t] - want[t]).max())


@pytest.mark.parametrize("n", [1, 7, 4099])
def test_clip_scale_matches_clip_grad_norm(n):
    _, gs = _data(n, seed=1)
    g = gs[0]
    for where in ("below", "above"):
        mx = _max_norm([g], where)
        t = torch.tensor(g, dtype=torch.float64, requires_grad=True)
        t.grad = torch.tensor(g, dtype=torch.float64)
        norm = torch.nn.utils.clip_grad_norm_([t], mx)
        assert abs(optim_ref.grad_norm(g) - float(norm)) <= TOL * float(norm)
        assert _close(g * optim_ref.clip_scale(g, mx), t.grad.numpy())
        assert (optim_ref.clip_scale(g, mx) < 1.0) == (where == "above")
    # the data-parallel average: the norm is taken of the scaled gradient
    assert abs(optim_ref.clip_scale(g, 0.0, 0.25) - 0.25) == 0.0
    assert abs(optim_ref.grad_norm(g, 0.5) - 0.5 * optim_ref.grad_norm(g)) <= TOL


def test_mutated_references_are_rejected():
    """The comparison above has teeth: eps inside the sqrt, a clip scale applied below the clip
    value, and a first step counted as 0 each miss the tolerance by orders of magnitude."""
    p0, gs = _data(4099)

    def adam_eps_inside(p, g, m, v, t, lr, b1, b2, eps, max_norm=0.0, gscale=1.0):
        gr = g * optim_ref.clip_scale(g, max_norm, gscale)
        m = b1 * m + (1 - b1) * gr
        v = b2 * v + (1 - b2) * gr * gr
        return p - (lr / (1 - b1 ** t)) * m / np.sqrt(v / (1 - b2 ** t) + eps), m, v

    def adam_step_late(p, g, m, v, t, *a, **k):
        return optim_ref.adam_step(p, g, m, v, t + 1, *a, **k)

    def rms_always_scaled(p, g, sq, ga, lr, alpha, eps, max_norm=0.0, gscale=1.0):
        s = max_norm / (optim_ref.grad_norm(g) + optim_ref.CLIP_EPS) if max_norm > 0 else 1.0
        return optim_ref.rmsprop_centered_step(p, g * s, sq, ga, lr, alpha, eps)

    def rms_eps_inside(p, g, sq, ga, lr, alpha, eps, max_norm=0.0, gscale=1.0):
        sq = alpha * sq + (1 - alpha) * g * g
        ga = alpha * ga + (1 - alpha) * g
        return p - lr * g / np.sqrt(sq - ga * ga + eps), sq, ga

    want = _torch_run("adam", p0, gs, 0.0)
    for bad in (adam_eps_inside, adam_step_late):
        got = _ref_run("adam", p0, gs, 0.0, adam=bad)
        assert not all(_close(got[t], want[t]) for t in range(3)), bad.__name__
    want = _torch_run("rmsprop_centered", p0, gs, 0.0)
    got = _ref_run("rmsprop_centered", p0, gs, 0.0, rms=rms_eps_inside)
    assert not all(_close(got[t], want[t]) for t in range(3))
    mx = _max_norm(gs, "below")         # no step is clipped: the scale must stay 1
    want = _torch_run("rmsprop_centered", p0, gs, mx)
    got = _ref_run("rmsprop_centered", p0, gs, mx, rms=rms_always_scaled)
    assert not all(_close(got[t], want[t]) for t in range(3))
    assert all(_close(a, b) for a, b in zip(_ref_run("rmsprop_centered", p0, gs, mx), want))
