"""The launches of the acting path (``infer.PolicyInference.run``) without a GPU: the kernel
library, the stream, the GEMM launchers and the fused torso, as the inference module sees them, are
recorders, and every case asserts the recorded sequence -- which launcher, how many jobs / chains,
and every word of every job row (pointer words = ``data_ptr()`` of the named buffer plus the
row-half byte offset; reserved words 0).  Written against the free functions this class replaced
(``actor_batched.infer_nets``), where it passed; only ``_inference`` below was ported."""
import types

import pytest
import torch

from pytorch_r2d2_amd import infer as mod
from pytorch_r2d2_amd.config import get_config

STREAM, GEOM, WORKERS, CTR_WORDS = 0x5EED, (4, 84, 84), 24, 6
PK_KEYS = ("conv1", "b1", "conv2", "b2", "conv3", "b3", "w_ih", "w_hh", "head1", "head_b1", "head_w2",
           "head_b2")


class _Kernels:
    """Every ``r2_*`` entry records (name, args) and returns 0."""

    def __init__(self, rec):
        self.rec = rec

    def r2_lstm_persist_ctr_words(self):
        return CTR_WORDS

    def __getattr__(self, name):
        return lambda *a: self.rec.append((name, a)) or 0


def _weights(lo: bool):
    """Stand-in weights: tiny tensors under the real key names."""
    planes = lambda dt: {k: torch.zeros(2, 2, dtype=dt) for k in PK_KEYS}  # noqa: E731
    return types.SimpleNamespace(pk=planes(torch.bfloat16), pk_lo=planes(torch.bfloat16) if lo else None,
                                 lstm_b=torch.zeros(2), flat=torch.zeros(2))


def _inference(monkeypatch, rec, n, E, fp32, lstm_step):
    """(inference object on the CPU device with forced fused torso, its nets, its run callable)."""
    monkeypatch.setattr(mod, "kernels", lambda: _Kernels(rec))
    monkeypatch.setattr(mod, "stream_handle", lambda: STREAM)
    monkeypatch.setattr(mod, "gemm", lambda *p: rec.append(("gemm", p)))
    monkeypatch.setattr(mod, "gemm_sp", lambda p, **kw: rec.append(("gemm_sp", (p, kw))))
    monkeypatch.setattr(mod, "torso_fwd_fused", lambda *a: rec.append(("torso_fwd_fused", a)))
    cfg = get_config("atari57", **{"model.hidden": 64, "actor.compute_dtype": "fp32" if fp32 else "bf16"})
    env = types.SimpleNamespace(E=E, frames=torch.zeros(E, 4, 84, 84, dtype=torch.uint8))
    keys = ("on", "tg")[:n]
    o = mod.PolicyInference(cfg, env, keys, "actor.compute_dtype", "cpu")
    o.fused_torso, o.fwd_geom = True, GEOM
    o.lstm_step, o.n_workers = lstm_step, WORKERS
    if fp32:
        o.sp_ws = {site: (torch.zeros(4), torch.zeros(4, dtype=torch.int32)) for site in ("xproj", "heads")}
    nets = tuple((k, _weights(fp32)) for k in keys)
    return o, nets, lambda: o.run(nets)


def _rows(arr, addr, n, words):
    """The job array a launcher was given: kept alive on the object, ``n`` rows of ``words``."""
    assert arr.ctypes.data == addr and arr.shape == (n, words) and arr.dtype.name == "int64"
    return arr.tolist()


def _p(t, off=0):
    return t.data_ptr() + off


def _check_gemm(problems, o, nets, a, b, c, bias, a_lo=None):
    assert len(problems) == len(nets)
    for p, (key, w) in zip(problems, nets):
        assert p.a is a[key] and p.c is c[key] and _p(p.b) == _p(w.pk[b]) and p.b.shape == w.pk[b].t().shape
        assert (p.bias is w.lstm_b) if bias else (p.bias is None)
        if a_lo is None:
            assert p.a_lo is None and p.b_lo is None
        else:
            assert p.a_lo is a_lo[key] and _p(p.b_lo) == _p(w.pk_lo[b])
        assert p.c_lo is None and p.crow is None and not p.accumulate and p.alpha == 1.0


def _check_chains(rows, o, nets, h0, Bc, lo):
    """One row per net and row range of Bc rows: LstmChain / PChain words."""
    E, H, G = o.E, o.H, o.layout.G
    want = []
    for key, w in nets:
        for r0 in range(0, E, Bc):
            row = [_p(o.xp[key], r0 * G * 4), _p(w.pk["w_hh"]), _p(h0[key], r0 * H * h0[key].element_size()),
                   _p(o.c[key], r0 * H * 4), _p(o.h_bf_new[key], r0 * H * 2), _p(o.c_new[key], r0 * H * 4),
                   _p(o.h32_new[key], r0 * H * 4), 0, 0]
            if lo:
                row += [_p(w.pk_lo["w_hh"]), _p(o.h_lo_new[key], r0 * H * 2)]
            want.append(row)
    assert rows == want


def _check_duel(rec, name, o, nets):
    got, a = rec
    assert got == name and a[1:] == (len(nets), o.A, o.layout.HD, STREAM)
    assert _rows(o._djobs, a[0], len(nets), 7) == [
        [_p(o.zh[key]), _p(w.pk["head_b1"]), _p(w.pk["head_w2"]), _p(w.pk["head_b2"]), _p(o.q[key]), 0, o.E]
        for key, w in nets]


def _halves(E):
    return (E, 1) if E <= 128 else (E // 2, 2)


SHAPES = [(n, E) for n in (1, 2) for E in (4, 128, 130, 256)]


@pytest.mark.parametrize("n,E", SHAPES)
@pytest.mark.parametrize("lstm_step", [False, True])
def test_bf16_launches(monkeypatch, n, E, lstm_step):
    rec = []
    o, nets, run = _inference(monkeypatch, rec, n, E, False, lstm_step)
    assert not o.sp and o.zh["on"].dtype == torch.bfloat16 and o.ctr.numel() == CTR_WORDS
    run()
    assert [r[0] for r in rec] == ["torso_fwd_fused", "gemm", "r2_lstm_fwd" if lstm_step else "r2_lstm_fwd_persist",
                                   "gemm", "r2_dueling_fwd_multi"]
    frames, tj, geom, workers, s = rec[0][1]
    assert _p(frames) == _p(o.env.frames) and frames.shape == (E, 4 * 84 * 84)
    assert tj is o._tjobs and (geom, workers, s) == (GEOM, WORKERS, STREAM)
    assert _rows(tj, tj.ctypes.data, n, 12) == [
        [0, E, _p(w.pk["conv1"]), _p(w.pk["b1"]), _p(w.pk["conv2"]), _p(w.pk["b2"]), _p(w.pk["conv3"]),
         _p(w.pk["b3"]), _p(o.Xn[key]), 0, 0, 0] for key, w in nets]
    _check_gemm(rec[1][1], o, nets, o.Xn, "w_ih", o.xp, bias=True)
    a = rec[2][1]
    if lstm_step:
        Bc, halves = _halves(E)
        assert a[1:] == (n * halves, Bc, 1, o.H, 0, STREAM)
        _check_chains(_rows(o._chains, a[0], n * halves, 9), o, nets, o.h_bf, Bc, lo=False)
    else:
        assert a[1:] == (n, E, 1, o.H, _p(o.ctr), _p(o.err), STREAM)
        _check_chains(_rows(o._chains, a[0], n, 9), o, nets, o.h_bf, E, lo=False)
    _check_gemm(rec[3][1], o, nets, o.h_bf_new, "head1", o.zh, bias=False)
    _check_duel(rec[4], "r2_dueling_fwd_multi", o, nets)


@pytest.mark.parametrize("n,E", SHAPES)
@pytest.mark.parametrize("lstm_step", [False, True])
def test_fp32_launches(monkeypatch, n, E, lstm_step):
    """The split-precision stages, whatever ``lstm_step`` says."""
    rec = []
    o, nets, run = _inference(monkeypatch, rec, n, E, True, lstm_step)
    assert o.sp and o.zh["on"].dtype == torch.float32
    run()
    assert [r[0] for r in rec] == ["r2_torso_fwd_sp_multi", "gemm_sp", "r2_lstm_fwd_sp", "gemm_sp",
                                   "r2_dueling_fwd_multi_f32"]
    a = rec[0][1]
    assert (a[0],) + a[2:] == (_p(o.env.frames), n, WORKERS, STREAM)
    assert _rows(o._tjobs, a[1], n, 20) == [
        [0, E, _p(w.pk["conv1"]), _p(w.pk_lo["conv1"]), _p(w.pk["b1"]), _p(w.pk["conv2"]), _p(w.pk_lo["conv2"]),
         _p(w.pk["b2"]), _p(w.pk["conv3"]), _p(w.pk_lo["conv3"]), _p(w.pk["b3"]), _p(o.Xn[key]),
         _p(o.Xn_lo[key]), 0, 0, 0, 0, 0, 0, 0] for key, w in nets]
    for i, site, args in ((1, "xproj", (o.Xn, "w_ih", o.xp, True, o.Xn_lo)),
                          (3, "heads", (o.h_bf_new, "head1", o.zh, False, o.h_lo_new))):
        problems, kw = rec[i][1]
        _check_gemm(problems, o, nets, *args)
        assert set(kw) == {"splits", "ws", "tickets", "n_cus"} and kw["splits"] == [0] * n
        assert kw["ws"] is o.sp_ws[site][0] and kw["tickets"] is o.sp_ws[site][1] and kw["n_cus"] == WORKERS
    Bc, halves = _halves(E)
    a = rec[2][1]
    assert a[1:] == (n * halves, Bc, 1, o.H, 0, STREAM)
    _check_chains(_rows(o._chains, a[0], n * halves, 11), o, nets, o.h32, Bc, lo=True)
    _check_duel(rec[4], "r2_dueling_fwd_multi_f32", o, nets)


@pytest.mark.parametrize("fp32", [False, True])
def test_an_odd_group_above_128_envs_is_refused(monkeypatch, fp32):
    o, nets, run = _inference(monkeypatch, [], 2, 129, fp32, True)
    with pytest.raises(ValueError, match="step-kernel LSTM: E <= 128 or an even E <= 256"):
        run()
