"""Adam and gradient-norm clipping on the fast learner path (csrc/kernels/optim.hip
r2_grad_sumsq / r2_adam_pack / r2_adam_pack_slab, engine/learner_engine.py ``_update``): the
deterministic clip norm against its a-priori error bound, the Adam pack kernels against the
kernels they fuse (bit for bit), and the engine -- hoisted == plain bitwise with either optimizer
and an active clip, an inactive clip free of side effects, one step against the float64 reference
(pytorch_r2d2_amd/optim_ref.py), resume."""
import functools
import math

import numpy as np
import pytest
import torch

from pytorch_r2d2_amd import optim_ref
from pytorch_r2d2_amd.config import get_config
from pytorch_r2d2_amd.engine.layout import ParamLayout
from pytorch_r2d2_amd.ops._lib import kernels, ptr, stream_handle

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
U = 2.0 ** -24            # fp32 unit roundoff
GSQ_MAX_FLAT = 256        # optim.hip: flat workgroups of the norm launch, 256 threads each


# ------------------------------------------------------------------ the norm kernel
def _gsq_chain(quads: int, tblocks: int = 0) -> int:
    """Longest chain of additions of grad_sumsq_kernel, from the summation tree its comment in
    optim.hip documents: per-thread accumulator steps + 2 (the four accumulators), wave 6 + block
    3, then the final stage over the T + F partials: per-thread steps, wave 6 + block 3."""
    F = min(GSQ_MAX_FLAT, -(-quads // 256))
    per_thread = -(-quads // (F * 256)) if F else 0
    return per_thread + 2 + 9 + -(-(tblocks + F) // 256) + 9


def _gsq_bound(quads: int, tblocks: int = 0) -> float:
    """Relative error of a sum of non-negative terms along a tree of depth d, each product
    rounded at most once: gamma_(d+1) = (d + 1) u / (1 - (d + 1) u)."""
    d = _gsq_chain(quads, tblocks)
    return (d + 1) * U / (1 - (d + 1) * U)


class _Gsq:
    def __init__(self):
        self.k = kernels()
        self.part = torch.zeros(int(self.k.r2_grad_sumsq_partials()), device=DEV)
        self.ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.out = torch.zeros(1, device=DEV)

    def __call__(self, g, fold=None):
        """One launch with the outputs NaN-poisoned; returns the bits of *out."""
        self.part.fill_(float("nan"))
        self.out.fill_(float("nan"))
        if fold is None:
            args = (0, 0, 0, 0, 0, 0, 0)
        else:
            slab, G, SL, dst, scale, tq = fold
            args = (ptr(slab), G, SL, ptr(dst), ptr(scale), ptr(g), tq)
        assert self.k.r2_grad_sumsq(ptr(g), g.numel(), ptr(self.out), ptr(self.part),
                                    ptr(self.ticket), *args, stream_handle()) == 0
        torch.cuda.synchronize()
        assert int(self.ticket.item()) == 0, "the last arriver resets the ticket"
        return self.out.clone()


def _atari_layout():
    cfg = get_config("atari57")
    return ParamLayout(cfg.model, cfg.env)


@pytest.mark.parametrize("n", [4, 252, 1024 * 4 + 4, "padded"])
def test_grad_sumsq_is_deterministic_and_within_its_bound(n):
    """10 launches on the same buffers: identical bits, ticket back to 0 each time; the value
    within the a-priori bound of the documented summation tree of a float64 sum."""
    n = _atari_layout().padded if n == "padded" else n
    torch.manual_seed(n)
    g = torch.randn(n, device=DEV) * 1e-3
    run = _Gsq()
    outs = [run(g) for _ in range(10)]
    assert all(torch.equal(outs[0].view(torch.int32), o.view(torch.int32)) for o in outs)
    ref = float((g.double() ** 2).sum().item())
    got = float(outs[0].item())
    err = abs(got - ref) / ref
    err_torch = abs(float((g * g).sum().item()) - ref) / ref
    bound = _gsq_bound(n // 4)
    print(f"n={n} d={_gsq_chain(n // 4)} bound={bound:.3e} kernel_err={err:.3e} torch_fp32_err={err_torch:.3e}")
    assert err <= bound, (err, bound)


def test_grad_sumsq_refuses_bad_arguments():
    run = _Gsq()
    g = torch.zeros(8, device=DEV)
    k, s = run.k, stream_handle()
    none = (0, 0, 0, 0, 0, 0, 0)
    assert k.r2_grad_sumsq(ptr(g), 6, ptr(run.out), ptr(run.part), ptr(run.ticket), *none, s) == -1
    assert k.r2_grad_sumsq(ptr(g) + 4, 4, ptr(run.out), ptr(run.part), ptr(run.ticket), *none, s) == -1
    assert k.r2_grad_sumsq(ptr(g), 8, ptr(run.out), ptr(run.part), ptr(run.ticket),
                           ptr(g), 1, 4, 0, 0, ptr(g), 1, s) == -1       # slabs without a map
    assert k.r2_grad_sumsq(ptr(g), 8, ptr(run.out), ptr(run.part), ptr(run.ticket),
                           ptr(g), 1, 4, ptr(g), ptr(g), ptr(g), 3, s) == -1     # 4 * tq > n


@pytest.mark.parametrize("SL", [17, 64, 200])
@pytest.mark.parametrize("G", [1, 5, 68])
def test_grad_sumsq_slab_section(G, SL):
    """Synthetic slabs (G: the 64-slab unrolled loop and its remainder), a random permutation as
    destination map, random scales; the flat part [0, 4 tq) and the torso part tile the vector."""
    tq = 300                                  # two flat workgroups
    region = (SL + 3 + 3) // 4 * 4            # the torso part, with >= 3 elements outside dst
    n = 4 * tq + region
    gen = torch.Generator(device="cpu").manual_seed(1000 * G + SL)
    slab = (torch.rand(G, SL, generator=gen) + 0.1).to(DEV)           # all positive
    scale = (torch.rand(SL, generator=gen) + 0.5).to(DEV)
    dst = (4 * tq + torch.randperm(region, generator=gen)[:SL]).to(torch.int32).to(DEV)
    g0 = torch.randn(n, generator=gen).to(DEV) * 1e-3
    g0[4 * tq:] = 7.0                         # sentinel: never read, overwritten only at dst
    g = g0.clone()
    run = _Gsq()
    out = run(g, (slab, G, SL, dst, scale, tq))
    # gw[dst] = column sum * scale: a serial sum of G positive terms and one product
    want = slab.double().sum(0) * scale.double()
    got = g[dst.long()].double()
    rel = ((got - want).abs() / want).max().item()
    assert rel <= G * U, (rel, G * U)
    # nothing else moved
    keep = torch.ones(n, dtype=torch.bool, device=DEV)
    keep[dst.long()] = False
    assert torch.equal(g[keep], g0[keep])
    # *out: the flat part and every torso element as written, each once
    ref = float((g[:4 * tq].double() ** 2).sum() + (got ** 2).sum())
    err = abs(float(out.item()) - ref) / ref
    bound = _gsq_bound(tq, -(-SL // 64))
    print(f"G={G} SL={SL} bound={bound:.3e} kernel_err={err:.3e} colsum_err={rel:.3e}")
    assert err <= bound, (err, bound)
    # and again on the same buffers: the same bits
    assert torch.equal(run(g, (slab, G, SL, dst, scale, tq)).view(torch.int32), out.view(torch.int32))


@pytest.mark.parametrize("G", [3, 68])
def test_grad_sumsq_slab_section_is_bitwise_torso_grad_reduce(G):
    L = _atari_layout()
    k, s = kernels(), stream_handle()
    SL = int(k.r2_torso_bwd_slab_floats())
    dst, scale = (t.to(DEV) for t in L.torso_grad_map())
    assert dst.numel() == SL and L.torso_offset % 4 == 0
    torch.manual_seed(G)
    slab = torch.randn(G, SL, device=DEV) * 1e-3
    g = torch.randn(L.padded, device=DEV) * 1e-3
    g[L.torso_offset:] = 0
    ref = g.clone()
    assert k.r2_torso_grad_reduce(ptr(slab), G, ptr(dst), ptr(scale), ptr(ref), s) == 0
    run = _Gsq()
    out = run(g, (slab, G, SL, dst, scale, L.torso_offset // 4))
    assert torch.equal(g, ref)
    want = float((ref.double() ** 2).sum().item())
    assert abs(float(out.item()) - want) / want <= _gsq_bound(L.torso_offset // 4, -(-SL // 64))


# ------------------------------------------------------------------ the Adam pack kernels
ADAM = (1e-4, 0.9, 0.999, 1e-3)     # lr, b1, b2, eps


class _Bufs:
    """Master, moments, target, packs of one arm."""

    def __init__(self, L, sp, p0, m0, v0):
        n, nb = L.padded, (2 * L.bf_numel if sp else L.bf_numel)
        z = lambda k, dt=torch.float32: torch.zeros(k, dtype=dt, device=DEV)  # noqa: E731
        self.p, self.m, self.v = p0.clone(), m0.clone(), v0.clone()
        self.tgt = z(n)
        self.bf, self.bft = z(nb, torch.bfloat16), z(nb, torch.bfloat16)
        self.f32, self.f32t = z(L.f_numel), z(L.f_numel)
        self.lb, self.lbt = z(L.G), z(L.G)

    def named(self):
        return dict(p=self.p, m=self.m, v=self.v, target=self.tgt, bf=self.bf, bf_t=self.bft,
                    f32=self.f32, f32_t=self.f32t, lb=self.lb, lb_t=self.lbt)


def _pack_step(k, L, b, idx, fidx, rows_done, step, interval, lo, s):
    n_master, n_bf = (0, L.bf_rows_begin) if rows_done else (L.padded, L.bf_numel)
    assert k.r2_pack_step(ptr(b.p), ptr(b.tgt), n_master, ptr(idx), ptr(b.bf), ptr(b.bft), n_bf,
                          ptr(fidx), ptr(b.f32), ptr(b.f32t), L.f_numel, L.f_offsets["b_ih"][0],
                          L.f_offsets["b_hh"][0], ptr(b.lb), ptr(b.lbt), L.G, ptr(step), interval,
                          lo, s) == 0


def _real_mask(L, sp):
    # padding slots of the packs (no master element) are not written by the fused path
    real = torch.ones(L.bf_numel, dtype=torch.bool, device=DEV)
    real[L.bf_rows_begin:] = L.bf_index[L.bf_rows_begin:].to(DEV) != L.segs["lstm.bias_ih"].offset
    return torch.cat([real, real]) if sp else real


def _diff(a, b, real):
    bad = []
    for name, x in a.named().items():
        y = b.named()[name]
        if name in ("bf", "bf_t"):
            x, y = x[real], y[real]
        if x.dtype == torch.bfloat16:
            x, y = x.view(torch.int16), y.view(torch.int16)
        if not torch.equal(x, y):
            bad.append(name)
    return bad


@pytest.mark.parametrize("clip", ["active", "inactive"])
@pytest.mark.parametrize("sp,due", [(True, False), (True, True), (False, True)])
def test_adam_pack_matches_adam_then_gather(sp, due, clip):
    """r2_adam_pack + the prefix pack launch == r2_adam + the full pack launch, bit for bit, over
    3 consecutive steps (interval 2: due and not-due steps alternate), with the clip above and
    below the norm; step_off 0 on a pre-advanced counter (the due decision baked into the
    interval, as the hoisted step does) == step_off 1."""
    L = _atari_layout()
    assert L.row_dst4 is not None
    n = L.padded
    torch.manual_seed(0)
    p0 = torch.randn(n, device=DEV) * 0.05
    m0 = torch.randn(n, device=DEV) * 1e-4
    v0 = torch.rand(n, device=DEV) * 1e-6 + 1e-7
    idx, fidx, dst4 = L.bf_index.to(DEV), L.f_index.to(DEV), L.row_dst4.to(DEV)
    lo = L.bf_numel if sp else 0
    k, s = kernels(), stream_handle()
    lr, b1, b2, eps = ADAM
    ref, one, zero = (_Bufs(L, sp, p0, m0, v0) for _ in range(3))
    real = _real_mask(L, sp)
    sumsq = torch.zeros(1, device=DEV)
    first = 1 if due else 0
    due_seen = []
    for t in range(first, first + 3):
        g = torch.randn(n, device=DEV) * 1e-3
        sumsq[0] = (g.double() ** 2).sum().float()
        norm = float(sumsq.item()) ** 0.5
        mx = 0.5 * norm if clip == "active" else 2.0 * norm
        step = torch.tensor([t], dtype=torch.int64, device=DEV)
        step_adv = step + 1
        is_due = (t + 1) % 2 == 0
        due_seen.append(is_due)
        baked = 1 if is_due else 1 << 62
        assert k.r2_adam(ptr(ref.p), ptr(g), ptr(ref.m), ptr(ref.v), n, lr, b1, b2, eps, 1.0,
                         ptr(step), ptr(sumsq), mx, s) == 0
        _pack_step(k, L, ref, idx, fidx, False, step, 2, lo, s)
        assert k.r2_adam_pack(ptr(one.p), ptr(g), ptr(one.m), ptr(one.v), n, lr, b1, b2, eps, 1.0,
                              ptr(sumsq), mx, ptr(dst4), ptr(one.bf), ptr(one.bft), lo,
                              ptr(one.tgt), ptr(step), 2, 1, s) == 0
        _pack_step(k, L, one, idx, fidx, True, step, 2, lo, s)
        assert k.r2_adam_pack(ptr(zero.p), ptr(g), ptr(zero.m), ptr(zero.v), n, lr, b1, b2, eps,
                              1.0, ptr(sumsq), mx, ptr(dst4), ptr(zero.bf), ptr(zero.bft), lo,
                              ptr(zero.tgt), ptr(step_adv), baked, 0, s) == 0
        _pack_step(k, L, zero, idx, fidx, True, step_adv, baked, lo, s)
        torch.cuda.synchronize()
        assert not _diff(ref, one, real), (t, _diff(ref, one, real))
        assert not _diff(ref, zero, real), (t, _diff(ref, zero, real))
        if is_due:
            assert torch.equal(one.tgt, one.p) and one.bft.abs().sum() > 0
    assert True in due_seen and False in due_seen
    assert not torch.equal(ref.p, p0)


@pytest.mark.parametrize("G", [3, 68])
def test_adam_pack_slab_matches_reduce_then_adam_pack(G):
    """r2_adam_pack_slab == r2_torso_grad_reduce + r2_adam_pack, bitwise: master, moments, packs,
    target and the gradient buffer, over a not-due and a due step."""
    L = _atari_layout()
    n, tq = L.padded, L.torso_offset // 4
    k, s = kernels(), stream_handle()
    SL = int(k.r2_torso_bwd_slab_floats())
    dst, scale = (t.to(DEV) for t in L.torso_grad_map())
    dst4 = L.row_dst4.to(DEV)
    assert bool((L.row_dst4[tq:] < 0).all())
    torch.manual_seed(7 + G)
    pad = torch.ones(n, dtype=torch.bool, device=DEV)      # master elements that are padding
    pad[:L.torso_offset] = False
    pad[dst.long()] = False
    p0 = torch.randn(n, device=DEV) * 0.05
    p0[pad] = 0
    m0 = torch.randn(n, device=DEV) * 1e-4
    v0 = torch.rand(n, device=DEV) * 1e-6 + 1e-7
    m0[pad] = 0
    v0[pad] = 0
    lo = L.bf_numel
    lr, b1, b2, eps = ADAM
    a, b = _Bufs(L, True, p0, m0, v0), _Bufs(L, True, p0, m0, v0)
    real = _real_mask(L, True)
    for t in (0, 1):
        slab = torch.randn(G, SL, device=DEV) * 1e-3
        ga = torch.randn(n, device=DEV) * 1e-3
        ga[L.torso_offset:] = 0
        gb = ga.clone()
        step = torch.tensor([t], dtype=torch.int64, device=DEV)
        assert k.r2_torso_grad_reduce(ptr(slab), G, ptr(dst), ptr(scale), ptr(ga), s) == 0
        assert k.r2_adam_pack(ptr(a.p), ptr(ga), ptr(a.m), ptr(a.v), n, lr, b1, b2, eps, 1.0, 0, 0.0,
                              ptr(dst4), ptr(a.bf), ptr(a.bft), lo, ptr(a.tgt), ptr(step), 2, 1,
                              s) == 0
        assert k.r2_adam_pack_slab(ptr(b.p), ptr(gb), ptr(b.m), ptr(b.v), n, lr, b1, b2, eps, 1.0,
                                   ptr(dst4), ptr(b.bf), ptr(b.bft), lo, ptr(b.tgt), ptr(step), 2,
                                   1, ptr(slab), G, SL, ptr(dst), ptr(scale), tq, s) == 0
        torch.cuda.synchronize()
        assert not _diff(a, b, real), (t, _diff(a, b, real))
        assert torch.equal(ga, gb)
    assert torch.equal(b.tgt, b.p)


# ------------------------------------------------------------------ the engine
def _engine(hoist, B=16, interval=3, graph=True, **kw):
    from pytorch_r2d2_amd.engine.learner_engine import LearnerEngine
    from pytorch_r2d2_amd.engine.replay_hbm import HBMReplay
    over = {"seed": 1234, "learner.batch_size": B, "learner.hoist": hoist,
            "learner.target_update_interval": interval, "learner.use_graph": graph}
    over.update(kw)
    cfg = get_config("atari57", **over)
    rp = HBMReplay(cfg, DEV, capacity=64000)
    rp.fill_synthetic(episode_len=200, seed=3)
    eng = LearnerEngine(cfg, rp, DEV)
    return rp, eng


def _state(rp, eng):
    # the packed layouts by name (their alignment padding is never read and not compared)
    out = {"master": eng.master, "target": eng.target, "opt_a": eng.opt_a, "opt_b": eng.opt_b,
           "lstm_b": eng.lstm_b, "lstm_b_t": eng.lstm_b_t, "priority": rp.priority,
           "tree": rp.tree, "step": rp.step, "loss": eng.loss, "grad": eng.grad}
    for tag, (bf, f32) in {"": (eng.bf, eng.f32), "_t": (eng.bf_t, eng.f32_t)}.items():
        for plane in range(bf.shape[0]):
            for k, v in eng.layout.packed_views(bf[plane], f32).items():
                out["%s%s.%d" % (k, tag, plane)] = v
    return out


def _opt(optimizer, clip):
    return {"learner.optimizer": optimizer, "learner.lr": 1e-4, "learner.eps": 1e-3,
            "learner.grad_clip": clip}


def _same(rp0, a, rp1, b, where):
    sa, sb = _state(rp0, a), _state(rp1, b)
    bad = [k for k in sa if not torch.equal(sa[k], sb[k])]
    assert not bad, (where, bad)


@functools.lru_cache(maxsize=None)
def _clip_from_data(optimizer: str, B: int) -> float:
    """Half the smallest pre-clip gradient norm of 10 plain steps taken with a clip too large to
    act: a clip value that is active at every step of a run from the same start."""
    rp, eng = _engine(False, B=B, graph=False, **_opt(optimizer, 1e30))
    norms = []
    for _ in range(10):
        eng.step()
        norms.append(eng.diagnostics()["grad_norm"])
    assert all(math.isfinite(x) and x > 0 for x in norms), norms
    return 0.5 * min(norms)


@pytest.mark.parametrize("optimizer", ["adam", "rmsprop_centered"])
@pytest.mark.parametrize("graph,B,early", [(True, 16, False), (False, 8, False), (True, 16, True)])
def test_hoisted_step_with_adam_and_clip_is_bitwise_the_plain_step(graph, B, early, optimizer):
    """10 steps, target sync every 3, one invalidation at step 6, the clip active at every step:
    every entry of the state and the gradient equal the plain engine's after every step."""
    c = _clip_from_data(optimizer, B)
    kw = _opt(optimizer, c)
    rp0, plain = _engine(False, B=B, graph=graph, **kw)
    rp1, hoist = _engine(True, B=B, graph=graph, **{"learner.hoist_early_fork": early}, **kw)
    assert hoist.hoist and not plain.hoist
    if graph:
        plain.capture(warmup=0)
        hoist.capture(warmup=0)
    for i in range(10):
        if i == 6:
            hoist.invalidate_hoist()
        plain.step()
        hoist.step()
        torch.cuda.synchronize()
        _same(rp0, plain, rp1, hoist, i)
        gn = plain.diagnostics()["grad_norm"]
        assert gn > c, (i, gn, c)                      # clipping is active
        assert hoist.diagnostics()["grad_norm"] == gn
    assert hoist.hoisted_steps == 8
    assert plain.error_word() == 0 and hoist.error_word() == 0


@pytest.mark.parametrize("optimizer", ["adam", "rmsprop_centered"])
def test_inactive_clip_has_no_side_effects(optimizer):
    """grad_clip 1e30 vs 0: the slab reduction moves from the optimizer launch to the norm
    launch, the optimizer launch becomes the non-slab pack kernel; the same bits over 4 steps."""
    rp0, a = _engine(True, interval=2, **_opt(optimizer, 1e30))
    rp1, b = _engine(True, interval=2, **_opt(optimizer, 0.0))
    assert a._fold_in_norm and a._fold_tq is not None
    assert not b._fold_in_norm and b._fold_tq is not None
    assert "grad_norm" in a.diagnostics() and "grad_norm" not in b.diagnostics()
    a.capture(warmup=0)
    b.capture(warmup=0)
    for i in range(4):
        a.step()
        b.step()
        torch.cuda.synchronize()
        _same(rp0, a, rp1, b, i)
    assert a.error_word() == 0 and b.error_word() == 0


def test_engine_adam_clip_step_matches_float64():
    """One eager step at B 8, Adam with an active clip: optim_ref predicts the master from the
    pre-step master and moments and the engine's own gradient; diagnostics' grad_norm is the
    float64 norm of that gradient within the norm kernel's bound."""
    c = _clip_from_data("adam", 8)
    rp, eng = _engine(True, B=8, graph=False, **_opt("adam", c))
    p0, m0, v0 = (t.double().cpu().numpy() for t in (eng.master, eng.opt_a, eng.opt_b))
    t = int(rp.step.item()) + 1
    eng.step()
    torch.cuda.synchronize()
    assert int(rp.step.item()) == t
    g = eng.grad.double().cpu().numpy()
    lc = eng.cfg.learner
    p, m, v = optim_ref.adam_step(p0, g, m0, v0, t, lc.lr, lc.adam_betas[0], lc.adam_betas[1],
                                  lc.eps, max_norm=c)
    norm = optim_ref.grad_norm(g)
    assert norm > c
    assert np.allclose(eng.master.double().cpu().numpy(), p, atol=1e-6, rtol=1e-5)
    assert np.abs(eng.master.double().cpu().numpy() - p0).max() > 1e-5      # the step moved it
    gn = eng.diagnostics()["grad_norm"]
    SL = int(kernels().r2_torso_bwd_slab_floats())
    assert eng._fold_in_norm
    bound = _gsq_bound(eng._fold_tq, -(-SL // 64))
    assert abs(gn - norm) / norm <= bound, (gn, norm, bound)
    assert eng.error_word() == 0


def test_resume_adam_clip_hoisted_run():
    """full_state_extra / load_full_state at step 3 of an Adam + clip hoisted run: steps 4..6 of
    the resumed engine equal the uninterrupted run's bitwise."""
    kw = _opt("adam", _clip_from_data("adam", 16))
    rp0, a = _engine(True, **kw)
    rp1, b = _engine(True, **kw)
    assert a.hoist and b.hoist
    a.capture(warmup=0)
    b.capture(warmup=0)
    for _ in range(3):
        a.step()
    torch.cuda.synchronize()
    obj = {"online": a.state_dict(), "target": a.target_state_dict(), "step": 3,
           "extra": a.full_state_extra()}
    for k, v in vars(rp0).items():          # the replay is not part of the checkpoint
        if torch.is_tensor(v):
            getattr(rp1, k).copy_(v)
    b.load_full_state(obj)
    assert b.steps_done == 3
    for i in range(3, 6):
        a.step()
        b.step()
        torch.cuda.synchronize()
        _same(rp0, a, rp1, b, i)
    assert a.hoisted_steps == 5 and b.hoisted_steps == 2
    assert a.error_word() == 0 and b.error_word() == 0
