"""Every entry point of the TD / dueling-head kernel family (csrc/kernels/td.hip, head.hip)
against the float64 oracle (pytorch_r2d2_amd/td_ref.py), element by element, at the smallest
shapes where each code path and each boundary is live.

Bounds (td_ref.check_td): without value rescaling |delta - delta_64| <= 4 * 2^-24 * (|q| + |r| +
gamma_n |boot|); with it, twice the error fp32 PyTorch makes on the same inputs with the
reference formulation (measured in the test on the CPU, never a constant), and no tighter than
the first bound.  Output buffers carry two extra rows; everything starts as NaN (priority: -1).

With R2D2_TD_ORACLE_REPORT=<file> the measured errors are written there
(profiles/td_oracle_errors.txt)."""
import numpy as np
import pytest
import torch

from gpu_support import DEV, NAN, dev, report_fixture, split_bf16
from gpu_support import stop_after_a_gpu_error  # noqa: F401
from pytorch_r2d2_amd import td_ref
from pytorch_r2d2_amd.ops._lib import kernels, ptr, stream_handle
from test_td_ref_cpu import (ALPHA, BURN_IN, GAMMA_N, N_VALID, PRIO_EPS, SHAPES, VR_EPS, f32,
                             make_case, make_terminal_case, make_tie_case, oracle, torch_delta)

pytestmark = pytest.mark.gpu

BETA = f32(0.6)
BF = torch.bfloat16
# (entry point, split precision)
ENTRIES = [("td_loss", False), ("td_duel", False), ("td_duel", True), ("td_duel_dh", False),
           ("td_duel_dh", True)]
DUEL = ENTRIES[1:]
_REPORT, _report = report_fixture(
    "R2D2_TD_ORACLE_REPORT",
    "# max |delta - delta_float64| per case: the kernel, fp32 PyTorch (reference\n"
    "# formulation, CPU), and fp32 with h^-1's sqrt(1+v)-1 taken as v/(sqrt(1+v)+1)\n"
    "# (the last two only with value rescaling, vr = 1; 0 otherwise)\n"
    "# case                         vr beta entry            kernel     torch_fp32 "
    "alt_hinv_fp32\n",
    fmt="%-30s %d  %.1f  %-16s %.3e  %.3e  %.3e")


def _poison(*shape, dtype=torch.float32, fill=NAN):
    return torch.full(shape, fill, dtype=dtype, device=DEV)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.uint8).numpy()


def _np(t, rows=None):
    t = t if rows is None else t[:rows]
    return t.detach().float().cpu().numpy().astype(np.float64)


def _stage(c):
    """Device copies of a case's inputs (once per case)."""
    if "dev" not in c:
        c["dev"] = {k: dev(np.asarray(c[k], dtype=np.float32) if k.startswith("q_") else c[k])
                    for k in ("q_sa", "q_arg", "q_tgt", "starts", "probs", "action", "reward", "done")}
        c["dev"]["n_valid"] = torch.tensor([N_VALID], dtype=torch.int32, device=DEV)
    return c["dev"]


def make_head(c, HD, H=256):
    """Head operands of the fused launches for case c: zr = relu(randn), about half of it exactly
    0 (bf16 values, and an fp32 draw for split precision), the second layer, and W1^T (H, 2 HD)
    as a bf16 matrix and as an fp32 one split into hi / lo planes."""
    key = ("head", HD)
    if key not in c:
        g = torch.Generator(device="cpu").manual_seed(7 * HD + c["A"])
        n, A = c["n"], c["A"]
        zr32 = torch.relu(torch.randn(n, 2 * HD, generator=g))
        w2 = torch.randn(1 + A, HD, generator=g)
        w1t = torch.randn(H, 2 * HD, generator=g) / float(np.sqrt(2 * HD))
        hi, lo = split_bf16(w1t)
        c[key] = dict(HD=HD, zr_bf=zr32.to(BF).to(DEV), zr_f32=zr32.to(DEV), w2=w2.to(DEV),
                      w1t=hi.to(DEV), w1t_lo=lo.to(DEV))
        frac = float((zr32 == 0).float().mean())
        assert 0.4 < frac < 0.6, frac
    return c[key]


def _launch(entry, c, vr, beta, *, sp=False, head=None, dp=None, probs=True, fuse_dh=None,
            fwd=None, A=None, H=256, Tl=None):
    """One launch of ``entry`` into fresh poisoned outputs.  Returns (rc, outputs) after a sync;
    outputs are device tensors with their 2 extra rows."""
    k = kernels()
    d = _stage(c)
    B, cap = c["B"], c["cap"]
    Tl = c["Tl"] if Tl is None else Tl
    A = c["A"] if A is None else A
    n = c["n"]
    o = dict(dq=_poison(n + 2, A), loss=_poison(3), td_abs=_poison(n + 2),
             priority=_poison(cap + 2, fill=-1.0), is_w=_poison(B + 2))
    part = torch.zeros(4096, device=DEV)
    o["ticket"] = torch.zeros(1, dtype=torch.int32, device=DEV)
    q = [d["q_sa"], d["q_arg"], d["q_tgt"]]
    if fwd is not None:       # the Q rows are outputs of the launch
        q = [_poison(n + 2, A) for _ in range(3)]
        o["q_on"], o["q_nx"], o["q_tg"] = q
    dpt = dev(np.asarray(dp, dtype=np.float32)) if dp is not None else None
    targs = (ptr(q[0]), ptr(q[1]), ptr(q[2]), ptr(d["starts"]), ptr(d["probs"]) if probs else 0,
             ptr(d["action"]), ptr(d["reward"]), ptr(d["done"]), ptr(o["dq"]), ptr(o["loss"]),
             ptr(o["td_abs"]), ptr(o["priority"]), ptr(o["is_w"]), ptr(d["n_valid"]), Tl, B, A,
             BURN_IN, c["cap_e"], GAMMA_N, int(vr), VR_EPS, ALPHA, PRIO_EPS, float(beta), ptr(part),
             ptr(o["ticket"]))
    if entry == "td_loss":
        rc = k.r2_td_loss(*targs, ptr(dpt), stream_handle())
    else:
        head = head or make_head(c, 64)
        HD = head["HD"]
        o["dz"], o["dva"] = _poison(n + 2, 2 * HD, dtype=BF), _poison(n + 2, 1 + A)
        if sp:
            o["dz_lo"] = _poison(n + 2, 2 * HD, dtype=BF)
        if fwd is not None:
            zr = o["zr"] = _poison(n + 2, 2 * HD, dtype=torch.float32 if sp else BF)
        else:
            zr = head["zr_f32" if sp else "zr_bf"]
        hargs = (ptr(zr), ptr(head["w2"]), ptr(o["dz"]), ptr(o["dva"]), HD, ptr(o.get("dz_lo")),
                 ptr(dpt))
        if entry == "td_duel":
            rc = k.r2_td_duel(*targs, *hargs, stream_handle())
        else:
            fuse_dh = fwd is None if fuse_dh is None else fuse_dh
            if fuse_dh:
                o["dh"] = _poison(n + 2, 256)
            farr = None
            if fwd is not None:
                farr = np.asarray([ptr(t) for t in fwd] + [ptr(t) for t in q] + [0], dtype=np.int64)
            rc = k.r2_td_duel_dh(*targs, *hargs, ptr(head["w1t"]) if fuse_dh else 0,
                                 ptr(head["w1t_lo"]) if fuse_dh and sp else 0, ptr(o.get("dh")), H,
                                 farr.ctypes.data if farr is not None else None, None,
                                 stream_handle())
    torch.cuda.synchronize()
    return rc, o


def _nothing_written(o):
    for key, t in o.items():
        if key == "ticket":
            assert int(t.item()) == 0
        elif key == "priority":
            assert bool((t == -1.0).all())
        else:
            assert bool(torch.isnan(t.float()).all()), key


def _tails_untouched(o, c):
    """The two extra rows of every output; priorities past the replay."""
    n, B, cap = c["n"], c["B"], c["cap"]
    for key, t in o.items():
        rows = {"ticket": None, "priority": None, "loss": 1, "is_w": B}.get(key, n)
        if rows is not None:
            assert bool(torch.isnan(t[rows:].float()).all()), key
            assert not bool(torch.isnan(t[:rows].float()).any()), key
    assert bool((o["priority"][cap:] == -1.0).all())


def _same_bits(o1, o2):
    for key in o1:
        assert np.array_equal(_bits(o1[key]), _bits(o2[key])), key


def fp32_floor(c, ref, vr):
    """With value rescaling: twice fp32 PyTorch's own worst error on this case (reference
    formulation, models.value_rescale / value_rescale_inv in float32 on the CPU)."""
    if not vr:
        return 0.0, 0.0
    d32, _ = torch_delta(c, vr, torch.float32)
    err = float(np.abs(d32.detach().double().numpy() - ref.delta).max())
    return 2.0 * err, err


def _alt_hinv_error(c, ref):
    """fp32 error of the same target with h^-1's sqrt(1 + v) - 1 taken as v / (sqrt(1 + v) + 1)
    (numpy float32 on the CPU; evidence for a later change, not a bound)."""
    one, eps = np.float32(1.0), np.float32(VR_EPS)
    x = ref.boot.astype(np.float32)
    v = np.float32(4.0) * eps * (np.abs(x) + one + eps)
    s = (v / (np.sqrt(one + v) + one)) / (np.float32(2.0) * eps)
    hinv = np.sign(x) * (s * s - one)
    y = ref.reward.astype(np.float32) + np.where(ref.done, np.float32(0.0), np.float32(GAMMA_N) * hinv)
    y = np.sign(y) * (np.sqrt(np.abs(y) + one) - one) + eps * y
    d = ref.q_taken.astype(np.float32) - y.astype(np.float32)
    return float(np.abs(d.astype(np.float64) - ref.delta).max())


def _check_core(o, c, ref, floor, extra=0.0):
    """dq, td_abs, loss, is_w against the oracle; priorities against the scatter of the
    launch's own td_abs (burn-in rows and rows outside every window stay -1); ticket 0."""
    n, B = c["n"], c["B"]
    out = dict(dq=_np(o["dq"], n), td_abs=_np(o["td_abs"], n), loss=float(o["loss"][0].item()),
               is_w=_np(o["is_w"], B))
    m = td_ref.check_td(out, ref, GAMMA_N, floor, extra)
    td_ref.check_priority(_np(o["priority"]), out["td_abs"].reshape(c["Tl"], B), ref, c["cap"],
                          ALPHA, PRIO_EPS)
    assert int(o["ticket"].item()) == 0
    _tails_untouched(o, c)
    return m


def _check_backward(o, c, ref, head, sp, floor, extra=0.0):
    n = c["n"]
    dz = _np(o["dz"], n) + (_np(o["dz_lo"], n) if sp else 0.0)
    zr = o["zr"][:n] if "zr" in o else head["zr_f32" if sp else "zr_bf"]
    td_ref.check_dueling_backward(dict(dva=_np(o["dva"], n), dz=dz), ref,
                                  td_ref.delta_bound(ref, GAMMA_N, floor, extra), _np(zr),
                                  _np(head["w2"]), head["HD"], sp)
    assert not dz[_np(zr) == 0].any(), "dz is nonzero where relu(z) is 0"


def _run_all_entries(c, vr, beta, name, entries=ENTRIES, dp=None, hd=64):
    ref = oracle(c, vr, beta, dp=dp)
    floor, err32 = fp32_floor(c, ref, vr)
    for entry, sp in entries:
        head = make_head(c, hd) if entry != "td_loss" else None
        rc, o = _launch(entry, c, vr, beta, sp=sp, head=head, dp=dp)
        assert rc == 0, (entry, rc)
        m = _check_core(o, c, ref, floor)
        if head is not None:
            _check_backward(o, c, ref, head, sp, floor)
        rc, o2 = _launch(entry, c, vr, beta, sp=sp, head=head, dp=dp)
        assert rc == 0
        _same_bits(o, o2)
        _REPORT.append((name, vr, beta, entry + ("_sp" if sp else ""), m["delta_err"], err32,
                        _alt_hinv_error(c, ref) if vr else 0.0))
    return ref


# ------------------------------------------------------------------ a. core TD outputs
@pytest.mark.parametrize("beta", [0.0, BETA], ids=["beta0", "beta0.6"])
@pytest.mark.parametrize("vr", [0, 1], ids=["plain", "rescale"])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_td_core_outputs_match_oracle(shape, vr, beta):
    """n not a multiple of 16 or 256, one action, both sides of the 8 LDS-staged second-layer
    rows, the 32 / 64 lane limits, B = 256; Q drawn at N(0, 0.05) and N(0, 10)."""
    Tl, B, A = shape
    for scale in (0.05, 10.0):
        c = make_case(Tl, B, A, q_scale=scale)
        entries = DUEL if A == 64 else ENTRIES
        ref = _run_all_entries(c, vr, beta, "core %dx%dx%d q%.2g" % (Tl, B, A, scale), entries)
        if c["n"] > 1:      # conditions on the inputs, not the kernel
            assert ref.done.any() and not ref.done.all() and (ref.act == A - 1).any()
            assert A == 1 or len(np.unique(ref.best)) > 1


# ------------------------------------------------------------------ b. argmax ties
@pytest.mark.parametrize("vr", [0, 1], ids=["plain", "rescale"])
@pytest.mark.parametrize("A", [6, 18])
def test_td_argmax_ties_pick_the_first_maximum(A, vr):
    """Two exact equal maxima, the maximum at A - 1, all entries equal, +0.0 against -0.0:
    every entry bootstraps from np.argmax's action (q_tgt differs by O(1) between actions)."""
    c = make_tie_case(A)
    first, last = oracle(c, vr, 0.0), oracle(c, vr, 0.0, mutation="last_max")
    assert (np.abs(first.delta - last.delta) > 0.1).sum() >= c["n"] // 2
    _run_all_entries(c, vr, 0.0, "ties A=%d" % A)


# ------------------------------------------------------------------ c. terminals
@pytest.mark.parametrize("vr", [0, 1], ids=["plain", "rescale"])
def test_td_terminal_rows_use_the_reward_only_target(vr):
    """q_tgt = 1e30 on every terminal row: all outputs finite, the target there is r (or h(r))."""
    c = make_terminal_case()
    ref = oracle(c, vr, BETA)
    r = ref.reward[ref.done]
    assert ref.done.sum() >= 4
    assert np.array_equal(ref.delta[ref.done], ref.q_taken[ref.done] - (td_ref.h(r, VR_EPS) if vr else r))
    _run_all_entries(c, vr, BETA, "terminals")


# ------------------------------------------------------------------ d. data-parallel IS weights
@pytest.mark.parametrize("beta", [0.0, BETA], ids=["beta0", "beta0.6"])
@pytest.mark.parametrize("shape", [(3, 33, 9), (1, 256, 4)], ids=["3x33x9", "1x256x4"])
def test_td_data_parallel_is_weights(shape, beta):
    from pytorch_r2d2_amd.parallel.sharded_replay import dp_is_weights
    c = make_case(*shape)
    dp = np.asarray([1.7, 0.4, 5000.0, 3.1], dtype=np.float32)
    _run_all_entries(c, 0, beta, "dp %dx%dx%d" % shape, dp=dp)
    want = dp_is_weights(torch.as_tensor(c["probs"]), torch.as_tensor(dp), beta)
    for entry, sp in ENTRIES:
        rc, o = _launch(entry, c, 0, beta, sp=sp, dp=dp)
        assert rc == 0
        torch.testing.assert_close(o["is_w"][:c["B"]].cpu(), want, rtol=2e-6, atol=1e-7)


# ------------------------------------------------------------------ e. fused dueling backward
@pytest.mark.parametrize("sp", [False, True], ids=["bf16", "split"])
@pytest.mark.parametrize("HD,A", [(64, 1), (128, 6), (256, 8), (512, 9), (512, 18), (64, 32)])
def test_td_fused_dueling_backward(HD, A, sp):
    """dva per element, dz to one bf16 rounding (bf16) or 16 mantissa bits (hi + lo), the ReLU
    mask exact where zr is 0; for bf16 and A <= 32 bitwise r2_dueling_bwd of the kernel's dq."""
    k = kernels()
    c = make_case(3, 7, A, seed=2)
    n = c["n"]
    head = make_head(c, HD)
    for vr, beta in ((0, 0.0), (1, BETA)):
        ref = oracle(c, vr, beta)
        floor, _ = fp32_floor(c, ref, vr)
        rc, o = _launch("td_duel", c, vr, beta, sp=sp, head=head)
        assert rc == 0
        _check_core(o, c, ref, floor)
        _check_backward(o, c, ref, head, sp, floor)
        if not sp:
            dz, dva = _poison(n + 2, 2 * HD, dtype=BF), _poison(n + 2, 1 + A)
            assert k.r2_dueling_bwd(ptr(o["dq"]), ptr(head["zr_bf"]), ptr(head["w2"]), ptr(dz),
                                    ptr(dva), n, A, HD, stream_handle()) == 0
            torch.cuda.synchronize()
            assert np.array_equal(_bits(dz), _bits(o["dz"]))
            assert np.array_equal(_bits(dva), _bits(o["dva"]))
            # the separate kernel against the oracle, a dense dq (every action's column live)
            g = torch.Generator(device="cpu").manual_seed(HD + A)
            dq = torch.randn(n, A, generator=g)
            assert k.r2_dueling_bwd(ptr(dq.to(DEV)), ptr(head["zr_bf"]), ptr(head["w2"]), ptr(dz),
                                    ptr(dva), n, A, HD, stream_handle()) == 0
            torch.cuda.synchronize()
            dva_r, dz_r = td_ref.dueling_backward_reference(dq.numpy(), _np(head["zr_bf"]),
                                                            _np(head["w2"]), A, HD)
            mag = np.abs(dq.numpy().astype(np.float64)).sum(1, keepdims=True)
            assert (np.abs(_np(dva, n) - dva_r) <= (A + 3) * td_ref.U24 * 2 * mag).all()
            w2a = np.abs(_np(head["w2"]))
            mz = np.concatenate([mag * w2a[0][None, :], (np.abs(dva_r[:, 1:]) + mag / A) @ w2a[1:]], 1)
            assert (np.abs(_np(dz, n) - dz_r) <= 2.0 ** -8 * np.abs(dz_r) + 2 * (A + 3) * td_ref.U24 * mz).all()
            assert bool(torch.isnan(dz[n:].float()).all()) and bool(torch.isnan(dva[n:]).all())


# ------------------------------------------------------------------ f. dueling forward, multi-job
def _fwd_operands(N, A, HD, seed, sp):
    g = torch.Generator(device="cpu").manual_seed(seed)
    z = torch.randn(max(N, 1), 2 * HD, generator=g)[:N]
    z = z if sp else z.to(BF)
    return dict(N=N, z=z.to(DEV), b1=(0.3 * torch.randn(2 * HD, generator=g)).to(DEV),
                w2=(torch.randn(1 + A, HD, generator=g) * float(1.5 / np.sqrt(HD))).to(DEV),
                b2=(0.3 * torch.randn(1 + A, generator=g)).to(DEV),
                q=_poison(N + 2, A), zr=_poison(N + 2, 2 * HD, dtype=torch.float32 if sp else BF))


def _fwd_multi(jobs, A, HD, sp):
    k = kernels()
    arr = np.asarray([[ptr(j["z"]), ptr(j["b1"]), ptr(j["w2"]), ptr(j["b2"]), ptr(j["q"]),
                       ptr(j["zr"]), j["N"]] for j in jobs], dtype=np.int64)
    fn = k.r2_dueling_fwd_multi_f32 if sp else k.r2_dueling_fwd_multi
    rc = fn(arr.ctypes.data, len(jobs), A, HD, stream_handle())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("sp", [False, True], ids=["bf16", "f32"])
@pytest.mark.parametrize("A", [1, 9, 32])
@pytest.mark.parametrize("HD", [64, 256, 512])
def test_dueling_forward_multi_job(HD, A, sp):
    """Three jobs with N = (5, 0, 7) -- a workgroup's four waves straddle two jobs, an empty job in
    the middle -- and one job of 3 rows; distinct parameters per job."""
    for Ns in ((5, 0, 7), (3,)):
        jobs = [_fwd_operands(N, A, HD, 100 * HD + 10 * A + i, sp) for i, N in enumerate(Ns)]
        assert _fwd_multi(jobs, A, HD, sp) == 0
        for j in jobs:
            N = j["N"]
            assert bool(torch.isnan(j["q"][N:]).all()) and bool(torch.isnan(j["zr"][N:].float()).all())
            if N:
                td_ref.check_dueling_forward(_np(j["q"], N), _np(j["zr"], N), _np(j["z"]), _np(j["b1"]),
                                             _np(j["w2"]), _np(j["b2"]), A, HD, zr_bf16=not sp)


@pytest.mark.parametrize("sp", [False, True], ids=["bf16", "f32"])
def test_dueling_forward_refuses_unsupported_shapes(sp):
    for A, HD, code in ((33, 64, -1), (6, 96, -2)):
        jobs = [_fwd_operands(N, A, HD, 5 + i, sp) for i, N in enumerate((5, 0, 7))]
        assert _fwd_multi(jobs, A, HD, sp) == code
        for j in jobs:
            assert bool(torch.isnan(j["q"]).all()) and bool(torch.isnan(j["zr"].float()).all())


# ------------------------------------------------------------------ g. fused head forward
# seeds picked on the CPU so that, in float64, the best and second-best q_arg are at least 1e-3
# apart on EVERY row (bf16 and fp32 z alike): the kernel's fp32 argmax is then free to agree
FWD_SEEDS = {(64, 6): 0, (256, 9): 0, (64, 18): 0, (256, 32): 0, (512, 6): 0, (128, 9): 0,
             (512, 32): 0}


def make_fwd_case(HD, A, seed, sp):
    """Case + head-forward operands: z of the online / online-on-next / target heads, distinct
    online and target parameters.  The case's Q arrays are the ORACLE's float64 Q rows."""
    c = make_case(3, 7, A, seed=seed)
    n = c["n"]
    g = torch.Generator(device="cpu").manual_seed(31 * seed + HD + A)
    zs = [torch.randn(n, 2 * HD, generator=g) for _ in range(3)]
    par = {}
    for net in ("on", "tg"):
        par[net] = dict(b1=0.3 * torch.randn(2 * HD, generator=g),
                        w2=torch.randn(1 + A, HD, generator=g) * float(1.5 / np.sqrt(HD)),
                        b2=0.3 * torch.randn(1 + A, generator=g))
    zs = [z if sp else z.to(BF) for z in zs]
    c["fz"], c["fpar"] = zs, par
    qs, qb = [], []
    for z, net in zip(zs, ("on", "on", "tg")):
        p = par[net]
        args = (_np(z), _np(p["b1"]), _np(p["w2"]), _np(p["b2"]), A, HD)
        qs.append(td_ref.dueling_forward_reference(*args))
        qb.append(td_ref.q_bound(*args))
    c["q_sa"], c["q_arg"], c["q_tgt"] = qs[0][0], qs[1][0], qs[2][0]
    c["hr_on"], c["q_bounds"] = qs[0][1], qb
    top = np.sort(c["q_arg"], axis=1)
    c["gap"] = float((top[:, -1] - top[:, -2]).min()) if A > 1 else np.inf
    return c


def _q_extra(c, ref, vr):
    """What the Q rows' own fp32 error (td_ref.q_bound) adds to |delta|: the taken action's
    bound, plus the bootstrap's through d y / d boot -- gamma_n, or with value rescaling
    gamma_n h'(r + gamma_n h^-1(boot)) / h'(h^-1(boot))."""
    Tl, B = c["Tl"], c["B"]
    pick = lambda a, i: np.take_along_axis(a.reshape(Tl, B, -1), i[..., None], -1)[..., 0]  # noqa: E731
    e_sa, e_bt = pick(c["q_bounds"][0], ref.act), pick(c["q_bounds"][2], ref.best)
    fac = np.full((Tl, B), GAMMA_N)
    if vr:
        hp = lambda x: 0.5 / np.sqrt(np.abs(x) + 1.0) + VR_EPS   # noqa: E731
        X = td_ref.h_inv(ref.boot, VR_EPS)
        fac = GAMMA_N * hp(ref.reward + GAMMA_N * X) / hp(X)
    return e_sa + np.where(ref.done, 0.0, fac * e_bt)


@pytest.mark.parametrize("sp", [False, True], ids=["bf16", "split"])
@pytest.mark.parametrize("HD,A", list(FWD_SEEDS), ids=["%dx%d" % k for k in FWD_SEEDS])
def test_td_fused_head_forward(HD, A, sp):
    """The ``fwd`` operand: the three Q outputs and the written zr bitwise equal to
    r2_dueling_fwd_multi / _f32 on the same operands and within the Q bound of the oracle; the TD
    outputs against the oracle run on the oracle's own Q."""
    c = make_fwd_case(HD, A, FWD_SEEDS[(HD, A)], sp)
    assert c["gap"] >= 1e-3, c["gap"]
    n = c["n"]
    head = make_head(c, HD)
    on, tg = ({k: v.to(DEV) for k, v in c["fpar"][net].items()} for net in ("on", "tg"))
    head = dict(head, w2=on["w2"])
    z = [t.to(DEV) for t in c["fz"]]
    fwd = [z[0], z[1], z[2], on["b1"], tg["b1"], tg["w2"], on["b2"], tg["b2"]]
    jobs = [dict(N=n, z=zz, q=_poison(n + 2, A), zr=None, **p) for zz, p in zip(z, (on, on, tg))]
    jobs[0]["zr"] = _poison(n + 2, 2 * HD, dtype=torch.float32 if sp else BF)
    assert _fwd_multi(jobs, A, HD, sp) == 0
    for vr in (0, 1):
        ref = oracle(c, vr, BETA)
        floor, _ = fp32_floor(c, ref, vr)
        extra = _q_extra(c, ref, vr)
        rc, o = _launch("td_duel_dh", c, vr, BETA, sp=sp, head=head, fwd=fwd)
        assert rc == 0
        for key, j, (zq, p) in zip(("q_on", "q_nx", "q_tg"), jobs, zip(z, (on, on, tg))):
            assert np.array_equal(_bits(o[key]), _bits(j["q"])), key
            td_ref.check_dueling_forward(_np(o[key], n), _np(o["zr"], n) if key == "q_on" else None,
                                         _np(zq), _np(p["b1"]), _np(p["w2"]), _np(p["b2"]), A, HD,
                                         zr_bf16=not sp)
        assert np.array_equal(_bits(o["zr"]), _bits(jobs[0]["zr"]))
        _check_core(o, c, ref, floor, extra)
        _check_backward(o, c, ref, head, sp, floor, extra)


@pytest.mark.parametrize("sp", [False, True], ids=["bf16", "split"])
def test_td_fused_head_forward_refuses_33_actions(sp):
    c = make_fwd_case(64, 6, 0, sp)
    head = make_head(c, 64)
    bufs = [torch.zeros(c["n"], 128, device=DEV) for _ in range(3)] + \
           [torch.zeros(34 * 64, device=DEV) for _ in range(5)]
    rc, o = _launch("td_duel_dh", c, 0, BETA, sp=sp, head=head, fwd=bufs, A=33)
    assert rc == -6
    _nothing_written(o)


# ------------------------------------------------------------------ h. fused dh
@pytest.mark.parametrize("sp", [False, True], ids=["bf16", "split"])
@pytest.mark.parametrize("HD", [64, 256])
def test_td_fused_dh_is_the_product_of_its_own_dz(HD, sp):
    """n = 35: the last workgroup has 3 valid rows and 13 idle waves.  dh against the float64
    product of the launch's own dz (hi + lo in split precision) with W1; relative norm below the
    project's bounds for the same products (2e-2 bf16, 2e-5 split)."""
    c = make_case(5, 7, 6, seed=4)
    n = c["n"]
    assert n == 35
    head = make_head(c, HD)
    rc, o = _launch("td_duel_dh", c, 0, 0.0, sp=sp, head=head)
    assert rc == 0
    ref = oracle(c, 0, 0.0)
    _check_core(o, c, ref, 0.0)
    _check_backward(o, c, ref, head, sp, 0.0)
    dz = _np(o["dz"], n) + (_np(o["dz_lo"], n) if sp else 0.0)
    w1t = _np(head["w1t"]) + (_np(head["w1t_lo"]) if sp else 0.0)
    want = dz @ w1t.T
    got = _np(o["dh"], n)
    assert np.abs(want).max() > 0
    rel = np.linalg.norm(got - want) / np.linalg.norm(want)
    assert rel < (2e-5 if sp else 2e-2), rel
    # every row on its own, too: a norm over 35 rows hides one wrong row of a small |delta|
    rows = np.linalg.norm(got - want, axis=1) / np.maximum(np.linalg.norm(want, axis=1), 1e-300)
    assert (rows < (2e-5 if sp else 2e-2)).all(), rows.max()
    rc, o = _launch("td_duel_dh", c, 0, 0.0, sp=sp, head=head, H=128)
    assert rc == -5
    _nothing_written(o)


# ------------------------------------------------------------------ i. loss over a large grid
def test_td_loss_reduction_over_a_large_grid():
    """(Tl, B) = (80, 256): 1,280 td_duel workgroups (the last arriver's strided partial sum takes
    a second trip), 80 td_kernel workgroups.  The sub-rings hold 128 rows here: a window of
    burn_in + 80 rows has to fit its ring, as every window the replay samples does."""
    c = make_case(80, 256, 4, cap_e=128)
    _run_all_entries(c, 0, BETA, "grid 80x256x4", entries=ENTRIES[:3])
    _run_all_entries(c, 1, 0.0, "grid 80x256x4", entries=ENTRIES[:3])


@pytest.mark.parametrize("sp", [False, True], ids=["bf16", "split"])
def test_td_duel_refuses_more_workgroups_than_partials(sp):
    c = make_case(1, 256, 4)
    rc, o = _launch("td_duel", c, 0, BETA, sp=sp, Tl=257)
    assert rc == -2
    _nothing_written(o)
