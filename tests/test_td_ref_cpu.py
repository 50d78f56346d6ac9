"""The float64 oracle of the TD / dueling-head kernels (pytorch_r2d2_amd/td_ref.py) against
independent float64 PyTorch, and the comparison functions against mutated oracles.

Also holds the case builder the GPU tests (test_td_head_gpu.py) share: seeded CPU generators, a
two-sub-ring replay with duplicate / overlapping / wrapping starts, terminals, every action."""
import numpy as np
import pytest
import torch

from pytorch_r2d2_amd import td_ref
from pytorch_r2d2_amd.models.qnet import value_rescale, value_rescale_inv

f32 = lambda x: float(np.float32(x))   # noqa: E731  (a launch passes its scalars as C floats)
BURN_IN, N_VALID = 2, 777
GAMMA_N, VR_EPS, ALPHA, PRIO_EPS = f32(0.997 ** 5), f32(1e-3), f32(0.9), f32(1e-6)
# duplicates (3, 5), overlaps (3 / 5 / 7), ring wraps (60, 62), the second sub-ring (64 + 10)
START_PATTERN = (3, 5, 3, 64 + 10, 60, 7, 5, 62)
SHAPES = [(6, 8, 6), (5, 7, 1), (3, 33, 9), (4, 16, 18), (2, 5, 32), (1, 256, 4), (1, 1, 2),
          (2, 3, 64)]


def make_starts(B, cap_e=64):
    """START_PATTERN repeated to B starts: block k of 8 is shifted by 5 k rows inside its
    sub-ring, odd blocks swap the sub-rings."""
    out = []
    for b in range(B):
        p, k = START_PATTERN[b % 8], b // 8
        sub, off = p // 64, p % 64
        out.append(((sub + k) % 2) * cap_e + (off + 5 * k) % cap_e)
    return np.asarray(out, dtype=np.int32)


def make_case(Tl, B, A, seed=0, q_scale=1.0, cap_e=64):
    """Inputs of one TD launch as float32 / integer numpy arrays (exact in both the kernel and
    the oracle).  done = 1 with probability 1/4, actions uniform, probs log-uniform in
    [1e-6, 1e-1] with the last entry exactly 0."""
    g = torch.Generator(device="cpu").manual_seed(1000 * seed + 17 * Tl + 3 * B + A)
    n, cap = Tl * B, 2 * cap_e
    starts = make_starts(B, cap_e)
    rows = td_ref.ring_rows(starts, Tl, BURN_IN, cap_e)
    q = [(torch.randn(n, A, generator=g) * q_scale).numpy() for _ in range(3)]
    action = torch.randint(0, A, (cap,), generator=g).to(torch.uint8).numpy()
    reward = torch.randn(cap, generator=g).numpy()
    done = (torch.rand(cap, generator=g) < 0.25).to(torch.uint8).numpy()
    probs = (10.0 ** (-6.0 + 5.0 * torch.rand(B, generator=g))).numpy().astype(np.float32)
    probs[B - 1] = 0.0
    if n > 1:
        # the input conditions every case must meet, whatever the draw: a terminal and a
        # non-terminal learning row, action A - 1 taken
        done[rows[0, 0]], action[rows[0, 0]] = 1, A - 1
        other = rows.reshape(-1)[rows.reshape(-1) != rows[0, 0]]
        done[other[-1]] = 0
    return dict(Tl=Tl, B=B, A=A, n=n, cap=cap, cap_e=cap_e, starts=starts, rows=rows, q_sa=q[0],
                q_arg=q[1], q_tgt=q[2], action=action, reward=reward, done=done, probs=probs)


def make_tie_case(A):
    """q_arg rows with two exact equal maxima, the maximum at A - 1, all entries equal, and
    +0.0 against -0.0 in both orders; q_tgt has a distinct O(1) value per action; no terminals."""
    c = make_case(4, 8, A, seed=3)
    n = c["n"]
    c["done"][:] = 0          # every row bootstraps: no tie hides behind a terminal
    qa = -1.0 - np.abs(c["q_arg"])
    for i in range(n):
        j, k = i % A, (3 * i + 1 + (i % A)) % A
        if k == j:
            k = (j + 1) % A
        lo, hi = min(j, k), max(j, k)
        kind = i % 5
        if kind == 0:
            qa[i, j] = qa[i, k] = 0.75
        elif kind == 1:
            qa[i, A - 1] = 0.5
        elif kind == 2:
            qa[i, :] = -0.25
        elif kind == 3:
            qa[i, lo], qa[i, hi] = -0.0, 0.0
        else:
            qa[i, lo], qa[i, hi] = 0.0, -0.0
    c["q_arg"] = qa.astype(np.float32)
    c["q_tgt"] = np.tile((0.5 * (1 + np.arange(A)) * (-1.0) ** np.arange(A)).astype(np.float32),
                         (n, 1))
    return c


def make_terminal_case(Tl=6, B=8, A=6):
    """1e30 in q_tgt on every terminal row: it must never reach the target."""
    c = make_case(Tl, B, A, seed=5)
    dn = c["done"][c["rows"]].reshape(-1) != 0
    c["q_tgt"] = c["q_tgt"].copy()
    c["q_tgt"][dn, :] = 1e30
    return c


def oracle(c, vr, beta, dp=None, mutation=None, probs=True):
    return td_ref.td_reference(c["q_sa"], c["q_arg"], c["q_tgt"], c["starts"],
                               c["probs"] if probs else None, c["action"], c["reward"], c["done"],
                               c["Tl"], c["B"], c["A"], BURN_IN, c["cap_e"], GAMMA_N, vr, VR_EPS,
                               ALPHA, PRIO_EPS, beta, N_VALID, dp, mutation=mutation)


def torch_delta(c, vr, dtype):
    """The reference formulation (learner_ref.r2d2_loss: gather, argmax, value_rescale_inv,
    value_rescale) in ``dtype`` on the CPU.  Returns (delta (Tl, B), q_sa leaf, its view)."""
    Tl, B, A = c["Tl"], c["B"], c["A"]
    t = lambda x: torch.as_tensor(np.asarray(x)).to(dtype)   # noqa: E731
    rows = torch.as_tensor(c["rows"])
    q_sa_all = t(c["q_sa"]).reshape(Tl, B, A).requires_grad_(True)
    q_arg, q_tgt = t(c["q_arg"]).reshape(Tl, B, A), t(c["q_tgt"]).reshape(Tl, B, A)
    action = torch.as_tensor(c["action"].astype(np.int64))[rows]
    reward, done = t(c["reward"])[rows], t(c["done"])[rows]
    q_sa = q_sa_all.gather(2, action.unsqueeze(-1)).squeeze(-1)
    a_star = q_arg.argmax(-1, keepdim=True)
    boot = q_tgt.gather(2, a_star).squeeze(-1)
    if vr:
        boot = value_rescale_inv(boot, VR_EPS)
    y = reward + GAMMA_N * boot * (1.0 - done)
    if vr:
        y = value_rescale(y, VR_EPS)
    return q_sa - y.detach(), q_sa_all


def _close(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    scale = max(float(np.abs(b).max()), 1e-300)
    assert np.abs(a - b).max() <= 1e-12 * scale, what


CASES = [("plain", lambda: make_case(6, 8, 6)), ("one_action", lambda: make_case(5, 7, 1)),
         ("wide", lambda: make_case(3, 33, 9, q_scale=10.0)), ("b256", lambda: make_case(1, 256, 4)),
         ("ties6", lambda: make_tie_case(6)), ("ties18", lambda: make_tie_case(18)),
         ("terminals", make_terminal_case)]


@pytest.mark.parametrize("vr", [0, 1])
@pytest.mark.parametrize("beta", [0.0, f32(0.6)])
@pytest.mark.parametrize("name,build", CASES, ids=[c[0] for c in CASES])
def test_td_reference_matches_float64_torch(name, build, beta, vr):
    c = build()
    ref = oracle(c, vr, beta)
    delta, q_leaf = torch_delta(c, vr, torch.float64)
    w = torch.ones(c["B"], dtype=torch.float64)
    if beta > 0:     # learner_ref.batch_from_hbm
        w = (max(N_VALID, 1) * torch.as_tensor(c["probs"]).double()).clamp_min(1e-30) ** (-beta)
        w = w / w.max()
    loss = (w[None, :] * 0.5 * delta ** 2).mean()
    loss.backward()
    assert np.isfinite(ref.delta).all() and np.isfinite(ref.loss)
    _close(ref.delta, delta.detach().numpy(), "delta")
    _close(ref.loss, loss.item(), "loss")
    _close(ref.dq, q_leaf.grad.numpy(), "dq")
    _close(ref.is_w, w.numpy(), "is_w")
    # ring rows: the reference's own index arithmetic (learner_ref.batch_from_hbm)
    s = torch.as_tensor(c["starts"]).long()
    base = s - s % c["cap_e"]
    t = BURN_IN + torch.arange(c["Tl"])
    rows = base[None, :] + (s[None, :] - base[None, :] + t[:, None]) % c["cap_e"]
    assert np.array_equal(ref.rows, rows.numpy())
    assert (ref.rows // c["cap_e"] == (c["starts"] // c["cap_e"])[None, :]).all()


def test_case_builder_meets_the_input_conditions():
    for Tl, B, A in SHAPES + [(80, 256, 4)]:
        c = make_case(Tl, B, A, cap_e=128 if Tl > 62 else 64)
        ref = oracle(c, 0, 0.0)
        assert c["probs"][-1] == 0 and (c["probs"][:-1] >= 1e-6).all() and (c["probs"] <= 0.1).all()
        if c["n"] > 1:
            assert ref.done.any() and not ref.done.all()
            assert (ref.act == A - 1).any()
        if c["n"] > 1 and A > 1:
            assert len(np.unique(ref.best)) > 1
        if B >= 8:
            s, e = c["starts"], c["cap_e"]
            assert len(np.unique(s)) < B and (s >= e).any() and (s % e + BURN_IN + Tl > e).any()
            counts = np.bincount(ref.rows.reshape(-1), minlength=c["cap"])
            assert counts.max() > 1 and ((counts == 0).any() or Tl > 62)
    for A in (6, 18):
        c = make_tie_case(A)
        first, last = oracle(c, 0, 0.0), oracle(c, 0, 0.0, mutation="last_max")
        assert (first.best != last.best).sum() >= c["n"] // 2
        assert (np.abs(first.delta - last.delta) > 0.1).sum() >= c["n"] // 2
        assert (first.best == A - 1).any() and (first.best == 0).any()


def test_is_weights_dp_form_matches_sharded_replay():
    from pytorch_r2d2_amd.parallel.sharded_replay import dp_is_weights
    c = make_case(3, 33, 9)
    dp = np.asarray([1.7, 0.4, 5000.0, 3.1], dtype=np.float32)
    for beta in (0.0, f32(0.6)):
        ref = oracle(c, 0, beta, dp=dp)
        want = dp_is_weights(torch.as_tensor(c["probs"]).double(), torch.as_tensor(dp).double(), beta)
        _close(ref.is_w, want.numpy(), "dp is_w")
        assert ref.is_w.max() != pytest.approx(1.0)      # not divided by the batch maximum


def test_priority_reference_is_numpy_duplicate_assignment():
    c = make_case(6, 8, 6)
    ref = oracle(c, 0, 0.0)
    td_abs = np.abs(ref.delta)
    got = td_ref.priority_reference(td_abs, ref.rows, c["cap"] + 2, ALPHA, PRIO_EPS, -1.0)
    want = np.full(c["cap"] + 2, -1.0)
    want[ref.rows.reshape(-1)] = ((td_abs + PRIO_EPS) ** ALPHA).reshape(-1)
    assert np.array_equal(got, want)
    burn = td_ref.ring_rows(c["starts"], BURN_IN, 0, c["cap_e"])
    only_burn = np.setdiff1d(burn.reshape(-1), ref.rows.reshape(-1))
    assert len(only_burn) and (got[only_burn] == -1.0).all()


@pytest.mark.parametrize("A,HD", [(1, 64), (6, 64), (9, 128), (32, 256)])
def test_dueling_references_match_autograd(A, HD):
    g = torch.Generator(device="cpu").manual_seed(A + HD)
    N = 11
    z = torch.randn(N, 2 * HD, generator=g, dtype=torch.float64)
    b1 = torch.randn(2 * HD, generator=g, dtype=torch.float64)
    w2 = torch.randn(1 + A, HD, generator=g, dtype=torch.float64)
    b2 = torch.randn(1 + A, generator=g, dtype=torch.float64)
    dq = torch.randn(N, A, generator=g, dtype=torch.float64)
    hr = torch.relu(z + b1).detach().requires_grad_(True)
    val = hr[:, :HD] @ w2[0] + b2[0]
    adv = hr[:, HD:] @ w2[1:].t() + b2[1:]
    q = val[:, None] + adv - adv.mean(dim=1, keepdim=True)
    q_ref, hr_ref = td_ref.dueling_forward_reference(z.numpy(), b1.numpy(), w2.numpy(), b2.numpy(),
                                                     A, HD)
    _close(q_ref, q.detach().numpy(), "q")
    assert np.array_equal(hr_ref, hr.detach().numpy())
    q.backward(dq)
    dva, dz = td_ref.dueling_backward_reference(dq.numpy(), hr_ref, w2.numpy(), A, HD)
    _close(dz, (hr.grad * (hr > 0)).numpy(), "dz")
    # dva = dL/d[val, adv]: through leaves standing for the second layer's outputs
    v = torch.zeros(N, dtype=torch.float64, requires_grad=True)
    a = torch.zeros(N, A, dtype=torch.float64, requires_grad=True)
    (v[:, None] + a - a.mean(dim=1, keepdim=True)).backward(dq)
    _close(dva, torch.cat([v.grad[:, None], a.grad], 1).numpy(), "dva")


# ------------------------------------------------------------------------------- mutations
# The comparison functions the GPU tests use must reject an oracle that is wrong in the one rule
# a sub-case is about.  The "kernel" here is the true oracle rounded to fp32.

def _as_kernel(ref):
    return dict(dq=ref.dq.astype(np.float32), td_abs=np.abs(ref.delta).astype(np.float32),
                loss=np.float32(ref.loss), is_w=ref.is_w.astype(np.float32))


@pytest.mark.parametrize("mutation,build,beta", [
    ("terminal_ignored", make_terminal_case, 0.0),
    ("terminal_ignored", lambda: make_case(6, 8, 6), 0.0),
    ("last_max", lambda: make_tie_case(6), 0.0),
    ("last_max", lambda: make_tie_case(18), 0.0),
    ("is_max_first_wave", lambda: make_case(1, 256, 4), f32(0.6)),
], ids=["terminals-1e30", "terminals-core", "ties6", "ties18", "is_max-b256"])
@pytest.mark.parametrize("vr", [0, 1])
def test_check_td_rejects_a_mutated_oracle(mutation, build, beta, vr):
    c = build()
    true = oracle(c, vr, beta)
    out = _as_kernel(true)
    floor = 2e-4 if vr else 0.0       # the order of twice fp32 PyTorch's error (GPU test: measured)
    td_ref.check_td(out, true, GAMMA_N, floor)
    with pytest.raises(AssertionError):
        td_ref.check_td(out, oracle(c, vr, beta, mutation=mutation), GAMMA_N, floor)


def test_check_priority_rejects_first_duplicate_winning():
    c = make_case(6, 8, 6)
    ref = oracle(c, 0, 0.0)
    td_abs = np.abs(ref.delta).astype(np.float32)
    prio = td_ref.priority_reference(td_abs, ref.rows, c["cap"] + 2, ALPHA, PRIO_EPS, -1.0)
    prio = prio.astype(np.float32)
    td_ref.check_priority(prio, td_abs, ref, c["cap"], ALPHA, PRIO_EPS)
    with pytest.raises(AssertionError):
        td_ref.check_priority(prio, td_abs, ref, c["cap"], ALPHA, PRIO_EPS, mutation="first_dup")


@pytest.mark.parametrize("sp", [False, True], ids=["bf16", "split"])
def test_check_dueling_backward_rejects_ge_mask(sp):
    c = make_case(3, 7, 6)
    ref = oracle(c, 0, 0.0)
    A, HD, n = 6, 64, c["n"]
    g = torch.Generator(device="cpu").manual_seed(2)
    zr = torch.relu(torch.randn(n, 2 * HD, generator=g)).to(torch.bfloat16).float().numpy()
    w2 = torch.randn(1 + A, HD, generator=g).numpy()
    assert 0.4 < (zr == 0).mean() < 0.6
    dva, dz = td_ref.dueling_backward_reference(ref.dq, zr, w2, A, HD)
    hi = torch.as_tensor(dz).float().to(torch.bfloat16).float().numpy()
    lo = torch.as_tensor(dz - hi).float().to(torch.bfloat16).float().numpy()
    out = dict(dva=dva.astype(np.float32), dz=(hi + lo) if sp else hi)
    bound = td_ref.delta_bound(ref, GAMMA_N)
    td_ref.check_dueling_backward(out, ref, bound, zr, w2, HD, sp)
    with pytest.raises(AssertionError):
        td_ref.check_dueling_backward(out, ref, bound, zr, w2, HD, sp, mutation="relu_ge")
