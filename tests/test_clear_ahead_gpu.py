"""Serial clear-ahead: the hoisted learner step kept under serial actor writes.

``actor.clear_ahead = A`` makes the batched actor clear the sequence start A rows AHEAD of its write
head (actor.hip, ahead > 0), so rows head .. head+A-1 of every sub-ring never hold a start and a
batch sampled before the next M <= A actor steps holds no window those steps overwrite.
``LearnerEngine.cover_writes(actor)`` then keeps the pre-sampled batch across such steps
(``_hoist_fresh``) and puts a device guard (replay.hip hoist_guard_kernel) in front of every step,
which recounts the claim from the actor's device words and reports torn pre-sampled windows in bit
29 of the error word.

Shapes as tests/test_hoist_live_gpu.py: burn-in 4, learn 6, overlap 5, n = 3, B = 8, 16 envs of
VecSyntheticAtari(episode_len=37), sub-rings of 128 rows, 80 warm actor steps."""
import numpy as np
import pytest
import torch

from pytorch_r2d2_amd.engine.replay_check import (bootstrap_violations, check_windows,
                                                  guard_reference, ring_offsets)
from test_hoist_live_gpu import (CAP_E, DEV, E, WARM, _assert_states_fresh, _assert_windows_whole,
                                 _cfg, _state)
from test_native_gpu import _record, _small_cfg, _tree_consistent

pytestmark = pytest.mark.gpu
GUARD_BIT = 1 << 29


def _build(hoist, graph, A, cover=True, **over):
    """test_hoist_live_gpu._live with ``actor.clear_ahead = A``, and ``cover_writes`` in front of
    the capture (``graph``: capture the learner step; the plain engine runs eager)."""
    from pytorch_r2d2_amd.actor_batched import BatchedActor, engine_weights
    from pytorch_r2d2_amd.engine.learner_engine import LearnerEngine
    from pytorch_r2d2_amd.engine.replay_hbm import HBMReplay
    from pytorch_r2d2_amd.envs.synthetic import VecSyntheticAtari
    cfg = _cfg(hoist, graph, **{"actor.clear_ahead": A}, **over)
    rp = HBMReplay(cfg, DEV, capacity=E * CAP_E, n_subrings=E)
    eng = LearnerEngine(cfg, rp, DEV)
    env = VecSyntheticAtari(E, DEV, seed=3, episode_len=37, n_actions=cfg.model.n_actions)
    on, tg = engine_weights(eng)
    actor = BatchedActor(cfg, rp, env, on, tg, seed=1)
    assert actor.clear_ahead == A
    for _ in range(WARM):
        actor.step()
    assert int(rp.n_valid.item()) >= 4 * cfg.learner.batch_size
    if hoist and cover:
        assert eng.hoist
        eng.cover_writes(actor)
    if graph:
        eng.capture(warmup=0)
    return cfg, rp, eng, actor


def _oracle_count(starts, head_before, M, rp, cfg):
    """Torn windows + bootstrap violations of one batch against the M rows written from
    ``head_before`` (engine/replay_check.py, brute force)."""
    T, n = cfg.replay.seq_len, cfg.replay.n_step
    torn, boot = check_windows(np.asarray(starts)[None], rp.cap_e, T, n,
                               [ring_offsets(head_before, M, rp.cap_e)])
    bad = bootstrap_violations(boot, rp.done.cpu().numpy(), rp.cap_e, T)
    return len(torn), len(bad)


# ------------------------------------------------------------------ 1. the actor kernel
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("A", [1, 4])
def test_actor_keeps_the_rows_ahead_of_its_head_free_of_starts(A, graph):
    from pytorch_r2d2_amd.actor_batched import BatchedActor, engine_weights
    from pytorch_r2d2_amd.engine.learner_engine import LearnerEngine
    from pytorch_r2d2_amd.engine.replay_hbm import HBMReplay
    from pytorch_r2d2_amd.envs.synthetic import VecSyntheticAtari
    cfg = _cfg(False, False, **{"actor.clear_ahead": A})
    rp = HBMReplay(cfg, DEV, capacity=E * CAP_E, n_subrings=E)
    eng = LearnerEngine(cfg, rp, DEV)
    env = VecSyntheticAtari(E, DEV, seed=3, episode_len=37, n_actions=cfg.model.n_actions)
    actor = BatchedActor(cfg, rp, env, *engine_weights(eng), seed=1)
    if graph:
        assert actor.can_capture
        actor.capture(warmup=1)      # (one real step: every kernel's first launch is eager)
    base = torch.arange(E, device=DEV)[:, None] * CAP_E
    ahead = torch.arange(A, device=DEV)[None, :]
    seen = 0
    for i in range(300):
        actor.step()
        rows = (base + (actor.head + ahead) % CAP_E).reshape(-1)
        assert int(actor.head_d.item()) == actor.head == (i + 1 + graph) % CAP_E
        assert int(rp.is_start[rows].sum().item()) == 0, i
        assert float(rp.tree[rows].abs().sum().item()) == 0.0, i
        nv = int(rp.n_valid.item())
        assert nv == int(rp.is_start.sum().item()), i
        seen = max(seen, nv)
    assert 300 > 2 * CAP_E                                 # the ring wrapped twice
    # full sub-rings hold a start every `overlap` rows except in the cleared rows and the
    # unfinished tail: the clear-ahead did not wipe the replay
    assert seen >= E * (CAP_E // cfg.replay.overlap) // 2
    _tree_consistent(rp)
    assert int(actor.infer.err.item()) == 0
    assert rp.covered_written == rp.total_written == (300 + graph) * E


def test_actor_refuses_what_clear_ahead_cannot_do():
    cfg, rp, eng, actor = _build(True, False, 2, cover=False)
    with pytest.raises(ValueError):
        actor.enable_deferred([None, None], [None, None], 16, 8)
    from pytorch_r2d2_amd.actor_batched import BatchedActor, engine_weights
    from pytorch_r2d2_amd.envs.synthetic import VecSyntheticAtari
    env = VecSyntheticAtari(E, DEV, seed=3, episode_len=37, n_actions=cfg.model.n_actions)
    big = _cfg(True, False, **{"actor.clear_ahead": CAP_E})
    with pytest.raises(ValueError):
        BatchedActor(big, rp, env, *engine_weights(eng), seed=1)
    # an actor that does not clear ahead cannot be covered; nor anything after a capture
    plain = BatchedActor(_cfg(True, False), rp, env, *engine_weights(eng), seed=1)
    with pytest.raises(ValueError):
        eng.cover_writes(plain)
    eng.capture(warmup=0)
    with pytest.raises(RuntimeError):
        eng.cover_writes(actor)


# ------------------------------------------------------------------ 2. the guard kernel alone
@pytest.mark.parametrize("delta", [0, 1, 4, 32])
def test_guard_kernel_equals_the_numpy_oracle(delta):
    from pytorch_r2d2_amd.ops._lib import check, kernels, ptr, stream_handle
    B, cap_e, T, n, n_sub, head, t_now = 8, 32, 10, 3, 2, 20, 100
    # with delta 4 offsets 16..19 are written: clear of them | first row written | last learning
    # row (16) written | window over the ring end | bootstrap-only, last row terminal |
    # bootstrap-only, last row not terminal | first row = last written | whole window behind
    starts_h = np.array([20, 17, 7, 28, 6, cap_e + 6, cap_e + 19, 2], dtype=np.int32)
    done_h = np.zeros(n_sub * cap_e, dtype=np.uint8)
    done_h[15] = 1
    starts = torch.as_tensor(starts_h, device=DEV)
    done = torch.as_tensor(done_h, device=DEV)
    head_d = torch.tensor([head], dtype=torch.int64, device=DEV)
    t_d = torch.tensor([t_now], dtype=torch.int64, device=DEV)
    want = guard_reference(starts_h, head, delta, cap_e, T, n, done_h)
    cnt = min(delta, cap_e)
    torn, boot = check_windows(starts_h[None], cap_e, T, n, [ring_offsets(head - cnt, cnt, cap_e)])
    assert want == len(torn) + len(bootstrap_violations(boot, done_h, cap_e, T))
    assert want == {0: 0, 1: 3, 4: 4, 32: 8}[delta]

    def run(check_flag):
        t_seen = torch.tensor([t_now - delta], dtype=torch.int64, device=DEV)
        err = torch.zeros(2, dtype=torch.int32, device=DEV)
        for _ in range(2):      # the second launch sees delta 0: the snapshot was refreshed
            check(kernels().r2_hoist_guard(ptr(starts), B, ptr(head_d), ptr(t_d), ptr(t_seen), cap_e,
                                           n_sub, T, n, ptr(done), check_flag, ptr(err),
                                           stream_handle()), "hoist_guard")
            torch.cuda.synchronize()
            assert int(t_seen.item()) == t_now
        return err.tolist()

    assert run(1) == [int(want > 0), want]
    assert run(0) == [0, 0]
    assert int(head_d.item()) == head and int(t_d.item()) == t_now
    assert torch.equal(starts.cpu(), torch.as_tensor(starts_h))


# ------------------------------------------------------------------ 3. the hoist is kept
@pytest.mark.parametrize("graph,M", [(g, m) for g in (True, False) for m in (1, 2, 4)])
def test_covered_actor_writes_keep_the_hoist(graph, M):
    """actor.step() x M, eng.step(), 60 rounds, clear_ahead = M: every step but the first trains
    on the batch the step before it sampled, and that batch is whole."""
    cfg, rp, eng, actor = _build(True, graph, M)
    for r in range(60):
        head = actor.head
        for _ in range(M):
            actor.step()
        taken = eng.hoisted_steps
        eng.step()
        torch.cuda.synchronize()
        _assert_states_fresh(rp, eng)
        pre = eng.hoisted_steps - taken
        assert pre == (1 if r else 0), r
        _assert_windows_whole(rp, eng, cfg, ring_offsets(head, M, CAP_E) if pre else [], r)
    assert WARM + 60 * M > CAP_E                           # the ring wrapped
    assert eng.hoisted_steps == 59
    assert eng.error_word() == 0 and eng.guard_count() == 0
    eng.check_errors()
    _tree_consistent(rp)
    assert int(actor.infer.err.item()) == 0


# ------------------------------------------------------------------ 4. the serial order's numbers
def test_covered_hoisted_step_equals_plain_step_sampling_a_step_early():
    """The hoisted step is bit-identical to the plain one in the one sampling order a pre-sample
    allows: the plain engine (eager, learner.hoist=False) samples step k+1's batch with its own
    _sample() right after step k, in front of the actor steps, and does not sample again at the
    step's start (step_eager's private ``_presampled``)."""
    M = 2
    h = _build(True, True, M)
    p = _build(False, False, M)
    cfg, rp, eng, actor = h
    _, rp0, plain, actor0 = p
    assert eng.hoist and not plain.hoist and actor0.clear_ahead == M

    def same(tag):
        torch.cuda.synchronize()
        sa, sb = _state(rp0, plain), _state(rp, eng)
        bad = [k for k in sa if not torch.equal(sa[k], sb[k])]
        assert not bad, (tag, bad)

    same("warm")
    for r in range(40):
        for _ in range(M):
            actor0.step()
            actor.step()
        plain.step_eager(_presampled=r > 0)
        eng.step()
        same(r)
        plain._sample()          # step r+1's batch, where the hoisted step r sampled it
    assert eng.hoisted_steps == 39
    assert plain.error_word() == 0 and eng.error_word() == 0 and eng.guard_count() == 0


# ------------------------------------------------------------------ 5. the host rule
def test_more_steps_than_clear_ahead_or_an_uncovered_write_drop_the_batch():
    cfg, rp, eng, actor = _build(True, True, 2)

    def round_(m):
        for _ in range(m):
            actor.step()
        taken = eng.hoisted_steps
        eng.step()
        return eng.hoisted_steps - taken

    assert [round_(2) for _ in range(3)] == [0, 1, 1]
    assert round_(3) == 0              # one covered step more than clear_ahead
    assert round_(2) == 1 and round_(0) == 1 and round_(1) == 1
    assert rp.ingest_memory(_record(20, 5), subring=0) == 20      # an uncovered writer
    assert round_(0) == 0
    assert round_(2) == 1
    torch.cuda.synchronize()
    assert eng.error_word() == 0 and eng.guard_count() == 0


# ------------------------------------------------------------------ 6. negative control
def test_guard_reports_windows_torn_by_steps_the_actor_did_not_clear_for():
    """The actor clears 1 row ahead; the engine is told 4 (its private field), so its host rule
    keeps batches across 4 actor steps that the actor's clears do not protect.  The guard's count
    equals the numpy oracle's over the run, bit 29 is set and check_errors names the guard.  (The
    step trains on stale rows of its own ring; nothing reads out of bounds.)"""
    M = 4
    cfg, rp, eng, actor = _build(True, True, 1)
    assert eng._cover["A"] == 1
    eng._cover["A"] = M
    torn = viol = 0
    for r in range(60):
        head = actor.head
        for _ in range(M):
            actor.step()
        taken = eng.hoisted_steps
        eng.step()
        torch.cuda.synchronize()
        if eng.hoisted_steps - taken:
            t_, v_ = _oracle_count(eng.starts.cpu().numpy(), head, M, rp, cfg)
            torn, viol = torn + t_, viol + v_
    assert eng.hoisted_steps == 59
    print("negative control: torn", torn, "bootstrap violations", viol, "guard", eng.guard_count())
    assert torn >= 1
    assert eng.guard_count() == torn + viol
    assert eng.error_word() & GUARD_BIT
    with pytest.raises(RuntimeError, match="hoist guard.*torn pre-sampled windows"):
        eng.check_errors()


# ------------------------------------------------------------------ 7. run_native
def test_run_native_serial_keeps_the_hoist_with_clear_ahead():
    from pytorch_r2d2_amd.runner import run_native
    kw = dict(steps=30, actor_steps_per_update=2, warmup_rows=32 * 120, capacity=32 * 600,
              log_every=30, check_every=10)
    cfg = _small_cfg(**{"actor.envs_per_actor": 32, "actor.clear_ahead": 2})
    out = run_native(cfg, **kw)          # (its check_errors calls raise on a non-zero error word)
    assert all(np.isfinite(out["losses"]))
    assert out["hoisted_steps"] >= 28
    with pytest.raises(ValueError):
        run_native(_small_cfg(**{"actor.envs_per_actor": 32, "actor.clear_ahead": 1}), **kw)
    with pytest.raises(ValueError):
        run_native(cfg, concurrent=True, **kw)
