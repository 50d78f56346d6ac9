"""The hoisted learner step (learner.hoist) against a replay that is being WRITTEN between steps,
as every training driver does (runner.run_native: actor steps then a learner step; the ingest
loops).  Step k samples step k+1's batch on a side stream; a write between the two steps makes that
batch stale (overwritten windows, another tree), so the engine must drop it and sample at the
step's start, which keeps the step bit-identical to the plain serial one (the reference learner
samples at the start of every train()).  A replay nobody wrote must still get the pre-sampled
batch (``hoisted_steps``).

Small configuration throughout (tests/test_native_gpu.py::_small_cfg: burn-in 4, learn 6, overlap
5, n = 3, B = 8), 16 envs of VecSyntheticAtari(episode_len=37), one sub-ring of 128 rows per env:
the ring wraps several times in a run."""
import pytest
import torch

from gpu_support import engine_state
from pytorch_r2d2_amd.engine.replay_check import bootstrap_violations, check_windows, ring_offsets
from test_native_gpu import _record, _small_cfg, _tree_consistent

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
E, CAP_E, WARM = 16, 128, 80


def _cfg(hoist, graph, **over):
    kw = {"seed": 1234, "actor.envs_per_actor": E, "learner.target_update_interval": 7,
          "learner.hoist": hoist, "learner.use_graph": graph}
    kw.update(over)
    return _small_cfg(**kw)


def _live(hoist, graph=True, **over):
    """Engine + its own replay + its own batched actor (same seeds for every call) reading the
    engine's live weights; WARM actor steps fill the first rows of every sub-ring."""
    from pytorch_r2d2_amd.actor_batched import BatchedActor, engine_weights
    from pytorch_r2d2_amd.engine.learner_engine import LearnerEngine
    from pytorch_r2d2_amd.engine.replay_hbm import HBMReplay
    from pytorch_r2d2_amd.envs.synthetic import VecSyntheticAtari
    cfg = _cfg(hoist, graph, **over)
    rp = HBMReplay(cfg, DEV, capacity=E * CAP_E, n_subrings=E)
    eng = LearnerEngine(cfg, rp, DEV)
    env = VecSyntheticAtari(E, DEV, seed=3, episode_len=37, n_actions=cfg.model.n_actions)
    on, tg = engine_weights(eng)
    actor = BatchedActor(cfg, rp, env, on, tg, seed=1)
    for _ in range(WARM):
        actor.step()
    assert int(rp.n_valid.item()) >= 4 * cfg.learner.batch_size
    if graph:
        eng.capture(warmup=0)
    return cfg, rp, eng, actor


def _state(rp, eng):
    out = engine_state(rp, eng)      # weights, moments, packs, priority, tree, step, loss
    out.update(is_start=rp.is_start, n_valid=rp.n_valid, starts=eng.starts)
    return out


def _assert_same(tag, a, b):
    torch.cuda.synchronize()
    sa, sb = _state(*a), _state(*b)
    bad = [k for k in sa if not torch.equal(sa[k], sb[k])]
    assert not bad, (tag, bad)


def _assert_states_fresh(rp, eng):
    """The stored recurrent states the step used equal a gather of the replay's rows at its starts
    now (nothing wrote the replay since the step trained)."""
    H = rp.H
    s = eng.starts.long()
    base = s - s % rp.cap_e
    _, states = eng._sample_dst(eng._cur)
    for hs_cs, off, h, c in states:
        rows = base + (s - base + int(off)) % rp.cap_e
        src = hs_cs[rows]
        assert torch.equal(h, src[:, :H].to(h.dtype)), ("h0", int(off))
        assert torch.equal(c, src[:, H:]), ("c0", int(off))


def _assert_windows_whole(rp, eng, cfg, written, tag):
    starts = eng.starts.cpu().numpy()[None]
    torn, boot = check_windows(starts, rp.cap_e, cfg.replay.seq_len, cfg.replay.n_step, [written])
    assert not torn, (tag, torn)
    if boot:
        bad = bootstrap_violations(boot, rp.done.cpu().numpy(), rp.cap_e, cfg.replay.seq_len)
        assert not bad, (tag, bad)


def test_plain_step_with_actor_writes_is_deterministic():
    """Control for the comparisons below: two PLAIN engines, each with its own replay and actor
    (same seeds), actor.step() x 2 then eng.step(), 40 rounds: every compared tensor is bitwise
    equal after every round (the actor's clears reach the dirty list in atomicAdd order)."""
    a = _live(False)
    b = _live(False)
    assert not a[2].hoist and not b[2].hoist
    _assert_same("warm", a[1:3], b[1:3])
    for r in range(40):
        for _, rp, eng, actor in (a, b):
            actor.step()
            actor.step()
            eng.step()
        _assert_same(r, a[1:3], b[1:3])
    assert a[2].error_word() == 0 and b[2].error_word() == 0


@pytest.mark.parametrize("graph,M,early", [(g, m, False) for g in (True, False) for m in (1, 2, 4)]
                         + [(True, 2, True), (False, 2, True)])
def test_hoisted_step_equals_plain_step_under_actor_writes(graph, M, early):
    """actor.step() x M, then eng.step(), 60 rounds, target sync every 7 steps, nobody calls
    invalidate_hoist().  After every round the hoisted engine's state equals the plain one's
    bitwise, the stored states it trained on are the replay's, and no window it trained on met
    the rows written since it was sampled (oracle: engine/replay_check.py, fed the host write
    heads).  Every step here follows a write, and a write makes the pre-sampled batch stale, so
    the engine must have taken none: hoisted_steps == 0."""
    p = _live(False, graph)
    h = _live(True, graph, **{"learner.hoist_early_fork": early})
    cfg, rp, eng, actor = h
    assert eng.hoist and not p[2].hoist
    _assert_same("warm", p[1:3], h[1:3])
    for r in range(60):
        head = actor.head
        for _, _, e_, a_ in (p, h):
            for _ in range(M):
                a_.step()
        taken = eng.hoisted_steps
        p[2].step()
        eng.step()
        _assert_same(r, p[1:3], h[1:3])
        _assert_states_fresh(rp, eng)
        # rows written between this batch's sampling and its training: the M rows in front of
        # the step when the previous step sampled it, none when the step sampled at its start
        pre = eng.hoisted_steps - taken
        assert pre in (0, 1)
        _assert_windows_whole(rp, eng, cfg, ring_offsets(head, M, CAP_E) if pre else [], r)
    assert WARM + 60 * M > CAP_E and actor.head == (WARM + 60 * M) % CAP_E     # wrapped
    assert p[2].error_word() == 0 and eng.error_word() == 0
    _tree_consistent(p[1])
    _tree_consistent(rp)
    assert eng.hoisted_steps == 0


@pytest.mark.parametrize("how", ["step", "run_steps"])
def test_static_replay_keeps_the_hoist(how):
    """Nothing writes the replay between steps (the benchmark's loop): every step but the first
    trains on the batch the step before it sampled."""
    cfg, rp, eng, actor = _live(True, True, **{"learner.target_update_interval": 1000,
                                               "learner.graph_chunk": 4})
    assert eng.hoist
    steps = 13
    if how == "step":
        for _ in range(steps):
            eng.step()
    else:
        eng.run_steps(steps)
        assert getattr(eng, "chunks_run", 0) >= 2
    torch.cuda.synchronize()
    assert eng.steps_done == steps and eng.hoisted_steps == steps - 1
    assert eng.error_word() == 0


def test_hoisted_step_equals_plain_step_under_ingest():
    """rp.ingest_memory between steps (the ingest drivers), a 60-row record in front of every 3rd
    step, alternating between two sub-rings of 300 rows so both wrap: bitwise the plain engine,
    whole windows, and the steps with no write in front of them still take the pre-sampled
    batch."""
    from pytorch_r2d2_amd.engine.learner_engine import LearnerEngine
    from pytorch_r2d2_amd.engine.replay_hbm import HBMReplay
    cap_e = 300
    pairs = []
    for hoist in (False, True):
        cfg = _cfg(hoist, True)
        rp = HBMReplay(cfg, DEV, capacity=2 * cap_e, n_subrings=2)
        assert rp.ingest_memory(_record(200, 1), subring=0) == 200
        assert rp.ingest_memory(_record(150, 2), subring=1) == 150
        eng = LearnerEngine(cfg, rp, DEV)
        eng.capture(warmup=0)
        pairs.append((cfg, rp, eng))
    (_, rp0, plain), (cfg, rp, eng) = pairs
    assert eng.hoist and not plain.hoist
    heads = [200, 150]
    expect = wrote = 0
    for i in range(20):
        written = {}
        if i and i % 3 == 0:
            sub = wrote & 1
            m = _record(60, 10 + i)
            for r_ in (rp0, rp):
                assert r_.ingest_memory(m, subring=sub) == 60
            written = {sub: ring_offsets(heads[sub], 60, cap_e)}
            heads[sub] = (heads[sub] + 60) % cap_e
            wrote += 1
        elif i:
            expect += 1
        taken = eng.hoisted_steps
        plain.step()
        eng.step()
        _assert_same(i, (rp0, plain), (rp, eng))
        _assert_states_fresh(rp, eng)
        pre = eng.hoisted_steps - taken
        assert pre == (0 if written or i == 0 else 1), i
        _assert_windows_whole(rp, eng, cfg, written if pre else [], i)
    assert wrote == 6 and heads == [80, 30]        # both sub-rings wrapped
    assert eng.hoisted_steps == expect == 13
    assert plain.error_word() == 0 and eng.error_word() == 0
    assert int(rp.ingest_err.item()) == 0
    _tree_consistent(rp0)
    _tree_consistent(rp)


def test_chunked_run_steps_stops_at_a_write():
    """learner.graph_chunk = 4: run_steps(8), one actor step, run_steps(8), against the plain
    loop.  Step 8 is even and follows a hoisted step, but the replay was written in front of it,
    so it must not start a chunk replay: it runs alone and samples at its start.  Chunks: steps
    2-5 and 10-13 (0 and 8 sample at their start, odd steps never start a chunk, 6-7 and 14-15
    are too few)."""
    over = {"learner.target_update_interval": 1000, "learner.graph_chunk": 4}
    p = _live(False, True, **over)
    h = _live(True, True, **over)
    eng = h[2]
    assert eng.hoist and eng._cgraph is not None
    for part in range(2):
        for _ in range(8):
            p[2].step()
        eng.run_steps(8)
        _assert_same(part, p[1:3], h[1:3])
        _assert_states_fresh(h[1], eng)
        if part == 0:
            assert eng.chunks_run == 1 and eng.hoisted_steps == 7
            p[3].step()
            h[3].step()
    assert eng.steps_done == p[2].steps_done == 16
    assert eng.chunks_run == 2
    assert eng.hoisted_steps == 14
    assert p[2].error_word() == 0 and eng.error_word() == 0
