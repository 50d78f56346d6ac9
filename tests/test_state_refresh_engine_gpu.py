"""replay.state_refresh in the learner engine: the launch at the top of ``_forward_tail`` writes
what the oracle (pytorch_r2d2_amd/state_refresh_ref.py) says from the engine's own chains, those
states are the float64 net's, the hoisted step stays bitwise the plain one with it, "off" and
"measure" leave the replay alone, a batch replayed with frozen weights reports no drift, the serial
runner logs it, and every refusal is raised."""
import numpy as np
import pytest
import torch

from gpu_support import engine_state, pong_small, rel_err, stop_after_a_gpu_error  # noqa: F401
from pytorch_r2d2_amd import state_refresh_ref as sr
from pytorch_r2d2_amd.utils.metrics import read_jsonl

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def _engine(mode, hoist=False, graph=False, net=None, capacity=64000, **kw):
    """B 8, burn-in 4 + learn 4, n 2 on a static synthetic replay (the shapes of test_hoist_gpu)."""
    from pytorch_r2d2_amd.config import get_config
    from pytorch_r2d2_amd.engine.learner_engine import LearnerEngine
    from pytorch_r2d2_amd.engine.replay_hbm import HBMReplay
    over = {"seed": 1234, "learner.batch_size": 8, "learner.hoist": hoist, "learner.use_graph": graph,
            "learner.target_update_interval": 3, "replay.burn_in": 4, "replay.learn": 4,
            "replay.overlap": 4, "replay.n_step": 2, "replay.state_refresh": mode}
    over.update(kw)
    cfg = get_config("atari57", **over)
    rp = HBMReplay(cfg, DEV, capacity=capacity)
    rp.fill_synthetic(episode_len=200, seed=3)
    eng = LearnerEngine(cfg, rp, DEV, init_module=net)
    return cfg, rp, eng


def _spec(cfg, rp):
    rc = cfg.replay
    return sr.Spec(B=cfg.learner.batch_size, burn_in=rc.burn_in, learn=rc.learn, n_step=rc.n_step,
                   cap_e=rp.cap_e, target_mode=cfg.learner.target_mode, stored_state=rc.stored_state,
                   context=rc.state_refresh_context)


def _chains(eng):
    """The engine's chains as the oracle takes them: fp32 h (hi + lo, one add) and c per chain."""
    h, c = {}, {}
    for ch in sr.CHAINS:
        bits = lambda t: t.view(torch.int16).cpu().numpy().view(np.uint16)   # noqa: E731
        lo = eng.hseq_lo.get(ch)
        h[ch] = sr.combine_h(bits(eng.hseq[ch]), bits(lo) if lo is not None else None)
        c[ch] = eng.cseq[ch].cpu().numpy()
    return h, c


def _drift_words(eng):
    return eng.sr_out.cpu().numpy()


# ---- (a) the engine writes what the oracle says, from its own chains
@pytest.mark.parametrize("dtype,tmode,stored,hoist", [("fp32", "fixed", "pre", True), ("fp32", "shifted", "post", False),
                                                      ("bf16", "fixed", "post", False), ("fp32", "reference", "pre", False)])
def test_write_step_matches_oracle(dtype, tmode, stored, hoist):
    cfg, rp, eng = _engine("write", hoist=hoist, **{"learner.compute_dtype": dtype, "learner.target_mode": tmode,
                                                    "replay.stored_state": stored})
    assert eng.hoist == hoist
    hs0, ths0 = rp.hs_cs.cpu().numpy(), rp.target_hs_cs.cpu().numpy()
    eng.step_eager()
    torch.cuda.synchronize()
    assert eng.error_word() == 0
    h, c = _chains(eng)
    ref = sr.refresh_ref(eng.starts.cpu().numpy(), _spec(cfg, rp), h, c, hs0, ths0, "write")
    assert ref.rows["on"] > 0 and ref.rows["tg"] > 0
    # every row: the refreshed ones equal the oracle's bits, all others their old bits
    assert np.array_equal(rp.hs_cs.cpu().numpy().view(np.uint32), ref.hs_cs.view(np.uint32))
    assert np.array_equal(rp.target_hs_cs.cpu().numpy().view(np.uint32), ref.target_hs_cs.view(np.uint32))
    assert (ref.hs_cs != hs0).any(1).sum() == ref.rows["on"]
    w = _drift_words(eng)
    sr.check_drift(ref, rp.H, {"on": w[0:4], "tg": w[4:8]}, {"on": w[8], "tg": w[9]})
    d = eng.diagnostics()
    assert d["state_rows"] == ref.rows["on"] + ref.rows["tg"]
    want = sr.drift_ratio(ref.sums["on"])
    assert d["state_drift_h"] == pytest.approx(want["h"], rel=1e-3) and d["state_drift_c"] == pytest.approx(want["c"], rel=1e-3)
    want = sr.drift_ratio(ref.sums["tg"])
    assert d["state_drift_h_tg"] == pytest.approx(want["h"], rel=1e-3)
    assert d["state_drift_c_tg"] == pytest.approx(want["c"], rel=1e-3)
    assert int(eng.sr_ticket.item()) == 0


# ---- (b) semantics: the refreshed states are the float64 net's, at the rows the rule names
@pytest.mark.parametrize("stored", ["pre", "post"])
def test_refreshed_states_are_the_float64_chain(stored):
    """A float64 QNet chain from the OLD stored start state over the window's frames; the state of
    chain step t must sit at row offset o + t (post) / o + t + 1 (pre), computed here without the
    oracle's row rule.  Tolerance: 2e-5 relative, that of
    test_split_gpu.py::test_engine_fp32_forward_activations for the same activations."""
    from pytorch_r2d2_amd.learner_ref import batch_from_hbm
    from pytorch_r2d2_amd.models import QNet
    from pytorch_r2d2_amd.config import get_config
    base_cfg = get_config("atari57")
    torch.manual_seed(7)
    net = QNet("cpu", base_cfg.model, base_cfg.env)
    cfg, rp, eng = _engine("write", net=net, **{"replay.stored_state": stored, "replay.state_refresh_context": 1})
    assert eng.sp and cfg.learner.target_mode == "fixed"
    eng._sample()
    torch.cuda.synchronize()
    b = batch_from_hbm(rp, eng.starts, eng.probs, cfg, "cpu")       # the old stored states
    eng._forward_rest()
    torch.cuda.synchronize()
    assert eng.error_word() == 0
    T, n, H, cap_e = cfg.replay.seq_len, cfg.replay.n_step, rp.H, rp.cap_e
    s = eng.starts.long().cpu()
    # the batch's windows are disjoint, so every slot owns its rows (the owner rule is (a)'s subject)
    rows, _, _ = sr.entries(s.numpy(), _spec(cfg, rp), "on")
    assert rows.size == np.unique(rows).size, "the sampled windows overlap: pick another seed"
    net64 = net.double()          # online == target at construction
    obs = b.obs.double()
    shift = 1 if stored == "pre" else 0
    with torch.no_grad():
        for arr, o, h0, c0 in ((rp.hs_cs, 0, b.h0, b.c0), (rp.target_hs_cs, n, b.th0, b.tc0)):
            x = obs[o: o + T]
            X = net64.torso(x.reshape(T * len(s), *x.shape[2:])).reshape(T, len(s), -1)
            hs, cs = net64.lstm_seq(X, h0.double(), c0.double())
            ts = [t for t in range(1, T) if o + t + shift <= T - 1]
            assert len(ts) >= 2
            got, want = [], []
            for t in ts:
                rows = (s // cap_e) * cap_e + (s % cap_e + o + t + shift) % cap_e
                got.append(arr[rows.to(DEV)].cpu().double())
                want.append(torch.cat([hs[t], cs[t]], dim=1))
            got, want = torch.stack(got), torch.stack(want)
            assert rel_err(got[..., :H], want[..., :H]) < 2e-5, (o, rel_err(got[..., :H], want[..., :H]))
            assert rel_err(got[..., H:], want[..., H:]) < 2e-5, (o, rel_err(got[..., H:], want[..., H:]))


# ---- (c) hoisted == plain, bitwise, with a target sync
def _all_state(rp, eng):
    out = engine_state(rp, eng)
    out.update(hs_cs=rp.hs_cs, target_hs_cs=rp.target_hs_cs, drift=eng.sr_out, ticket=eng.sr_ticket)
    return out


def _same(tag, a, b):
    torch.cuda.synchronize()
    sa, sb = _all_state(*a), _all_state(*b)
    bad = [k for k in sa if not torch.equal(sa[k], sb[k])]
    assert not bad, (tag, bad)


@pytest.mark.parametrize("how", ["eager", "graph", "chunk"])
def test_hoisted_step_is_bitwise_the_plain_step_with_refresh(how):
    graph = how != "eager"
    kw = {"learner.graph_chunk": 2}
    _, rp0, plain = _engine("write", hoist=False, graph=graph, **kw)
    _, rp1, hoist = _engine("write", hoist=True, graph=graph, **kw)
    assert hoist.hoist and not plain.hoist
    hs0 = rp1.hs_cs.clone()
    if graph:
        plain.capture(warmup=0)
        hoist.capture(warmup=0)
    if how == "chunk":
        for i in range(5):
            plain.step()
            plain.step()
            hoist.run_steps(2)
            _same(i, (rp0, plain), (rp1, hoist))
        assert hoist.chunks_run >= 1
    else:
        for i in range(10):
            if i == 6:
                hoist.invalidate_hoist()
            plain.step()
            hoist.step()
            _same(i, (rp0, plain), (rp1, hoist))
        assert hoist.hoisted_steps >= 7
    assert plain.error_word() == 0 and hoist.error_word() == 0
    assert not torch.equal(rp1.hs_cs, hs0)
    assert hoist.diagnostics()["state_rows"] > 0


# ---- (d) off and measure leave the replay's states alone; measure changes nothing else either
def test_off_and_measure_write_nothing():
    runs = {}
    for mode in ("off", "measure"):
        _, rp, eng = _engine(mode, hoist=True, graph=True)
        hs0, ths0 = rp.hs_cs.clone(), rp.target_hs_cs.clone()
        eng.capture(warmup=0)
        for _ in range(10):
            eng.step()
        torch.cuda.synchronize()
        assert eng.error_word() == 0
        assert torch.equal(rp.hs_cs, hs0) and torch.equal(rp.target_hs_cs, ths0), mode
        runs[mode] = engine_state(rp, eng)
        d = eng.diagnostics()
        if mode == "off":
            assert not hasattr(eng, "sr_out") and not [k for k in d if k.startswith("state_")]
        else:
            assert d["state_rows"] > 0 and d["state_drift_h"] > 0 and d["state_drift_c_tg"] > 0
    bad = [k for k in runs["off"] if not torch.equal(runs["off"][k], runs["measure"][k])]
    assert not bad, bad


# ---- (e) frozen weights, the same batch twice: the second pass finds its own states
@pytest.mark.parametrize("stored", ["pre", "post"])
def test_replayed_batch_with_frozen_weights_has_no_drift(stored):
    cfg, rp, eng = _engine("write", **{"learner.lr": 0.0, "replay.stored_state": stored})
    assert sr.check_config("write", cfg.replay.state_refresh_context, 4, 4) >= 1
    eng._sample()
    torch.cuda.synchronize()
    rows, _, _ = sr.entries(eng.starts.cpu().numpy(), _spec(cfg, rp), "on")
    assert rows.size == np.unique(rows).size, "the sampled windows overlap: pick another seed"
    master = eng.master.clone()
    eng.step_eager(_presampled=True)
    first = eng.diagnostics()
    assert first["state_rows"] > 0 and first["state_drift_h"] > 0 and first["state_drift_c"] > 0
    assert torch.equal(eng.master, master)
    eng.step_eager(_presampled=True)
    d = eng.diagnostics()
    assert eng.error_word() == 0
    assert d["state_rows"] == first["state_rows"]
    for k in ("state_drift_h", "state_drift_c", "state_drift_h_tg", "state_drift_c_tg"):
        assert d[k] == 0.0, (k, d[k])


# ---- (f) the serial runner
def test_run_native_serial_with_write(tmp_path, monkeypatch):
    from pytorch_r2d2_amd import actor_batched, runner
    from pytorch_r2d2_amd.engine import learner_engine
    from pytorch_r2d2_amd.engine.replay_check import bootstrap_violations, check_windows, ring_offsets
    made = {}

    class Eng(learner_engine.LearnerEngine):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made["eng"] = self

    class Act(actor_batched.BatchedActor):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made["actor"] = self

    monkeypatch.setattr(learner_engine, "LearnerEngine", Eng)
    monkeypatch.setattr(actor_batched, "BatchedActor", Act)
    cfg = pong_small(**{"replay.state_refresh": "write"})
    seen = []

    def on_step(it):
        eng, actor = made["eng"], made["actor"]
        seen.append((eng.starts.cpu().numpy().copy(), eng.hoisted_steps, (actor.head - 1) % eng.replay.cap_e))

    path = str(tmp_path / "m.jsonl")
    out = runner.run_native(cfg, steps=40, warmup_rows=16 * 40, capacity=16 * 128, log_every=10,
                            metrics_path=path, on_step=on_step)
    eng = made["eng"]
    assert eng.error_word() == 0 and len(seen) == 40 and np.isfinite(out["losses"]).all()
    recs = [r for r in read_jsonl(path) if r["kind"] == "native"]
    assert len(recs) == 4 and all(r["state_rows"] > 0 for r in recs)
    assert all(np.isfinite(r[k]) for r in recs for k in ("state_drift_h", "state_drift_c", "state_drift_h_tg",
                                                         "state_drift_c_tg"))
    # the windows the steps trained on (and refreshed) met no row written since they were sampled
    rc, cap_e = cfg.replay, eng.replay.cap_e
    taken, written = 0, []
    for _, hoisted, head in seen:
        written.append(ring_offsets(head, 1, cap_e) if hoisted > taken else [])
        taken = hoisted
    torn, boot = check_windows(np.stack([s for s, _, _ in seen]), cap_e, rc.seq_len, rc.n_step, written)
    assert not torn
    assert not bootstrap_violations(boot, eng.replay.done.cpu().numpy(), cap_e, rc.seq_len)


# ---- the concurrent driver: the lookahead keeps the actor off every row the launch writes
def test_concurrent_driver_with_write():
    """engine/concurrent.py, shared chip, hoisted step, "write", 40 rounds of 2 actor steps beside
    a learner step: no window a step trained on (and refreshed) meets the rows written since it was
    sampled (engine/replay_check.py, as test_native_gpu.py checks the driver without the knob), and
    the rows the last step owns still hold that step's states bit for bit although an actor round
    ran beside it."""
    from test_native_gpu import _concurrent_setup
    from pytorch_r2d2_amd.engine.replay_check import bootstrap_violations, check_windows, ring_offsets
    M, R = 2, 40
    cfg, rp, eng, actor, drv, _ = _concurrent_setup(masked=False, M=M, **{"replay.state_refresh": "write"})
    assert eng.hoist and eng.writes_covered and eng._refresh["mode"] == "write"
    hist = torch.zeros(R, cfg.learner.batch_size, dtype=torch.int32, device=DEV)
    taken = []

    def log_starts(i):
        if i < R:
            hist[i].copy_(eng.starts)
            taken.append(eng.hoisted_steps)
    drv.on_learner_step = log_starts
    drv.run(R)
    drv.finish()
    drv.check_errors()
    assert eng.error_word() == 0
    cap_e = rp.cap_e
    assert drv.rounds * M + drv.heads[0] < cap_e
    pre = [b - a == 1 for a, b in zip([0] + taken[:-1], taken)]
    written = []
    for r in range(R):
        w = ring_offsets(drv.heads[r], M, cap_e)
        if pre[r]:
            w = np.concatenate([ring_offsets(drv.heads[r - 1], M, cap_e), w])
        written.append(w)
    torn, boot = check_windows(hist.cpu().numpy(), cap_e, cfg.replay.seq_len, cfg.replay.n_step, written)
    assert not torn, torn[:8]
    assert not bootstrap_violations(boot, rp.done.cpu().numpy(), cap_e, cfg.replay.seq_len)
    # the last step's refresh is in the replay
    h, c = _chains(eng)
    spec = _spec(cfg, rp)
    assert np.array_equal(eng.starts.cpu().numpy(), hist[R - 1].cpu().numpy())
    for ch, arr in (("on", rp.hs_cs), ("tg", rp.target_hs_cs)):
        o = sr.owners(eng.starts.cpu().numpy(), spec, ch)
        assert o.rows.size > 0
        want = np.concatenate([h[ch][o.t, o.b], c[ch][o.t, o.b]], axis=1)
        got = arr[torch.as_tensor(o.rows, device=DEV)].cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), ch
    assert eng.diagnostics()["state_rows"] > 0


# ---- (g) every refusal
def test_refusals():
    from pytorch_r2d2_amd.config import get_config
    from pytorch_r2d2_amd.engine.learner_engine import LearnerEngine
    from pytorch_r2d2_amd.engine.replay_hbm import HBMReplay
    with pytest.raises(ValueError, match="state_refresh"):
        _engine("on")
    with pytest.raises(ValueError, match="state_refresh_context"):
        _engine("write", **{"replay.state_refresh_context": 8})
    with pytest.raises(ValueError, match="state_refresh_context"):
        _engine("measure", **{"replay.state_refresh_context": -2})
    with pytest.raises(ValueError, match="zero_stored_state"):
        _engine("write", **{"learner.zero_stored_state": True})
    _, _, eng = _engine("measure", **{"learner.zero_stored_state": True})
    assert eng._refresh["mode"] == "measure"
    # a data-parallel engine (one forced rank): refused before the process group is ever used
    cfg = get_config("atari57", **{"learner.batch_size": 8, "replay.state_refresh": "write", "dist.force_dp": True})
    rp = HBMReplay(cfg, DEV, capacity=64000)
    with pytest.raises(NotImplementedError, match="data-parallel"):
        LearnerEngine(cfg, rp, DEV, process_group=object())
    with pytest.raises(NotImplementedError, match="data-parallel"):
        LearnerEngine(cfg.replace(**{"replay.state_refresh": "measure"}), rp, DEV, process_group=object())
    # a sub-ring shorter than the window
    cfg = get_config("atari57", **{"learner.batch_size": 8, "replay.state_refresh": "write", "replay.n_subrings": 1})
    with pytest.raises(ValueError, match="sub-ring"):
        LearnerEngine(cfg, HBMReplay(cfg, DEV, capacity=64), DEV)
