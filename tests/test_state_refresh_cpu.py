"""The stored-state refresh oracle (pytorch_r2d2_amd/state_refresh_ref.py) against a brute-force
simulation that holds a dict per physical row and loops over every (b, c, t); the mutations the
check must reject; the knobs' refusals."""
import numpy as np
import pytest

from pytorch_r2d2_amd import state_refresh_ref as sr
from pytorch_r2d2_amd.config import get_config

H = 8
N_SUB = 3


def _starts(spec, seed):
    """Random starts with forced overlaps, a duplicate and a window that wraps its sub-ring."""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, spec.cap_e * N_SUB, spec.B)
    s[1] = s[0] + 2 if (s[0] + 2) // spec.cap_e == s[0] // spec.cap_e else s[0] - 2   # overlaps slot 0
    s[2] = s[0]                                                                       # the same start
    s[3] = (s[3] // spec.cap_e) * spec.cap_e + spec.cap_e - 3                          # wraps
    s[4] = (s[3] // spec.cap_e) * spec.cap_e + 1        # meets the wrapped tail of slot 3
    return s.astype(np.int64)


def _data(spec, seed):
    rng = np.random.default_rng(seed + 100)
    steps = spec.T + spec.n_step + 2      # long enough for every mutation's reach
    f = lambda *s: rng.standard_normal(s).astype(np.float32)   # noqa: E731
    h = {ch: f(steps, spec.B, H) for ch in sr.CHAINS}
    c = {ch: f(steps, spec.B, H) for ch in sr.CHAINS}
    cap = spec.cap_e * N_SUB
    return h, c, f(cap, 2 * H), f(cap, 2 * H)


def brute(starts, spec, h, c, hs, ths):
    """Per net a dict physical row -> (t, b); every (b, c, t) is visited in turn."""
    out = {"on": hs.copy(), "tg": ths.copy()}
    sums, rows = {}, {}
    T, ctx = spec.T, spec.burn_in if spec.context < 0 else spec.context
    for ch in ("on", "tg"):
        o = 0 if ch == "on" or spec.target_mode == "shifted" else spec.n_step
        held = {}
        for b in range(spec.B):
            base = int(starts[b]) // spec.cap_e * spec.cap_e
            for t in range(T + spec.n_step):
                j = o + t + (1 if spec.stored_state == "pre" else 0)
                if t < ctx or j > T - 1:
                    continue
                row = base + (int(starts[b]) - base + j) % spec.cap_e
                if row not in held or t > held[row][0]:      # (b ascends: a tie keeps the smaller b)
                    held[row] = (t, b)
        s = np.zeros(4)
        for row, (t, b) in held.items():
            new = np.concatenate([h[ch][t, b], c[ch][t, b]])
            d = new.astype(np.float64) - out[ch][row].astype(np.float64)
            s += [(d[:H] ** 2).sum(), (new[:H].astype(np.float64) ** 2).sum(),
                  (d[H:] ** 2).sum(), (new[H:].astype(np.float64) ** 2).sum()]
            out[ch][row] = new
        sums[ch], rows[ch] = s, len(held)
    return out, sums, rows


def _agrees(ref, want):
    out, sums, rows = want
    return (np.array_equal(ref.hs_cs, out["on"]) and np.array_equal(ref.target_hs_cs, out["tg"])
            and all(ref.rows[ch] == rows[ch] and np.allclose(ref.sums[ch], sums[ch], rtol=1e-12, atol=0)
                    for ch in sr.CHAINS))


CASES = [(st, tm, ctx) for st in ("post", "pre") for tm in ("shifted", "fixed") for ctx in (0, -1)]


@pytest.mark.parametrize("stored,tmode,context", CASES)
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_oracle_matches_brute_force(stored, tmode, context, seed):
    spec = sr.Spec(B=7, burn_in=3, learn=5, n_step=2, cap_e=16, target_mode=tmode,
                   stored_state=stored, context=context)
    starts = _starts(spec, seed)
    h, c, hs, ths = _data(spec, seed)
    want = brute(starts, spec, h, c, hs, ths)
    ref = sr.refresh_ref(starts, spec, h, c, hs, ths, "write")
    assert _agrees(ref, want)
    assert ref.rows["on"] > 0
    # several slots really met on a row, and one window really wrapped
    rows, _, _ = sr.entries(starts, spec, "on")
    assert rows.size > ref.rows["on"]
    assert (sr.ring_row(starts, spec.T - 1, spec.cap_e) < starts).any()
    # measure: the same sums, nothing written
    m = sr.refresh_ref(starts, spec, h, c, hs, ths, "measure")
    assert np.array_equal(m.hs_cs, hs) and np.array_equal(m.target_hs_cs, ths)
    assert all(np.array_equal(m.sums[ch], ref.sums[ch]) and m.rows[ch] == ref.rows[ch] for ch in sr.CHAINS)


@pytest.mark.parametrize("mutation", sr.MUTATIONS)
@pytest.mark.parametrize("stored,tmode,context", CASES)
def test_wrong_variants_are_rejected(mutation, stored, tmode, context):
    spec = sr.Spec(B=7, burn_in=3, learn=5, n_step=2, cap_e=16, target_mode=tmode,
                   stored_state=stored, context=context)
    starts = _starts(spec, 0)
    h, c, hs, ths = _data(spec, 0)
    want = brute(starts, spec, h, c, hs, ths)
    assert _agrees(sr.refresh_ref(starts, spec, h, c, hs, ths, "write"), want)
    assert not _agrees(sr.refresh_ref(starts, spec, h, c, hs, ths, "write", mutation=mutation), want)


def test_reference_mode_uses_the_fixed_offsets():
    assert sr.chain_offset("tg", "reference", 3) == sr.chain_offset("tg", "fixed", 3) == 3
    assert sr.chain_offset("tg", "shifted", 3) == sr.chain_offset("on", "fixed", 3) == 0
    with pytest.raises(ValueError):
        sr.chain_offset("nx", "fixed", 3)


def test_combine_h_is_one_fp32_add():
    from pytorch_r2d2_amd.refnum import bf16_bits, split_planes
    x = np.random.default_rng(0).standard_normal(64).astype(np.float32)
    hi, lo = split_planes(x)
    want = (hi + lo).astype(np.float32)
    assert np.array_equal(sr.combine_h(bf16_bits(hi), bf16_bits(lo)), want)
    assert np.array_equal(sr.combine_h(hi, lo), want)
    assert np.array_equal(sr.combine_h(bf16_bits(hi)), hi)


def test_drift_bound_and_check():
    spec = sr.Spec(B=7, burn_in=3, learn=5, n_step=2, cap_e=16)
    starts = _starts(spec, 0)
    h, c, hs, ths = _data(spec, 0)
    ref = sr.refresh_ref(starts, spec, h, c, hs, ths, "measure")
    n = ref.rows["on"] * H
    assert sr.drift_bound(n) == pytest.approx((n + 1) * 2.0 ** -24, rel=1e-3)
    # an fp32 accumulation in any order stays inside the bound; a doubled sum or one row more does not
    f32 = {ch: np.asarray([np.float32(v) for v in ref.sums[ch]]) for ch in sr.CHAINS}
    assert sr.check_drift(ref, H, f32, ref.rows) <= 1.0
    with pytest.raises(AssertionError):
        sr.check_drift(ref, H, {ch: 2 * f32[ch] for ch in sr.CHAINS}, ref.rows)
    with pytest.raises(AssertionError):
        sr.check_drift(ref, H, f32, {"on": ref.rows["on"] + 1, "tg": ref.rows["tg"]})
    r = sr.drift_ratio(ref.sums["on"])
    assert r["h"] == pytest.approx(np.sqrt(ref.sums["on"][0] / ref.sums["on"][1]))
    assert sr.drift_ratio(np.zeros(4)) == {"h": 0.0, "c": 0.0}


def test_config_knobs_and_refusals():
    cfg = get_config("atari57")
    assert cfg.replay.state_refresh == "off" and cfg.replay.state_refresh_context == -1
    cfg = get_config("atari57", **{"replay.state_refresh": "write", "replay.state_refresh_context": "7"})
    assert cfg.replay.state_refresh == "write" and cfg.replay.state_refresh_context == 7
    assert sr.check_config("off", -1, 40, 40) == 40
    assert sr.check_config("write", 0, 40, 40) == 0
    assert sr.check_config("measure", 79, 40, 40) == 79
    for mode, ctx in (("on", -1), ("Write", 0), ("write", 80), ("write", -2), ("measure", 1000)):
        with pytest.raises(ValueError):
            sr.check_config(mode, ctx, 40, 40)


def test_main_passes_the_knob_to_the_native_runner(monkeypatch):
    import main
    from pytorch_r2d2_amd import runner
    got = {}
    monkeypatch.setattr(runner, "run_native", lambda cfg, **kw: got.update(cfg=cfg) or {})
    main.run(["--mode", "native", "--config", "pong", "--steps", "1", "--set", "replay.state_refresh=write",
              "replay.state_refresh_context=2"])
    assert got["cfg"].replay.state_refresh == "write" and got["cfg"].replay.state_refresh_context == 2


def test_learn_check_passes_the_knob():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "learn_check.py")
    spec = importlib.util.spec_from_file_location("learn_check_tool", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    cfg = mod.make_cfg(mod.parse(["--memory", "--state-refresh", "write"]), "fp32")
    assert cfg.replay.state_refresh == "write" and cfg.env.cue_only_first
    assert mod.make_cfg(mod.parse(["--memory"]), "fp32").replay.state_refresh == "off"


def test_engine_refusals_need_no_gpu():
    """The engine's own refusals are raised before it allocates anything."""
    from pytorch_r2d2_amd.engine.learner_engine import state_refresh_plan
    ok = get_config("atari57", **{"replay.state_refresh": "write"})
    plan = state_refresh_plan(ok, dp=False)
    assert plan["mode"] == "write" and plan["context"] == 40 and plan["o_tg"] == 5 and plan["shift"] == 1
    assert state_refresh_plan(get_config("atari57"), dp=True) is None        # off: nothing to refuse
    with pytest.raises(NotImplementedError, match="data-parallel"):
        state_refresh_plan(ok, dp=True)
    with pytest.raises(ValueError, match="zero_stored_state"):
        state_refresh_plan(ok.replace(**{"learner.zero_stored_state": True}), dp=False)
    # measuring the drift of states the learner ignores is allowed
    assert state_refresh_plan(ok.replace(**{"learner.zero_stored_state": True,
                                            "replay.state_refresh": "measure"}), dp=False)["mode"] == "measure"
    with pytest.raises(ValueError, match="state_refresh"):
        state_refresh_plan(ok.replace(**{"replay.state_refresh": "yes"}), dp=False)
    with pytest.raises(ValueError, match="state_refresh_context"):
        state_refresh_plan(ok.replace(**{"replay.state_refresh_context": 80}), dp=False)


def test_set_hs_cs_scatters_rows_on_the_native_replay():
    """HBMReplay.set_hs_cs: the reference's ReplayMemory.set_hs_cs scatter (PARITY C16), on the CPU device."""
    import torch
    from pytorch_r2d2_amd.engine.replay_hbm import HBMReplay
    cfg = get_config("atari57", **{"model.hidden": 64, "replay.n_subrings": 2})
    rp = HBMReplay(cfg, "cpu", capacity=64, frame_bytes=4)
    g = torch.Generator().manual_seed(0)
    rp.hs_cs.normal_(generator=g)
    rp.target_hs_cs.normal_(generator=g)
    before, before_t = rp.hs_cs.clone(), rp.target_hs_cs.clone()
    rows = [5, 40, 63]
    hs, cs, ths, tcs = (torch.randn(3, 64, generator=g) for _ in range(4))
    rp.set_hs_cs(rows, hs, cs, ths, tcs)
    assert torch.equal(rp.hs_cs[rows], torch.cat([hs, cs], 1))
    assert torch.equal(rp.target_hs_cs[rows], torch.cat([ths, tcs], 1))
    keep = torch.ones(64, dtype=torch.bool)
    keep[rows] = False
    assert torch.equal(rp.hs_cs[keep], before[keep]) and torch.equal(rp.target_hs_cs[keep], before_t[keep])
    with pytest.raises(ValueError):
        rp.set_hs_cs([64], hs[:1], cs[:1], ths[:1], tcs[:1])
    with pytest.raises(ValueError):
        rp.set_hs_cs(rows, hs[:2], cs, ths, tcs)
