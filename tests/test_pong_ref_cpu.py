"""The Pong-like game's oracle (pytorch_r2d2_amd/pong_ref.py) under its own control, on the CPU:
scripted single frames against hand-computed integers, the two ways an episode ends, the render,
a play control (no-op loses, a ball tracker wins, every game ends on points), the env classes and
``make_device_env``.  It also holds the scripted run that tests/test_pong_gpu.py replays on the
kernel, with the proof that the run covers every branch and that the comparison rejects two wrong
games (a wall one row off, the spin drawn with the serve's salt)."""
import ctypes
from dataclasses import replace

import numpy as np
import pytest
import torch

from pytorch_r2d2_amd import pong_ref as pr
from pytorch_r2d2_amd.config import EnvConfig, get_config
from pytorch_r2d2_amd.envs import (DevicePongEnv, VecPong, VecSyntheticAtari, make_device_env,
                                   make_env)
from pytorch_r2d2_amd.envs.pong_device import PongArgs
from pytorch_r2d2_amd.pong_ref import PA, PO, SA, SO, T, TIMER, VX, VY, X, Y
from pytorch_r2d2_amd.refnum import mix64

Q = 256
SEED = 7


# ================================================================== scripted single frames
def _one(action=0, lapse=0, **cols):
    """One env with the given state columns (ball in play unless TIMER is given), one raw frame."""
    ref = pr.PongRef(1, seed=SEED, lapse=lapse)
    ref.state[0, TIMER] = 0
    for name, v in cols.items():
        ref.state[0, getattr(pr, name)] = v
    k0 = int(ref.k[0])
    r = ref._frame(np.array([action]), np.array([True]))
    assert int(ref.k[0]) == k0 + 1
    return ref, ref.state[0].tolist(), int(r[0])


def _spin(ref):
    h = int(pr.env_hash(ref.seed, ref.k, np.uint64(2 << 32))[0])
    return (h % 3 - 1) * 48


def _serve_vy(ref):
    h = int(pr.env_hash(ref.seed, ref.k, np.uint64(3 << 32))[0])
    return (h % 5 - 2) * 72


def test_hash_is_env_hip_s():
    """splitmix64's first output for state 0 is the published 0xE220A8397B1DCDAF; env_hash nests
    two of them as env.hip does."""
    assert int(mix64(np.array([0], dtype=np.uint64))[0]) == 0xE220A8397B1DCDAF
    a, b, seed = 5, (2 << 32) + 1, 0x1234
    inner = int(mix64(np.array([(a * 0x9E3779B97F4A7C15 + b) % 2 ** 64], dtype=np.uint64))[0])
    want = int(mix64(np.array([seed ^ inner], dtype=np.uint64))[0]) >> 32
    assert int(pr.env_hash(seed, [a], [b])[0]) == want


def test_wall_bounce_top_and_bottom():
    _, s, r = _one(X=30 * Q, Y=6 * Q + 50, VX=192, VY=-120)
    assert (s[X], s[Y], s[VX], s[VY], r) == (7872, 1606, 192, 120, 0)     # 1466 -> 2*1536 - 1466
    _, s, r = _one(X=30 * Q, Y=80 * Q - 10, VX=-192, VY=100)
    assert (s[X], s[Y], s[VX], s[VY], r) == (7488, 20390, -192, -100, 0)  # 20570 -> 2*20480 - 20570
    # exactly on the wall rows: no reflection
    _, s, _ = _one(X=30 * Q, Y=6 * Q + 120, VX=192, VY=-120)
    assert (s[Y], s[VY]) == (1536, -120)


def test_agent_paddle_hit_and_sweep():
    # leading edge 19912 -> 20104 crosses the face 19968; rows 45..46 on a paddle at 40..47
    ref, s, r = _one(X=19400, Y=45 * Q + 128, VX=192, VY=0, PA=40)
    assert (s[X], s[VX], r) == (2 * 19456 - 19592, -216, 0)
    assert s[VY] == ((11648 + 256 - 44 * 256) * 72 >> 8) + _spin(ref) == 180 + _spin(ref)
    # at full speed the ball would be 2.5 px further: still a hit, the speed stays at the cap
    ref, s, _ = _one(X=18856, Y=40 * Q, VX=640, VY=30, PA=40)
    assert (s[X], s[VX]) == (2 * 19456 - 19496, -640) and s[X] == 19416
    assert s[VY] == ((40 * Q + 30 + 256 - 44 * 256) * 72 >> 8) + _spin(ref)
    # the lowest and highest overlapping rows, and one past each
    for y_row, hit in ((38, False), (39, True), (47, True), (48, False)):
        _, s, _ = _one(X=19400, Y=y_row * Q, VX=192, VY=0, PA=40)
        assert (s[VX] < 0) == hit, y_row
    # moving away from the paddle, or already past the face: no hit
    _, s, _ = _one(X=19400, Y=43 * Q, VX=-192, VY=0, PA=40)
    assert (s[X], s[VX]) == (19208, -192)
    _, s, _ = _one(X=19500, Y=43 * Q, VX=192, VY=0, PA=40)
    assert (s[X], s[VX]) == (19692, 192)


def test_opponent_paddle_hit_and_sweep():
    ref, s, r = _one(lapse=256, X=1600, Y=41 * Q, VX=-192, VY=10, PO=40)
    assert (s[X], s[VX], s[PO], r) == (2 * 1536 - 1408, 216, 40, 0)
    assert s[VY] == ((41 * Q + 10 + 256 - 44 * 256) * 72 >> 8) + _spin(ref)
    ref, s, _ = _one(lapse=256, X=2136, Y=40 * Q, VX=-640, VY=0, PO=40)
    assert (s[X], s[VX]) == (1576, 640)
    assert s[VY] == -216 + _spin(ref)
    # exactly at the face after the move is not yet past it
    _, s, _ = _one(lapse=256, X=1536 + 192, Y=40 * Q, VX=-192, VY=0, PO=40)
    assert (s[X], s[VX]) == (1536, -192)


def test_miss_on_each_side_scores_and_serves():
    # past the agent's paddle (at the top): no hit at the face, then the point at the edge
    _, s, r = _one(X=19400, Y=43 * Q, VX=192, VY=0, PA=6)
    assert (s[X], s[VX], r) == (19592, 192, 0)
    ref, s, r = _one(X=82 * Q - 100, Y=50 * Q, VX=192, VY=40, SO=3, SA=1)
    assert r == -1 and (s[SA], s[SO]) == (1, 4)
    assert (s[X], s[Y], s[VX], s[TIMER]) == (41 * Q, 43 * Q, 192, 16)      # toward the agent, who conceded
    assert s[VY] == _serve_vy(ref) and s[VY] in (-144, -72, 0, 72, 144)
    # one frame earlier the ball is not yet at the edge
    _, s, r = _one(X=82 * Q - 193, Y=50 * Q, VX=192, VY=0)
    assert r == 0 and s[X] == 82 * Q - 1
    ref, s, r = _one(lapse=256, X=-412, Y=20 * Q, VX=-192, VY=0, SA=5)
    assert r == 1 and (s[SA], s[SO]) == (6, 0)
    assert (s[X], s[Y], s[VX], s[TIMER], s[VY]) == (41 * Q, 43 * Q, -192, 16, _serve_vy(ref))
    _, s, r = _one(lapse=256, X=-319, Y=20 * Q, VX=-192, VY=0)            # -511: one sub-pixel still on the field
    assert r == 0 and s[X] == -511


def test_paddles_and_serve_timer():
    for action, dy in ((0, 0), (1, 0), (2, -2), (3, 2), (4, -2), (5, 2)):
        _, s, _ = _one(action=action, PA=30)
        assert s[PA] == 30 + dy
    assert _one(action=2, PA=7)[1][PA] == 6 and _one(action=3, PA=73)[1][PA] == 74
    # the opponent follows the approaching ball's centre row, else returns to the centre; lapse 256 never moves
    assert _one(X=40 * Q, Y=60 * Q, VX=-192, PO=40)[1][PO] == 41
    assert _one(X=40 * Q, Y=20 * Q, VX=-192, PO=40)[1][PO] == 39
    assert _one(X=40 * Q, Y=43 * Q, VX=-192, PO=40)[1][PO] == 40
    assert _one(X=40 * Q, Y=60 * Q, VX=192, PO=30)[1][PO] == 31
    assert _one(lapse=256, X=40 * Q, Y=60 * Q, VX=-192, PO=40)[1][PO] == 40
    # a resting ball: the timer counts, the paddles move, the ball does not
    _, s, r = _one(action=3, X=41 * Q, Y=43 * Q, VX=192, VY=72, TIMER=5, PA=40)
    assert (s[X], s[Y], s[TIMER], s[PA], r) == (41 * Q, 43 * Q, 4, 42, 0)


# ================================================================== episode end
def test_done_on_points_stops_the_repeat_loop():
    ref = pr.PongRef(1, seed=SEED, points=2)
    ref.state[0, [X, Y, VX, VY, SO, TIMER, T]] = [82 * Q - 300, 50 * Q, 192, 0, 1, 0, 9]
    ref.ep_return[0] = -1.0
    k0 = int(ref.k[0])
    reward, done, finished = ref.step([0])
    # frame 0: 20884 < 20992; frame 1: the point, the second of two
    assert ref.frames_run[0] == 2 and int(ref.k[0]) == k0 + 2
    assert reward[0] == -1.0 and done[0] and finished[0] == -2.0 and ref.ep_return[0] == 0.0
    s = ref.state[0]
    assert (s[SA], s[SO], s[PA], s[PO], s[T], s[TIMER]) == (0, 0, 40, 40, 0, 16)
    assert (s[X], s[Y]) == (41 * Q, 43 * Q) and abs(s[VX]) == 192 and s[VY] in (-144, -72, 0, 72, 144)
    want = np.empty((84, 84), dtype=np.uint8)
    pr.render_plane(want, 41, 43, 40, 40, 0, 0)
    planes = ref.frames.reshape(4, 84, 84)
    assert all(np.array_equal(p, want) for p in planes)
    assert ref.events["done_mid_repeat"] == 1 and ref.events["done_cap"] == 0


def test_done_at_the_step_cap():
    ref = pr.PongRef(1, seed=SEED, max_steps=3)
    for i in range(3):
        reward, done, finished = ref.step([0])
        assert reward[0] == 0 and bool(done[0]) == (i == 2) and ref.frames_run[0] == 4
        assert np.isnan(finished[0]) != (i == 2)
    assert finished[0] == 0.0 and ref.state[0, T] == 0 and ref.state[0, TIMER] == 16
    assert ref.events["done_cap"] == 1 and ref.events["done_points"] == 0


# ================================================================== render
def _counts(plane):
    return {int(v): int(n) for v, n in zip(*np.unique(plane, return_counts=True))}


def test_every_plane_shows_its_record():
    ref = pr.PongRef(2, seed=SEED, points=3)
    rng = np.random.default_rng(0)
    checked = 0
    for _ in range(120):
        ref.step(rng.integers(0, 6, 2))
        planes = ref.frames.reshape(2, 4, 84, 84)
        for e in range(2):
            for p in range(4):
                bx, by, pa, po, sa, so = (int(v) for v in ref.rec[e, p])
                if not (6 <= bx <= 76):       # the ball over a paddle column or off the edge
                    continue
                c = _counts(planes[e, p])
                lit = 4 * 84 + 4 * (sa + so) + 4
                assert c == {236: lit, 147: 16, 148: 16, 87: 84 * 84 - lit - 32}
                assert (planes[e, p, by:by + 2, bx:bx + 2] == 236).all()
                assert (planes[e, p, pa:pa + 8, 78:80] == 147).all() and (planes[e, p, po:po + 8, 4:6] == 148).all()
                checked += 1
    assert checked > 600 and ref.events["point_opp"] > 0
    # a clipped ball: one column at the left edge, none beyond it
    out = np.empty((84, 84), dtype=np.uint8)
    pr.render_plane(out, -1, 30, 40, 40, 0, 0)
    assert _counts(out)[236] == 336 + 2 and (out[30:32, 0] == 236).all()
    pr.render_plane(out, -2, 30, 40, 40, 0, 0)
    assert _counts(out)[236] == 336
    pr.render_plane(out, 83, 30, 40, 40, 0, 0)
    assert _counts(out)[236] == 336 + 2 and (out[30:32, 83] == 236).all()


def test_score_strip():
    ref = pr.PongRef(1, seed=SEED)
    plane = ref.frames.reshape(4, 84, 84)[0]
    assert (plane[0:4] == 87).all() and (plane[4:6] == 236).all() and (plane[82:84] == 236).all()
    ref.state[0, [SA, SO]] = 20
    ref.step([0])
    for plane in ref.frames.reshape(4, 84, 84):
        assert (plane[0:4, :20] == 236).all() and (plane[0:4, 64:] == 236).all() and (plane[0:4, 20:64] == 87).all()
        assert _counts(plane)[236] == 336 + 4 * 40 + 4


def test_planes_are_the_last_frames_of_the_step():
    """Plane p shows raw frame action_repeat - n_stacks + p: two stacks are the last two of four."""
    a, b = pr.PongRef(2, seed=SEED, points=2), pr.PongRef(2, seed=SEED, points=2, n_stacks=2)
    rng = np.random.default_rng(1)
    moving = 0
    for _ in range(80):
        act = rng.integers(0, 6, 2)
        a.step(act)
        b.step(act)
        pa, pb = a.frames.reshape(2, 4, -1), b.frames.reshape(2, 2, -1)
        assert np.array_equal(pa[:, 2:], pb) and np.array_equal(a.state, b.state)
        moving += int((pa[:, 0] != pa[:, 3]).any())
    assert moving > 40
    with pytest.raises(ValueError):
        pr.PongRef(1, action_repeat=2, n_stacks=4)


# ================================================================== play control
def tracker(ref, dead=2):
    """Move toward the ball's centre row (reads the state, not the pixels)."""
    s = ref.state
    d = ((s[:, Y] >> 8) + 1) - (s[:, PA] + 4)
    return np.where(d < -dead, 2, np.where(d > dead, 3, 0))


def _play(policy, n=8):
    ref = pr.PongRef(n, seed=0, render=False)
    ret, length = np.full(n, np.nan), np.zeros(n, dtype=np.int64)
    for step in range(1, 5001):
        _, done, finished = ref.step(policy(ref))
        first = done & np.isnan(ret)
        ret[first], length[first] = finished[first], step
        if not np.isnan(ret).any():
            break
    return ret, length, ref.events


def test_play_control():
    """8 games each (profiles/pong_env.txt has the figures): the no-op policy loses at least 18
    points net on average, the tracker wins on average, and every game ends on points before the
    5000-step cap."""
    ret, length, ev = _play(lambda ref: np.zeros(ref.E, dtype=np.int64))
    print("no-op", ret.tolist(), length.tolist())
    assert not np.isnan(ret).any() and ret.mean() <= -18 and length.max() < 5000 and ev["done_cap"] == 0
    ret, length, ev = _play(tracker)
    print("tracker", ret.tolist(), length.tolist())
    assert not np.isnan(ret).any() and ret.mean() > 0 and length.max() < 5000 and ev["done_cap"] == 0
    assert ev["hit_agent"] > 100 and ev["hit_opp"] > 100 and ev["point_agent"] > ev["point_opp"] > 0


# ================================================================== the classes
def test_vecpong_on_cpu_is_the_oracle():
    env = VecPong(3, "cpu", seed=5, points=2, max_steps=40, randomize_start=True)
    ref = pr.PongRef(3, seed=5, points=2, max_steps=40, randomize_start=True)
    assert env.capture_safe and env.E == 3 and env.A == 6
    assert env.frames.shape == (3, 4 * 84 * 84) and env.frames.dtype == torch.uint8
    assert len(set(ref.state[:, TIMER].tolist())) > 1, "randomize_start spreads the serve timers"
    where = env.frames.data_ptr()
    for obj in (env, ref):
        obj.reset_all()
    rng = np.random.default_rng(2)
    dones = 0
    for _ in range(150):
        act = rng.integers(0, 6, 3)
        reward, done, finished = env.step(torch.from_numpy(act))
        ref.step(act)
        assert reward.dtype == torch.float32 and done.dtype == torch.bool and finished.dtype == torch.float32
        got = dict(state=env.state.numpy(), k=env.k.numpy(), ep_return=env.ep_return.numpy(),
                   reward=reward.numpy(), done=done.numpy(), finished=finished.numpy(),
                   frames=env.frames.numpy())
        assert pr.check(got, ref.snapshot()) == 7
        assert torch.equal(torch.isnan(finished), ~done)
        dones += int(done.sum())
    assert dones > 3 and env.frames.data_ptr() == where
    # a second reset_all starts other episodes
    before = env.state.clone()
    env.reset_all()
    assert (env.state[:, [SA, SO, T]] == 0).all() and not torch.equal(env.state, before)
    assert ctypes.sizeof(PongArgs) == 8 * 8 + 8 + 9 * 4 + 4


def test_device_pong_env_has_the_pong_env_api():
    cfg = get_config("pong", **{"env.name": "pong_device", "env.pong_points": 1})
    env = make_env(cfg, seed=3)
    assert isinstance(env, DevicePongEnv) and env.ref.points == 1
    obs = env.reset()
    assert obs.shape == (4, 84, 84) and obs.dtype == np.float32
    assert set(np.unique(obs)) == {np.float32(v) / np.float32(255.0) for v in (87, 147, 148, 236)}
    assert all(0 <= env.action_space.sample() < 6 for _ in range(20)) and env.action_space.n == 6
    total, steps, done = 0.0, 0, False
    while not done:
        obs, reward, done, info = env.step(env.action_space.sample())
        assert isinstance(reward, float) and isinstance(done, bool) and info == {} and obs.shape == (4, 84, 84)
        total += reward
        steps += 1
    assert total in (-1.0, 1.0) and 4 <= steps < 400
    k = int(env.ref.k[0])
    assert np.array_equal(env.reset(), obs) and int(env.ref.k[0]) == k      # already reset in place
    env.step(0)
    env.reset()
    assert int(env.ref.k[0]) == k + 4 + 1 and env.ref.state[0, T] == 0     # a reset mid-episode


def test_env_config_defaults_and_make_device_env():
    e = EnvConfig()
    assert (e.pong_points, e.pong_max_steps, e.pong_opp_lapse) == (21, 5000, 64)
    for preset in ("pong", "atari57", "dmlab30", "reference"):
        assert get_config(preset).env.name != "pong_device"
    # every other name: the VecSyntheticAtari the drivers built before
    for preset, name in (("pong", "synthetic"), ("dmlab30", "dmlab_synth")):
        cfg = get_config(preset, **{"env.episode_len": 33, "env.switch": 5, "env.cue_only_first": True})
        assert cfg.env.name == name
        env = make_device_env(cfg, 3, "cpu", seed=11)
        assert type(env) is VecSyntheticAtari
        old = VecSyntheticAtari(3, "cpu", seed=11, episode_len=33, n_actions=cfg.model.n_actions,
                                n_stacks=cfg.env.channels_per_frame * cfg.env.n_stacks,
                                shape=(cfg.env.frame_h, cfg.env.frame_w), switch=5, cue_only_first=True)
        for field in ("E", "A", "episode_len", "switch", "cue_only_first", "C", "h", "w", "randomize_start",
                      "_seed", "fused"):
            assert getattr(env, field) == getattr(old, field), field
        assert env.randomize_start and env.frames.shape == old.frames.shape
        assert torch.equal(env.reset_all(), old.reset_all())
    assert not make_device_env(get_config("pong"), 2, "cpu", seed=1, randomize_start=False).randomize_start
    # the new name
    cfg = get_config("pong", **{"env.name": "pong_device", "env.pong_points": 5, "env.pong_max_steps": 77,
                                "env.pong_opp_lapse": 9})
    env = make_device_env(cfg, 2, "cpu", seed=1, randomize_start=False)
    assert type(env) is VecPong and (env.points, env.max_steps, env.lapse, env.C) == (5, 77, 9, 4)
    assert (env.state[:, TIMER] == 16).all()
    for bad in ({"model.n_actions": 4}, {"env.n_stacks": 5}, {"env.frame_h": 96}, {"env.channels_per_frame": 3},
                {"env.pong_points": 0}, {"env.pong_points": 43}):
        with pytest.raises(ValueError):
            make_device_env(get_config("pong", **{"env.name": "pong_device", **bad}), 2, "cpu")
    with pytest.raises(ValueError):
        VecPong(0, "cpu")


# ================================================================== the scripted run of the GPU test
RUN = dict(points=2, max_steps=100)       # the bitwise run: first to 2, at most 100 agent steps
STEPS = 600
PHASE = 150


def scripted_actions(E, steps, seed=SEED, **kw):
    """Actions (steps, E) that exercise the game: in phases of 150 steps each env plays the
    tracker, the no-op or uniformly random actions, the envs one phase apart.  Returns the actions
    and the events the oracle counted while they were played."""
    ref = pr.PongRef(E, seed=seed, render=False, **kw)
    rng = np.random.default_rng(seed)
    out = np.zeros((steps, E), dtype=np.int64)
    for s in range(steps):
        kind = (np.arange(E) + s // PHASE) % 3
        out[s] = np.where(kind == 0, tracker(ref), np.where(kind == 1, 0, rng.integers(0, 6, E)))
        ref.step(out[s])
    return out, ref.events


_CASES = {}


def scripted_case(E, steps, **kw):
    key = (E, steps, tuple(sorted(kw.items())))
    if key not in _CASES:
        _CASES[key] = scripted_actions(E, steps, **kw)
    return _CASES[key]


def compare_run(make_kernel, E, actions, seed=SEED, **kw):
    """Replay ``actions`` on the oracle and on ``make_kernel(oracle)`` -- which returns a callable
    ``step(actions) -> dict of the CHECKED arrays`` starting from the oracle's present arrays --
    and ``pr.check`` after every step.  Returns the oracle."""
    ref = pr.PongRef(E, seed=seed, **kw)
    kernel = make_kernel(ref)
    for s, act in enumerate(actions):
        ref.step(act)
        got = kernel(act)
        try:
            assert pr.check(got, ref.snapshot()) == len(pr.CHECKED)
        except AssertionError as err:
            raise AssertionError(f"step {s}: {err}") from None
    return ref


def oracle_as_kernel(rules=pr.PongRules()):
    def make(ref):
        other = pr.PongRef(ref.E, action_repeat=ref.action_repeat, n_stacks=ref.C, points=ref.points,
                           max_steps=ref.max_steps, lapse=ref.lapse, rules=rules)
        other.seed = ref.seed
        for name in ("state", "k", "ep_return", "frames"):
            getattr(other, name)[...] = getattr(ref, name)

        def step(act):
            other.step(act)
            return other.snapshot()
        return step
    return make


def test_scripted_run_covers_every_branch():
    actions, ev = scripted_case(3, STEPS, **RUN)
    print(ev)
    assert actions.shape == (600, 3) and set(np.unique(actions)) == set(range(6))
    assert ev["hit_agent"] >= 10 and ev["hit_opp"] >= 10 and ev["wall"] >= 10
    assert ev["point_agent"] >= 3 and ev["point_opp"] >= 3
    assert ev["done_mid_repeat"] >= 2 and ev["done_points"] > ev["done_mid_repeat"] and ev["done_cap"] >= 1


def test_comparison_accepts_the_oracle_and_rejects_wrong_games():
    actions, _ = scripted_case(3, STEPS, **RUN)
    ref = compare_run(oracle_as_kernel(), 3, actions, **RUN)
    assert ref.events == scripted_case(3, STEPS, **RUN)[1]
    # the top wall one row lower
    with pytest.raises(AssertionError, match=r"step \d+: (state|frames)"):
        compare_run(oracle_as_kernel(replace(pr.PongRules(), y_min=7 * Q)), 3, actions, **RUN)
    # the spin drawn with the serve's salt and the serve with the spin's
    with pytest.raises(AssertionError, match=r"step \d+: state"):
        compare_run(oracle_as_kernel(replace(pr.PongRules(), salt_spin=3, salt_serve=2)), 3, actions, **RUN)
    # one byte of one plane
    def one_byte(ref_):
        step = oracle_as_kernel()(ref_)

        def bad(act):
            got = step(act)
            got["frames"][2, 3 * 7056 + 83] ^= 1      # env 2, plane 3, row 0, column 83
            return got
        return bad
    with pytest.raises(AssertionError, match=r"step 0: frames: element 77699 "):
        compare_run(one_byte, 3, actions[:1], **RUN)
