"""The Breakout-like game's oracle (pytorch_r2d2_amd/breakout_ref.py) under its own control, on the
CPU: scripted single frames against hand-computed integers, the three ways an episode ends, the
render, the flicker, a play control (no-op scores nothing, a ball tracker scores well, every game
ends on lives), the env classes and ``make_device_env``.  It also holds the scripted runs that
tests/test_breakout_gpu.py replays on the kernel, with the proof that together they cover every
event and that the comparison rejects wrong games (the brick band one row off, the spin drawn with
the serve's salt, one flipped frame byte)."""
import ctypes
from dataclasses import replace

import numpy as np
import pytest
import torch

from pytorch_r2d2_amd import breakout_ref as br
from pytorch_r2d2_amd.breakout_ref import B0, LIVES, PX, T, TIMER, VX, VY, X, Y
from pytorch_r2d2_amd.config import EnvConfig, get_config
from pytorch_r2d2_amd.envs import (DeviceBreakoutEnv, VecBreakout, VecPong, VecSyntheticAtari,
                                   make_device_env, make_env)
from pytorch_r2d2_amd.envs.breakout_device import BreakoutArgs

Q = 256
SEED = 7
FULL = 0x7FFFF
COLS = dict(X=X, Y=Y, VX=VX, VY=VY, PX=PX, LIVES=LIVES, TIMER=TIMER, T=T)


# ================================================================== scripted single frames
def _one(action=0, bricks=None, **cols):
    """One env with the given state columns (ball in play unless TIMER is given) and brick words
    (a dict row -> word over the full wall), one raw frame."""
    ref = br.BreakoutRef(1, seed=SEED)
    ref.state[0, TIMER] = 0
    for name, v in cols.items():
        ref.state[0, COLS[name]] = v
    for r, word in (bricks or {}).items():
        ref.state[0, B0 + r] = word
    k0 = int(ref.k[0])
    r = ref._frame(np.array([action]), np.array([True]))
    assert int(ref.k[0]) == k0 + 1
    return ref, ref.state[0].tolist(), int(r[0])


def _spin(ref):
    h = int(br.env_hash(ref.seed, ref.k, np.uint64(2 << 32))[0])
    return (h % 3 - 1) * 32


def _serve_vx(ref):
    h = int(br.env_hash(ref.seed, ref.k, np.uint64(3 << 32))[0])
    return (-144, -72, 72, 144)[h % 4]


def _bricks_left(s):
    return sum(bin(w).count("1") for w in s[B0:])


def test_state_layout_and_the_reset():
    assert (X, Y, VX, VY, PX, LIVES, TIMER, T, B0) == tuple(range(9)) and br.NS == 14
    ref = br.BreakoutRef(2, seed=SEED)
    for s in ref.state.tolist():
        assert s[:2] == [41 * Q, 40 * Q] and s[VX] in (-144, -72, 72, 144) and s[VY] == 160
        assert s[PX:] == [36, 5, 16, 0] + [FULL] * 6
    assert ref.state.dtype == np.int32 and ref.k.tolist() == [1, 1] and ref.k.dtype == np.int64
    lumas = {br.BG, br.WALL, br.LIFE, br.PADDLE, br.BALL, *br.ROW_LUMA}
    assert len(lumas) == 11 and 0 not in lumas and all(0 < v < 256 for v in lumas)


def test_side_walls_and_top_wall():
    _, s, r = _one(X=4 * Q + 50, Y=50 * Q, VX=-120, VY=100)
    assert (s[X], s[Y], s[VX], s[VY], r) == (1094, 12900, 120, 100, 0)       # 954 -> 2*1024 - 954
    _, s, r = _one(X=78 * Q - 10, Y=50 * Q, VX=100, VY=100)
    assert (s[X], s[VX], r) == (19878, -100, 0)                              # 20058 -> 2*19968 - 20058
    # exactly on a wall: no reflection
    _, s, _ = _one(X=4 * Q + 120, Y=50 * Q, VX=-120, VY=100)
    assert (s[X], s[VX]) == (1024, -120)
    _, s, _ = _one(X=78 * Q - 100, Y=50 * Q, VX=100, VY=100)
    assert (s[X], s[VX]) == (19968, 100)
    ref, s, r = _one(X=30 * Q, Y=6 * Q + 50, VX=72, VY=-120)
    assert (s[X], s[Y], s[VX], s[VY], r) == (7752, 1606, 72, 120, 0)         # 1466 -> 2*1536 - 1466
    assert ref.events["top"] == 1 and ref.events["side"] == 0
    _, s, _ = _one(X=30 * Q, Y=6 * Q + 120, VX=72, VY=-120)
    assert (s[Y], s[VY]) == (1536, -120)


def test_brick_hit_from_below_and_from_above():
    # from below: 7268 - 160 = 7108, row 27 = the lower row of brick row 5; column 20 is brick 4
    ref, s, r = _one(X=20 * Q, Y=28 * Q + 100, VX=0, VY=-160)
    assert (s[X], s[Y], s[VY], r) == (5120, 7108, 160, 1)
    assert s[B0 + 5] == FULL & ~(1 << 4) and s[B0:B0 + 5] == [FULL] * 5
    assert ref.events["brick"] == 1 and ref.events["brick_upper"] == 0
    # one row lower the ball is not yet in the band
    _, s, r = _one(X=20 * Q, Y=29 * Q + 100, VX=0, VY=-160)
    assert (s[Y], s[VY], r, _bricks_left(s)) == (7364, -160, 0, 114)
    # the second column is tested when the first is empty: columns 19 (brick 3, gone) and 20 (brick 4)
    _, s, r = _one(X=19 * Q, Y=28 * Q + 100, VX=0, VY=-160, bricks={5: FULL & ~(1 << 3)})
    assert (s[VY], r, s[B0 + 5]) == (160, 1, FULL & ~(1 << 3) & ~(1 << 4))
    # ... and the first wins when both stand
    _, s, r = _one(X=19 * Q, Y=28 * Q + 100, VX=0, VY=-160)
    assert (r, s[B0 + 5]) == (1, FULL & ~(1 << 3))
    # both empty: no hit
    _, s, r = _one(X=19 * Q, Y=28 * Q + 100, VX=0, VY=-160, bricks={5: FULL & ~(3 << 3)})
    assert (s[VY], r, _bricks_left(s)) == (-160, 0, 112)
    # from above: 3784 + 160 = 3944, pixel row 15, the leading row 16 is brick row 0; column 40 is brick 9
    ref, s, r = _one(X=40 * Q, Y=14 * Q + 200, VX=0, VY=160)
    assert (s[Y], r, s[B0]) == (3944, 7, FULL & ~(1 << 9))
    assert s[VY] == -320 and ref.events["brick_upper"] == 1                   # the speed-up, upward
    # one row higher: the leading row 15 is above the band
    _, s, r = _one(X=40 * Q, Y=13 * Q + 200, VX=0, VY=160)
    assert (s[VY], r) == (160, 0)
    # the last column: pixel columns 78 / 79 are brick 18
    _, s, r = _one(X=78 * Q, Y=28 * Q + 100, VX=0, VY=-160)
    assert (r, s[B0 + 5]) == (1, FULL & ~(1 << 18))


def test_reward_and_speed_up_of_each_row():
    for row, value in enumerate((7, 7, 4, 4, 1, 1)):
        y = (17 + 2 * row) * Q + 100 + 160          # lands in the row's lower pixel row
        ref, s, r = _one(X=30 * Q, Y=y, VX=0, VY=-160)
        assert r == value and s[B0 + row] == FULL & ~(1 << 6), row
        assert s[VY] == (320 if row < 4 else 160), row
        assert _bricks_left(s) == 113, "at most one brick per raw frame"
        assert ref.events["brick_upper"] == (row < 4)
    # a ball that is already faster keeps its speed
    ref, s, r = _one(X=30 * Q, Y=17 * Q + 100 + 400, VX=0, VY=-400)
    assert (r, s[VY], ref.events["brick_upper"]) == (7, 400, 0)
    # the fastest ball (448 = 1.75 px) still takes one brick, of the leading row only
    _, s, r = _one(X=30 * Q, Y=27 * Q + 448, VX=0, VY=-448, bricks={5: 0})
    assert (s[Y] >> 8, r, _bricks_left(s)) == (27, 0, 95)
    _, s, r = _one(X=30 * Q, Y=25 * Q + 448, VX=0, VY=-448)      # from pixel row 26 (brick row 5) into 25
    assert (s[Y] >> 8, r, s[B0 + 4], s[B0 + 5]) == (25, 1, FULL & ~(1 << 6), FULL)


def test_paddle_sweep():
    # bottom edge 19912 -> 20072 crosses the face 19968; columns 41..42 on a paddle at 36..47
    ref, s, r = _one(X=41 * Q, Y=75 * Q + 200, VX=10, VY=160, PX=36)
    assert (s[Y], s[VY], r) == (2 * 19456 - 19560, -168, 0) and s[Y] == 19352
    assert s[VX] == ((10506 + 256 - 42 * 256) * 40 >> 8) + _spin(ref) == 1 + _spin(ref)
    assert ref.events["paddle"] == 1
    ref, s, _ = _one(X=44 * Q + 128, Y=75 * Q + 200, VX=0, VY=160, PX=36)
    assert s[VX] == 140 + _spin(ref)
    # the lowest and highest overlapping column, and one past each
    for col, hit in ((34, False), (35, True), (47, True), (48, False)):
        ref, s, _ = _one(X=col * Q, Y=75 * Q + 200, VX=0, VY=160, PX=36)
        assert (s[VY] < 0) == hit, col
        if hit:
            assert s[VX] == ((col - 41) * 40) + _spin(ref)
        else:
            assert (s[Y], s[VX]) == (19560, 0)
    # at the speed cap
    ref, s, _ = _one(X=41 * Q, Y=75 * Q + 200, VX=0, VY=445, PX=36)
    assert (s[Y], s[VY]) == (2 * 19456 - 19845, -448)
    # moving up, or the edge already past the face: no hit
    _, s, _ = _one(X=41 * Q, Y=75 * Q + 200, VX=0, VY=-160, PX=36)
    assert (s[Y], s[VY]) == (19240, -160)
    _, s, _ = _one(X=41 * Q, Y=75 * Q + 300, VX=0, VY=160, PX=36)
    assert (s[Y], s[VY]) == (19660, 160)
    # the edge exactly on the face after the move is not yet past it
    _, s, _ = _one(X=41 * Q, Y=76 * Q - 160, VX=0, VY=160, PX=36)
    assert (s[Y], s[VY]) == (19456, 160)
    # the paddle moves before the test: from 33 it reaches column 36 and meets the ball at 47
    _, s, _ = _one(action=2, X=47 * Q, Y=75 * Q + 200, VX=0, VY=160, PX=33)
    assert s[PX] == 36 and s[VY] == -168


def test_miss_costs_a_life_and_serves():
    ref, s, r = _one(X=20 * Q, Y=84 * Q - 100, VX=50, VY=160, LIVES=3)
    assert r == 0 and s[LIVES] == 2 and ref.events["lost"] == 1
    assert (s[X], s[Y], s[VY], s[TIMER]) == (41 * Q, 40 * Q, 160, 16)
    assert s[VX] == _serve_vx(ref) and s[VX] in (-144, -72, 72, 144)
    # one sub-pixel short of the edge: still in play
    _, s, _ = _one(X=20 * Q, Y=84 * Q - 161, VX=50, VY=160, LIVES=3)
    assert (s[Y], s[LIVES], s[TIMER]) == (84 * Q - 1, 3, 0)
    # beside the paddle at the face: no hit
    _, s, _ = _one(X=20 * Q, Y=75 * Q + 200, VX=0, VY=160, PX=36)
    assert (s[Y], s[VY]) == (19560, 160)


def test_paddle_actions_and_serve_timer():
    for action, dx in ((0, 0), (1, 0), (2, 3), (3, -3), (4, 3), (5, -3)):
        _, s, _ = _one(action=action, PX=30)
        assert s[PX] == 30 + dx
    assert _one(action=3, PX=5)[1][PX] == 4 and _one(action=2, PX=67)[1][PX] == 68
    # a resting ball: the timer counts, the paddle moves, the ball does not
    _, s, r = _one(action=2, X=41 * Q, Y=40 * Q, VX=72, VY=160, TIMER=5, PX=36)
    assert (s[X], s[Y], s[TIMER], s[PX], r) == (41 * Q, 40 * Q, 4, 39, 0)
    _, s, _ = _one(X=41 * Q, Y=40 * Q, VX=72, VY=160, TIMER=1)
    assert (s[X], s[Y], s[TIMER]) == (41 * Q, 40 * Q, 0)
    _, s, _ = _one(X=41 * Q, Y=40 * Q, VX=72, VY=160, TIMER=0)
    assert (s[X], s[Y]) == (41 * Q + 72, 40 * Q + 160)


# ================================================================== episode end
def _reset_plane(lives=5):
    want = np.empty((84, 84), dtype=np.uint8)
    br.render_plane(want, 41, 40, 36, lives, [FULL] * 6)
    return want


def test_last_life_lost_stops_the_repeat_loop():
    ref = br.BreakoutRef(1, seed=SEED)
    ref.state[0, [X, Y, VX, VY, LIVES, TIMER, T]] = [20 * Q, 84 * Q - 200, 0, 160, 1, 0, 9]
    ref.state[0, B0 + 5] = FULL & ~7
    ref.ep_return[0] = 3.0
    k0 = int(ref.k[0])
    reward, done, finished = ref.step([0])
    # frame 0: 21464 < 21504; frame 1: the last life
    assert ref.frames_run[0] == 2 and int(ref.k[0]) == k0 + 2
    assert reward[0] == 0.0 and done[0] and finished[0] == 3.0 and ref.ep_return[0] == 0.0
    s = ref.state[0].tolist()
    assert s[:2] == [41 * Q, 40 * Q] and s[VX] in (-144, -72, 72, 144) and s[VY:] == [160, 36, 5, 16, 0] + [FULL] * 6
    assert all(np.array_equal(p, _reset_plane()) for p in ref.frames.reshape(4, 84, 84))
    ev = ref.events
    assert (ev["done_lives"], ev["done_mid_repeat"], ev["done_clear"], ev["done_cap"]) == (1, 1, 0, 0)


def test_wall_cleared():
    ref = br.BreakoutRef(1, seed=SEED, lives=3)
    ref.state[0, [X, Y, VX, VY, TIMER, LIVES]] = [20 * Q, 28 * Q + 100, 0, -160, 0, 2]
    ref.state[0, B0:] = [0, 0, 0, 0, 0, 1 << 4]
    reward, done, finished = ref.step([0])
    assert ref.frames_run[0] == 1 and reward[0] == 1.0 and done[0] and finished[0] == 1.0
    assert ref.state[0, B0:].tolist() == [FULL] * 6 and ref.state[0, LIVES] == 3 and ref.state[0, T] == 0
    assert all(np.array_equal(p, _reset_plane(3)) for p in ref.frames.reshape(4, 84, 84))
    ev = ref.events
    assert (ev["done_clear"], ev["done_mid_repeat"], ev["done_lives"], ev["done_cap"]) == (1, 1, 0, 0)


def test_done_at_the_step_cap():
    ref = br.BreakoutRef(1, seed=SEED, max_steps=3)
    for i in range(3):
        reward, done, finished = ref.step([0])
        assert reward[0] == 0 and bool(done[0]) == (i == 2) and ref.frames_run[0] == 4
        assert np.isnan(finished[0]) != (i == 2)
    assert finished[0] == 0.0 and ref.state[0, T] == 0 and ref.state[0, TIMER] == 16
    assert ref.events["done_cap"] == 1 and ref.events["done_lives"] == 0 and ref.events["done_clear"] == 0


# ================================================================== render
def _counts(plane):
    return {int(v): int(n) for v, n in zip(*np.unique(plane, return_counts=True))}


def tracker(ref, dead=2):
    """Move toward the ball's centre column (reads the state, not the pixels)."""
    s = ref.state
    d = ((s[:, X] >> 8) + 1) - (s[:, PX] + 6)
    return np.where(d > dead, 2, np.where(d < -dead, 3, 0))


def test_every_plane_shows_its_record():
    ref = br.BreakoutRef(2, seed=SEED, lives=3)
    rng = np.random.default_rng(0)
    checked, fewer = 0, 0
    for _ in range(300):
        ref.step(np.array([tracker(ref)[0], rng.integers(0, 6)]))        # env 0 tracks, env 1 plays at random
        planes = ref.frames.reshape(2, 4, 84, 84)
        for e in range(2):
            for p in range(4):
                bx, by, px, lives = (int(v) for v in ref.rec[e, p, :4])
                words = [int(w) for w in ref.rec[e, p, 4:]]
                plane = planes[e, p]
                assert (plane[by:by + 2, bx:bx + 2] == 236).all()
                assert (plane[0:4, :4 * lives] == 200).all() and (plane[0:4, 4 * lives:] == 24).all()
                if 14 <= by <= 27 or 76 <= by <= 79:      # the ball over the brick band or the paddle's rows
                    continue
                want = {236: 4 if by < 83 else 2, 200: 16 * lives, 142: 2 * 84 + 78 * 8, 110: 24}
                for r, w in enumerate(words):
                    if w:
                        want[br.ROW_LUMA[r]] = 8 * bin(w).count("1")
                want[24] = 84 * 84 - sum(want.values())
                assert _counts(plane) == want
                assert (plane[78:80, px:px + 12] == 110).all()
                checked += 1
                fewer += sum(words) != 6 * FULL
    assert checked > 1200 and fewer > 300 and ref.events["lost"] > 0 and ref.events["brick"] > 5
    # a removed brick is background, its neighbours keep their row's luma
    out = np.empty((84, 84), dtype=np.uint8)
    br.render_plane(out, 41, 40, 36, 5, [FULL, FULL & ~(1 << 7), FULL, FULL, FULL, FULL & ~1])
    assert (out[18:20, 32:36] == 24).all() and (out[18:20, 28:32] == 119).all() and (out[18:20, 36:40] == 119).all()
    assert (out[16:18, 32:36] == 98).all() and (out[20:22, 32:36] == 133).all()
    assert (out[26:28, 4:8] == 24).all() and (out[26:28, 8:12] == 90).all() and (out[26:28, 76:80] == 90).all()
    assert (out[28, 4:80] == 24).all() and (out[15, 4:80] == 24).all()
    # walls and the strip
    assert (out[4:6] == 142).all() and (out[4:, :4] == 142).all() and (out[4:, 80:] == 142).all()
    assert (out[0:4, :20] == 200).all() and (out[0:4, 20:] == 24).all() and (out[6:, 4:80] != 142).all()
    br.render_plane(out, 41, 40, 36, 2, [FULL] * 6)
    assert (out[0:4, :8] == 200).all() and (out[0:4, 8:] == 24).all()
    br.render_plane(out, 41, 40, 36, 0, [0] * 6)
    assert _counts(out) == {236: 4, 142: 792, 110: 24, 24: 7056 - 820}
    # the ball clipped at the bottom edge: one row left
    br.render_plane(out, 40, 83, 36, 5, [FULL] * 6)
    assert _counts(out)[236] == 2 and (out[83, 40:42] == 236).all()
    br.render_plane(out, 40, 82, 36, 5, [FULL] * 6)
    assert _counts(out)[236] == 4
    # the ball is drawn last: over a brick and over the paddle
    br.render_plane(out, 40, 79, 36, 5, [FULL] * 6)
    assert _counts(out)[110] == 22 and _counts(out)[236] == 4
    br.render_plane(out, 41, 17, 36, 5, [FULL] * 6)
    assert (out[17:19, 41:43] == 236).all() and _counts(out)[98] == 8 * 19 - 2


def test_planes_are_the_last_frames_of_the_step():
    """Plane p shows raw frame action_repeat - n_stacks + p: two stacks are the last two of four."""
    a, b = br.BreakoutRef(2, seed=SEED, lives=2), br.BreakoutRef(2, seed=SEED, lives=2, n_stacks=2)
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
        br.BreakoutRef(1, action_repeat=2, n_stacks=4)


# ================================================================== flicker
def _flicker_pair(flicker, steps, E=4, **kw):
    """The same actions on a game with flicker and on one without; yields both after every step."""
    a, b = br.BreakoutRef(E, seed=SEED, flicker=flicker, **kw), br.BreakoutRef(E, seed=SEED, **kw)
    assert np.array_equal(a.frames, b.frames), "planes written by reset_all are never blank"
    rng = np.random.default_rng(2)
    for _ in range(steps):
        act = rng.integers(0, 6, E)
        a.step(act)
        b.step(act)
        for name in ("state", "k", "ep_return", "reward", "done"):
            assert np.array_equal(getattr(a, name), getattr(b, name)), name
        assert np.array_equal(a.finished, b.finished, equal_nan=True)
        yield a, b


def test_flicker_blanks_about_half_the_planes_and_touches_no_state():
    blank = total = 0
    for a, b in _flicker_pair(128, 60, lives=2, max_steps=50):
        pa, pb = a.frames.reshape(4, 4, -1), b.frames.reshape(4, 4, -1)
        for e in range(4):
            for p in range(4):
                if a.blank[e, p]:
                    assert not pa[e, p].any(), "a blank plane is all zeros"
                else:
                    assert np.array_equal(pa[e, p], pb[e, p]) and pa[e, p].all()
            if a.done[e]:
                assert not a.blank[e].any(), "planes written by a reset are never blank"
            else:
                blank += int(a.blank[e].sum())
                total += 4
    assert total > 800 and 0.4 <= blank / total <= 0.6, (blank, total)
    assert a.events == b.events and a.events["done_lives"] + a.events["done_cap"] >= 4


def test_flicker_256_blanks_every_plane_but_a_reset_s():
    resets = 0
    for a, b in _flicker_pair(256, 50, E=2, lives=1, max_steps=40):
        pa, pb = a.frames.reshape(2, 4, -1), b.frames.reshape(2, 4, -1)
        for e in range(2):
            if a.done[e]:
                assert np.array_equal(pa[e], pb[e]) and pa[e].all()
                resets += 1
            else:
                assert not pa[e].any() and pb[e].all()
    assert resets >= 2
    for a, b in _flicker_pair(0, 5):
        assert np.array_equal(a.frames, b.frames) and not a.blank.any()


def test_flicker_draw_is_the_frame_s_own():
    """Plane p's draw: the flicker's salt (6) at the counter of raw frame action_repeat - n_stacks + p."""
    ref = br.BreakoutRef(3, seed=SEED, flicker=100, n_stacks=2)
    k0 = ref.k.copy()
    ref.step([0, 0, 0])
    for e in range(3):
        for p in range(2):
            h = int(br.env_hash(ref.seed, [int(k0[e]) + 1 + 2 + p], [(6 << 32) + e])[0])
            assert bool(ref.blank[e, p]) == ((h & 255) < 100)
    assert (ref.k == k0 + 4).all()


# ================================================================== play control
def _play(policy, n=8):
    ref = br.BreakoutRef(n, seed=0, render=False)
    ret, length = np.full(n, np.nan), np.zeros(n, dtype=np.int64)
    for step in range(1, 5001):
        _, done, finished = ref.step(policy(ref))
        first = done & np.isnan(ret)
        ret[first], length[first] = finished[first], step
        if not np.isnan(ret).any():
            break
    return ret, length, ref.events


def test_play_control():
    """8 games each (profiles/breakout_env.txt has the figures): the no-op policy scores at most 1
    on average, the tracker at least 50 and more than uniformly random play, and every game ends
    before the 5000-step cap."""
    rng = np.random.default_rng(0)
    ret, length, ev = _play(lambda ref: np.zeros(ref.E, dtype=np.int64))
    print("no-op", ret.tolist(), length.tolist())
    assert not np.isnan(ret).any() and ret.mean() <= 1 and length.max() < 5000 and ev["done_cap"] == 0
    rand, length, ev = _play(lambda ref: rng.integers(0, 6, ref.E))
    print("random", rand.tolist(), length.tolist())
    assert not np.isnan(rand).any() and length.max() < 5000 and ev["done_cap"] == 0
    ret, length, ev = _play(tracker)
    print("tracker", ret.tolist(), length.tolist(), ev)
    assert not np.isnan(ret).any() and ret.mean() >= 50 and ret.mean() > rand.mean()
    assert length.max() < 5000 and ev["done_cap"] == 0 and ev["done_lives"] >= 8
    assert ev["paddle"] > 100 and ev["brick"] > 100 and ev["brick_upper"] > 0 and ev["top"] > 0


# ================================================================== the classes
def test_vecbreakout_on_cpu_is_the_oracle():
    kw = dict(lives=1, max_steps=40, flicker=64)
    env = VecBreakout(3, "cpu", seed=5, randomize_start=True, **kw)
    ref = br.BreakoutRef(3, seed=5, randomize_start=True, **kw)
    assert env.capture_safe and env.E == 3 and env.A == 6 and env.max_episode_len == 40
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
        assert br.check(got, ref.snapshot()) == 7
        assert torch.equal(torch.isnan(finished), ~done)
        dones += int(done.sum())
    assert dones > 3 and env.frames.data_ptr() == where
    # a second reset_all starts other episodes
    before = env.k.clone()
    env.reset_all()
    assert (env.state[:, T] == 0).all() and (env.state[:, LIVES] == 1).all() and torch.equal(env.k, before + 1)
    assert ctypes.sizeof(BreakoutArgs) == 8 * 8 + 8 + 9 * 4 + 4


def test_device_breakout_env_has_the_pong_env_api():
    cfg = get_config("pong", **{"env.name": "breakout_device", "env.breakout_lives": 1, "env.breakout_flicker": 0})
    env = make_env(cfg, seed=3)
    assert isinstance(env, DeviceBreakoutEnv) and env.ref.lives == 1 and env.ref.max_steps == 5000
    obs = env.reset()
    assert obs.shape == (4, 84, 84) and obs.dtype == np.float32
    lumas = (24, 142, 200, 110, 236, 98, 119, 133, 151, 129, 90)
    assert set(np.unique(obs)) == {np.float32(v) / np.float32(255.0) for v in lumas}
    assert all(0 <= env.action_space.sample() < 6 for _ in range(20)) and env.action_space.n == 6
    total, steps, done = 0.0, 0, False
    while not done:
        obs, reward, done, info = env.step(env.action_space.sample())
        assert isinstance(reward, float) and isinstance(done, bool) and info == {} and obs.shape == (4, 84, 84)
        total += reward
        steps += 1
    assert total >= 0.0 and 20 <= steps < 2000
    k = int(env.ref.k[0])
    assert np.array_equal(env.reset(), obs) and int(env.ref.k[0]) == k      # already reset in place
    env.step(0)
    env.reset()
    assert int(env.ref.k[0]) == k + 4 + 1 and env.ref.state[0, T] == 0     # a reset mid-episode
    with pytest.raises(ValueError):
        make_env(get_config("pong", **{"env.name": "breakout_device", "env.channels_per_frame": 3}))


def test_env_config_defaults_and_make_device_env():
    e = EnvConfig()
    assert (e.breakout_lives, e.breakout_max_steps, e.breakout_flicker) == (5, 5000, 0)
    for preset in ("reference", "cartpole", "pong", "atari57", "seaquest8", "dmlab30"):
        assert get_config(preset).env.name != "breakout_device"
    # every other name builds what it built before
    assert type(make_device_env(get_config("pong"), 2, "cpu", seed=1)) is VecSyntheticAtari
    assert type(make_device_env(get_config("pong", **{"env.name": "pong_device"}), 2, "cpu", seed=1)) is VecPong
    # the new name
    cfg = get_config("pong", **{"env.name": "breakout_device", "env.breakout_lives": 3, "env.breakout_max_steps": 77,
                                "env.breakout_flicker": 9})
    env = make_device_env(cfg, 2, "cpu", seed=1, randomize_start=False)
    assert type(env) is VecBreakout and (env.lives, env.max_steps, env.flicker, env.C) == (3, 77, 9, 4)
    assert (env.state[:, TIMER] == 16).all() and (env.state[:, LIVES] == 3).all() and not env.fused
    assert make_device_env(cfg, 2, "cpu", seed=1).randomize_start
    for bad in ({"model.n_actions": 4}, {"env.n_stacks": 5}, {"env.n_stacks": 9, "env.action_repeat": 9},
                {"env.action_repeat": 65}, {"env.frame_h": 96}, {"env.frame_w": 96}, {"env.channels_per_frame": 3},
                {"env.breakout_lives": 0}, {"env.breakout_lives": 6}, {"env.breakout_max_steps": 0},
                {"env.breakout_flicker": -1}, {"env.breakout_flicker": 257}):
        with pytest.raises(ValueError):
            make_device_env(get_config("pong", **{"env.name": "breakout_device", **bad}), 2, "cpu")
    with pytest.raises(ValueError):
        VecBreakout(0, "cpu")
    VecBreakout(1, "cpu", flicker=256, lives=5, n_stacks=8, action_repeat=64)


# ================================================================== the scripted runs of the GPU test
RUN = dict(lives=2, max_steps=100)        # the main bitwise run: two lives, at most 100 agent steps
STEPS = 600
PHASE = 150
CHANNEL = FULL & ~(0x1F << 7)             # every row without its brick columns 7..11
EVENTS = ("brick", "brick_upper", "paddle", "side", "top", "lost", "done_lives", "done_clear", "done_cap",
          "done_mid_repeat")


def first_bricks(E, n=3, seed=SEED, **kw):
    """The first ``n`` bricks the tracker removes from a full wall in each env: (E, 6) words."""
    ref = br.BreakoutRef(E, seed=seed, render=False, **kw)
    keep, left = np.zeros((E, br.ROWS), dtype=np.int32), np.full(E, n)
    for _ in range(400):
        before = ref.state[:, B0:].copy()
        _, done, _ = ref.step(tracker(ref))
        assert not (done & (left > 0)).any(), "an episode ended before the tracker had its bricks"
        gone = before & ~ref.state[:, B0:]
        for e, r in zip(*np.nonzero(gone)):
            if left[e] > 0:           # one brick per raw frame and row word: a single bit, or a few
                for j in range(br.COLS):
                    if gone[e, r] >> j & 1 and left[e] > 0:
                        keep[e, r] |= 1 << j
                        left[e] -= 1
        if not left.any():
            return keep
    raise AssertionError("the tracker did not reach its bricks")


def edit_clear(ref):
    """A wall of the three bricks the tracker hits first: it is cleared within ~110 steps."""
    ref.state[:, B0:] = first_bricks(ref.E, 3, action_repeat=ref.action_repeat, n_stacks=ref.C,
                                     lives=ref.lives, max_steps=ref.max_steps)


def edit_channel(ref):
    """A five-column channel through the wall: the ball reaches the top wall and the upper rows."""
    ref.state[:, B0:] = CHANNEL


def seven_start(state):
    """(E, 14) state words -> ball in play under a wall of its two upper rows, moving up at 320:
    whatever the actions, it takes a brick worth 7 within 8 agent steps."""
    state[:, [X, Y, VX, VY, TIMER]] = np.asarray([41 * Q, 30 * Q, 72, -320, 0], dtype=state.dtype)
    state[:, B0 + 2:] = 0


EDITS = {None: lambda ref: None, "clear": edit_clear, "channel": edit_channel,
         "seven": lambda ref: seven_start(ref.state)}


def scripted_actions(E, steps, seed=SEED, edit=None, policy="phases", **kw):
    """Actions (steps, E) that exercise the game.  ``phases``: in phases of 150 steps each env
    plays the tracker, the no-op or uniformly random actions, the envs one phase apart;
    ``tracker``: every env tracks.  ``edit`` names the change made to the start state.  Returns
    the actions and the events the oracle counted while they were played."""
    ref = br.BreakoutRef(E, seed=seed, render=False, **kw)
    EDITS[edit](ref)
    rng = np.random.default_rng(seed)
    out = np.zeros((steps, E), dtype=np.int64)
    for s in range(steps):
        kind = (np.arange(E) + s // PHASE) % 3 if policy == "phases" else np.zeros(E, dtype=np.int64)
        out[s] = np.where(kind == 0, tracker(ref), np.where(kind == 1, 0, rng.integers(0, 6, E)))
        ref.step(out[s])
    return out, ref.events


_CASES = {}


def scripted_case(E, steps, edit=None, policy="phases", **kw):
    key = (E, steps, edit, policy, tuple(sorted(kw.items())))
    if key not in _CASES:
        _CASES[key] = scripted_actions(E, steps, edit=edit, policy=policy, **kw)
    return _CASES[key]


# the edited-start runs of the GPU test: (E, steps, edit, keywords)
CLEAR_RUN = (3, 112, "clear", {})
CHANNEL_RUN = (2, 300, "channel", {})


def compare_run(make_kernel, E, actions, seed=SEED, edit=None, **kw):
    """Replay ``actions`` on the oracle (its start state changed by ``edit``) and on
    ``make_kernel(oracle)`` -- which returns a callable ``step(actions) -> dict of the CHECKED
    arrays`` starting from the oracle's present arrays -- and ``br.check`` after every step.
    Returns the oracle."""
    ref = br.BreakoutRef(E, seed=seed, **kw)
    EDITS[edit](ref)
    kernel = make_kernel(ref)
    for s, act in enumerate(actions):
        ref.step(act)
        got = kernel(act)
        try:
            assert br.check(got, ref.snapshot()) == len(br.CHECKED)
        except AssertionError as err:
            raise AssertionError(f"step {s}: {err}") from None
    return ref


def oracle_as_kernel(rules=br.BreakoutRules()):
    def make(ref):
        other = br.BreakoutRef(ref.E, action_repeat=ref.action_repeat, n_stacks=ref.C, lives=ref.lives,
                               max_steps=ref.max_steps, flicker=ref.flicker, rules=rules)
        other.seed = ref.seed
        for name in ("state", "k", "ep_return", "frames"):
            getattr(other, name)[...] = getattr(ref, name)

        def step(act):
            other.step(act)
            return other.snapshot()
        return step
    return make


def test_scripted_runs_cover_every_event():
    actions, ev = scripted_case(3, STEPS, **RUN)
    print("main", ev)
    assert actions.shape == (600, 3) and set(np.unique(actions)) == set(range(6))
    assert ev["brick"] >= 10 and ev["paddle"] >= 10 and ev["side"] >= 10 and ev["lost"] >= 20
    assert ev["done_lives"] >= 10 and ev["done_mid_repeat"] >= 10 and ev["done_cap"] >= 3
    E, steps, edit, kw = CLEAR_RUN
    _, clear = scripted_case(E, steps, edit=edit, policy="tracker", **kw)
    print("clear", clear)
    assert clear["done_clear"] == E and clear["brick"] >= 3 * E and clear["done_mid_repeat"] >= 1
    E, steps, edit, kw = CHANNEL_RUN
    _, chan = scripted_case(E, steps, edit=edit, policy="tracker", **kw)
    print("channel", chan)
    assert chan["top"] >= 5 and chan["brick_upper"] >= 1 and chan["brick"] >= 20
    assert all(ev[n] + clear[n] + chan[n] >= 1 for n in EVENTS) and set(ev) == set(EVENTS)


def test_seven_start_scores_seven_whatever_the_actions():
    """The start of the actor test (tests/test_vec_breakout_gpu.py): with one life and a cap of 30 every
    env finishes an episode worth at least 7 within 40 steps, under no-op, tracker and random play."""
    rng = np.random.default_rng(3)
    for policy in (lambda ref: np.zeros(4, dtype=np.int64), tracker, lambda ref: rng.integers(0, 6, 4)):
        ref = br.BreakoutRef(4, seed=3, lives=1, max_steps=30, render=False)
        seven_start(ref.state)
        first = np.full(4, np.nan)
        for _ in range(40):
            _, done, finished = ref.step(policy(ref))
            new = done & np.isnan(first)
            first[new] = finished[new]
        assert (first >= 7).all(), first


def test_comparison_accepts_the_oracle_and_rejects_wrong_games():
    actions, _ = scripted_case(3, STEPS, **RUN)
    ref = compare_run(oracle_as_kernel(), 3, actions, **RUN)
    assert ref.events == scripted_case(3, STEPS, **RUN)[1]
    E, steps, edit, kw = CLEAR_RUN
    ref = compare_run(oracle_as_kernel(), E, scripted_case(E, steps, edit=edit, policy="tracker", **kw)[0], edit=edit, **kw)
    assert ref.events["done_clear"] == E
    # the brick band one row lower
    with pytest.raises(AssertionError, match=r"step \d+: (state|frames)"):
        compare_run(oracle_as_kernel(replace(br.BreakoutRules(), brick_top=17)), 3, actions, **RUN)
    # the spin drawn with the serve's salt and the serve with the spin's
    with pytest.raises(AssertionError, match=r"step \d+: state"):
        compare_run(oracle_as_kernel(replace(br.BreakoutRules(), salt_spin=3, salt_serve=2)), 3, actions, **RUN)
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
