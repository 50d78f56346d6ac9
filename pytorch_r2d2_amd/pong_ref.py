"""A Pong-like game in integers: the normative definition of csrc/kernels/pong.hip.

This is NOT the Atari 2600 game and claims no ALE pixel parity (that needs the ROM): it is a
native two-paddle game rendered directly at 84x84 gray, with the lumas of Atari Pong's colours,
the reference's action repeat and frame stack (env.py: repeat 4, the stack holds the frames of
the agent step), Atari Pong's 6 actions, +-1 rewards and first-to-21 episodes.  Everything in
the dynamics is an int32 (positions and velocities in Q8 fixed point, 256 = one pixel), every
random draw is a counter hash, so the kernel is compared with this module bit for bit.

Field (one uint8 plane per raw frame)
    rows 0-3          score strip, 236 where lit: the agent's points from the right edge, the
                      opponent's from the left, one column per point
    rows 4-5, 82-83   walls, 236
    rows 6-81         play area, background 87
    columns 4-5       opponent paddle, 8 rows, 148        columns 78-79  agent paddle, 8 rows, 147
    ball              2x2, 236, drawn last (clipped at the left / right edge)

State of env e: ``state[e]`` (int32, columns X Y VX VY PA PO SA SO TIMER T), ``k[e]`` (int64, the
env's RNG counter), ``ep_return[e]`` (float32).  X / Y are the Q8 position of the ball's top-left
pixel, PA / PO the top rows of the agent's / opponent's paddle, SA / SO the points, TIMER the
serve timer in raw frames, T the agent steps of the episode.

One raw frame (``PongRef._frame``), in this order:
 1. ``k += 1``.  A draw is ``env_hash(seed, k, salt * 2^32 + e)`` (env.hip's hash).
 2. agent paddle: -2 rows on actions 2 / 4, +2 on 3 / 5, clamped to rows 6..74.
 3. opponent: with probability lapse/256 it stays; else one row toward the ball's centre row
    ``(Y >> 8) + 1`` while ``VX < 0``, toward the field's centre row 44 otherwise; clamped.
 4. ``TIMER > 0``: it counts down, the ball rests (steps 5-7 are skipped).
 5. ``X += VX, Y += VY``; ``Y < 6*256`` reflects to ``2*6*256 - Y``, ``Y > 80*256`` to
    ``2*80*256 - Y``, ``VY`` flips.
 6. hit, a swept test on the leading edge L (X + 512 toward the agent, X toward the opponent) and
    the face F (78*256 / 6*256): the ball moves toward the paddle, L was at or before F and is now
    past it, and the ball's rows ``Y>>8 .. +1`` overlap the paddle's.  Then L is reflected about
    F, ``|VX| = min(|VX| + 24, 640)`` with the direction flipped, and
    ``VY = ((Y + 256 - (paddle_top + 4) * 256) * 72 >> 8) + spin``, spin one of -48 / 0 / 48.
 7. point: ``X + 512 <= 0`` gives the agent a point (reward +1), ``X >= 82*256`` the opponent
    (reward -1); the ball goes back to the centre (41, 43), ``VX`` = 192 toward the side that
    conceded, ``VY`` one of -144 / -72 / 0 / 72 / 144, ``TIMER`` = 16.

One agent step: ``action_repeat`` raw frames with one action, rewards summed; the loop stops
after the frame in which a side reaches ``points``.  Then ``T += 1``; the episode is done on
points or at ``T >= max_steps``; a done env resets in place (scores 0, paddles centred, a serve
in a drawn direction).  Plane p (oldest first) shows the state after raw frame
``action_repeat - n_stacks + p``; after a reset every plane shows the reset state.

``check`` is the comparison the GPU test applies after every step; ``PongRules`` holds the few
constants the mutation control changes (tests/test_pong_ref_cpu.py).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .refnum import mix64

H = W = 84
N_ACTIONS = 6
BG, LIT, AGENT, OPP = 87, 236, 147, 148
X, Y, VX, VY, PA, PO, SA, SO, TIMER, T = range(10)
NS = 10
Q = 256
PAD_H = 8
PAD_MIN, PAD_MAX = 6, 82 - PAD_H          # top row of a paddle
PAD_HOME = 40                             # centred: rows 40..47
Y_MAX = 80 * Q
FACE_O, FACE_A = 6 * Q, 78 * Q
X_RIGHT = 82 * Q
X_SERVE, Y_SERVE = 41 * Q, 43 * Q
CENTRE_ROW = 44
SPEED0, SPEED_UP, SPEED_MAX = 192, 24, 640
ANGLE, SPIN, SERVE_VY, SERVE_FRAMES = 72, 48, 72, 16
START_SPREAD = 128                        # randomize_start: up to this many extra timer frames
MAX_POINTS = 42                           # the score strip holds both sides' points
MAX_STACKS = 8
MAX_REPEAT = 64                           # the kernel draws a step's lapses in one wave

_M = (1 << 64) - 1


@dataclass(frozen=True)
class PongRules:
    """What the mutation control varies; the kernel has the defaults built in."""
    y_min: int = 6 * Q
    salt_lapse: int = 1
    salt_spin: int = 2
    salt_serve: int = 3
    salt_dir: int = 4
    salt_start: int = 5


def env_hash(seed: int, a, b) -> np.ndarray:
    """env.hip env_hash(seed, a, b): uint32 per element of the uint64 arrays ``a`` / ``b``."""
    a = np.atleast_1d(np.asarray(a)).astype(np.uint64)
    b = np.atleast_1d(np.asarray(b)).astype(np.uint64)
    z = mix64(np.uint64(seed & _M) ^ mix64(a * np.uint64(0x9E3779B97F4A7C15) + b))
    return (z >> np.uint64(32)).astype(np.int64)


def device_seed(seed: int) -> int:
    return (int(seed) * 0x9E3779B97F4A7C15 + 0x9067) & _M


def check_params(n_envs, n_actions, action_repeat, n_stacks, points, max_steps, lapse, shape=(H, W)):
    """The launcher's refusals (pong.hip r2_pong_env_step), as a ValueError."""
    if n_envs <= 0:
        raise ValueError("pong_device: n_envs must be positive")
    if n_actions != N_ACTIONS:
        raise ValueError(f"pong_device has Atari Pong's {N_ACTIONS} actions, not n_actions={n_actions}")
    if not 1 <= n_stacks <= MAX_STACKS or n_stacks > action_repeat or action_repeat > MAX_REPEAT:
        raise ValueError(f"pong_device: n_stacks={n_stacks} must lie in 1..{MAX_STACKS} and not exceed "
                         f"action_repeat={action_repeat} (the stack holds frames of one agent step), "
                         f"itself at most {MAX_REPEAT}")
    if tuple(shape) != (H, W):
        raise ValueError(f"pong_device renders {H}x{W} gray frames, not {tuple(shape)}")
    if not 1 <= points <= MAX_POINTS or max_steps <= 0 or not 0 <= lapse <= 256:
        raise ValueError(f"pong_device: pong_points in 1..{MAX_POINTS}, pong_max_steps > 0, "
                         "pong_opp_lapse in 0..256")


def render_plane(out: np.ndarray, bx: int, by: int, pa: int, po: int, sa: int, so: int) -> None:
    """One (84, 84) uint8 plane from a record: ball pixel position, paddle rows, points."""
    out[:] = BG
    out[4:6] = LIT
    out[82:84] = LIT
    out[0:4, :so] = LIT
    out[0:4, W - sa:] = LIT
    out[po:po + PAD_H, 4:6] = OPP
    out[pa:pa + PAD_H, 78:80] = AGENT
    out[by:by + 2, max(bx, 0):max(min(bx + 2, W), 0)] = LIT


class PongRef:
    """E games, numpy, one agent step per ``step``.  ``frames`` (E, n_stacks*84*84) uint8,
    ``reward`` / ``done`` / ``finished`` are rewritten in place.  ``render=False`` skips the planes
    (the play control); ``events`` counts what happened, for the tests' coverage checks."""

    def __init__(self, n_envs: int, seed: int = 0, action_repeat: int = 4, n_stacks: int = 4,
                 points: int = 21, max_steps: int = 5000, lapse: int = 64,
                 randomize_start: bool = False, render: bool = True, rules: PongRules = PongRules()):
        check_params(n_envs, N_ACTIONS, action_repeat, n_stacks, points, max_steps, lapse)
        self.E, self.A, self.C = int(n_envs), N_ACTIONS, int(n_stacks)
        self.action_repeat, self.points, self.max_steps = int(action_repeat), int(points), int(max_steps)
        self.lapse, self.randomize_start, self.render, self.rules = int(lapse), randomize_start, render, rules
        self.seed = device_seed(seed)
        E = self.E
        self.state = np.zeros((E, NS), dtype=np.int32)
        self.k = np.zeros(E, dtype=np.int64)
        self.ep_return = np.zeros(E, dtype=np.float32)
        self.reward = np.zeros(E, dtype=np.float32)
        self.done = np.zeros(E, dtype=bool)
        self.finished = np.full(E, np.nan, dtype=np.float32)
        self.frames = np.zeros((E, self.C * H * W), dtype=np.uint8)
        self.rec = np.zeros((E, self.C, 6), dtype=np.int32)
        self.frames_run = np.zeros(E, dtype=np.int32)     # raw frames of the last agent step
        self._e = np.arange(E, dtype=np.uint64)
        self.events = dict(hit_agent=0, hit_opp=0, point_agent=0, point_opp=0, wall=0,
                           done_mid_repeat=0, done_points=0, done_cap=0)
        self.reset_all()

    # ------------------------------------------------------------------ draws
    def _draw(self, salt: int) -> np.ndarray:
        return env_hash(self.seed, self.k, (np.uint64(salt) << np.uint64(32)) + self._e)

    def _serve_vy(self) -> np.ndarray:
        return ((self._draw(self.rules.salt_serve) % 5 - 2) * SERVE_VY).astype(np.int32)

    def _reset(self, m: np.ndarray) -> None:
        """Reset the envs of mask ``m`` in place, with draws at their current ``k``."""
        s = self.state
        fresh = np.zeros((self.E, NS), dtype=np.int32)
        fresh[:, X], fresh[:, Y] = X_SERVE, Y_SERVE
        fresh[:, VX] = np.where(self._draw(self.rules.salt_dir) & 1, SPEED0, -SPEED0)
        fresh[:, VY] = self._serve_vy()
        fresh[:, PA] = fresh[:, PO] = PAD_HOME
        fresh[:, TIMER] = SERVE_FRAMES
        s[m] = fresh[m]

    def reset_all(self):
        """Every env at the start of an episode.  ``k`` moves on by one, so a second call starts
        other episodes; ``randomize_start`` lengthens each env's first serve timer by a drawn
        0..127 frames, which de-synchronises the envs."""
        self.k += 1
        every = np.ones(self.E, dtype=bool)
        self._reset(every)
        if self.randomize_start:
            self.state[:, TIMER] += (self._draw(self.rules.salt_start) % START_SPREAD).astype(np.int32)
        self.ep_return[:] = 0
        self.rec[:] = self._record()[:, None, :]
        self._render(every)
        return self.frames

    # ------------------------------------------------------------------ one raw frame
    def _frame(self, act: np.ndarray, live: np.ndarray) -> np.ndarray:
        """Advance the envs of mask ``live`` by one raw frame; the reward of the frame (int)."""
        R, s = self.rules, self.state
        self.k += live
        x, y, vx, vy = (s[:, i].astype(np.int64) for i in (X, Y, VX, VY))
        pa, po, sa, so, timer = (s[:, i].astype(np.int64) for i in (PA, PO, SA, SO, TIMER))
        # 2. agent paddle
        dy = np.where((act == 2) | (act == 4), -2, np.where((act == 3) | (act == 5), 2, 0))
        pa = np.clip(pa + dy, PAD_MIN, PAD_MAX)
        # 3. opponent
        stays = (self._draw(R.salt_lapse) & 255) < self.lapse
        aim = np.where(vx < 0, (y >> 8) + 1, CENTRE_ROW)
        po = np.where(stays, po, np.clip(po + np.sign(aim - (po + PAD_H // 2)), PAD_MIN, PAD_MAX))
        # 4. serve timer
        move = timer <= 0
        timer = np.where(move, timer, timer - 1)
        # 5. motion and walls
        x2, y2 = x + vx, y + vy
        low, high = y2 < R.y_min, y2 > Y_MAX
        y2 = np.where(low, 2 * R.y_min - y2, np.where(high, 2 * Y_MAX - y2, y2))
        vy2 = np.where(low | high, -vy, vy)
        # 6. paddle hit
        by = y2 >> 8
        hit_a = (vx > 0) & (x + 2 * Q <= FACE_A) & (x2 + 2 * Q > FACE_A) & (by + 1 >= pa) & (by <= pa + PAD_H - 1)
        hit_o = (vx < 0) & (x >= FACE_O) & (x2 < FACE_O) & (by + 1 >= po) & (by <= po + PAD_H - 1)
        x2 = np.where(hit_a, 2 * (FACE_A - 2 * Q) - x2, np.where(hit_o, 2 * FACE_O - x2, x2))
        speed = np.minimum(np.abs(vx) + SPEED_UP, SPEED_MAX)
        vx2 = np.where(hit_a, -speed, np.where(hit_o, speed, vx))
        spin = (self._draw(R.salt_spin) % 3 - 1) * SPIN
        top = np.where(hit_a, pa, po)
        vy2 = np.where(hit_a | hit_o, (((y2 + Q - (top + PAD_H // 2) * Q) * ANGLE) >> 8) + spin, vy2)
        # 7. point
        pt_a, pt_o = x2 + 2 * Q <= 0, x2 >= X_RIGHT
        pt = pt_a | pt_o
        x2, y2 = np.where(pt, X_SERVE, x2), np.where(pt, Y_SERVE, y2)
        vx2 = np.where(pt_a, -SPEED0, np.where(pt_o, SPEED0, vx2))
        vy2 = np.where(pt, self._serve_vy(), vy2)
        # the resting ball keeps its place; everything is written back for live envs only
        m = live & move
        new = s.copy()
        new[:, PA], new[:, PO] = pa, po
        new[:, TIMER] = np.where(m & pt, SERVE_FRAMES, timer)
        for col, val in ((X, x2), (Y, y2), (VX, vx2), (VY, vy2), (SA, sa + pt_a), (SO, so + pt_o)):
            new[:, col] = np.where(m, val, s[:, col])
        s[live] = new[live]
        ev = self.events
        for name, mask in (("hit_agent", hit_a), ("hit_opp", hit_o), ("point_agent", pt_a),
                           ("point_opp", pt_o), ("wall", low | high)):
            ev[name] += int((mask & m).sum())
        return np.where(m, pt_a.astype(np.int64) - pt_o, 0)

    # ------------------------------------------------------------------ one agent step
    def _record(self) -> np.ndarray:
        s = self.state
        return np.stack([s[:, X] >> 8, s[:, Y] >> 8, s[:, PA], s[:, PO], s[:, SA], s[:, SO]], axis=1)

    def _render(self, m: np.ndarray) -> None:
        if not self.render:
            return
        planes = self.frames.reshape(self.E, self.C, H, W)
        for e in np.nonzero(m)[0]:
            for p in range(self.C):
                render_plane(planes[e, p], *(int(v) for v in self.rec[e, p]))

    def step(self, actions):
        """actions (E,) -> (reward float32, done bool, finished float32), rewritten in place."""
        act = np.asarray(actions).reshape(-1).astype(np.int64)
        if act.shape != (self.E,):
            raise ValueError(f"{self.E} actions expected")
        s, first = self.state, self.action_repeat - self.C
        live = np.ones(self.E, dtype=bool)
        total = np.zeros(self.E, dtype=np.int64)
        self.frames_run[:] = 0
        for f in range(self.action_repeat):
            total += self._frame(act, live)
            self.frames_run += live
            if f >= first:
                self.rec[live, f - first] = self._record()[live]
            live &= (s[:, SA] < self.points) & (s[:, SO] < self.points)
        s[:, T] += 1
        on_points = ~live
        done = on_points | (s[:, T] >= self.max_steps)
        self.reward[:] = total.astype(np.float32)
        self.ep_return += self.reward
        self.done[:] = done
        self.finished[:] = np.where(done, self.ep_return, np.float32(np.nan))
        ev = self.events
        ev["done_points"] += int(on_points.sum())
        ev["done_mid_repeat"] += int((on_points & (self.frames_run < self.action_repeat)).sum())
        ev["done_cap"] += int((done & ~on_points).sum())
        if done.any():
            self._reset(done)
            self.ep_return[done] = 0
            self.rec[done] = self._record()[done, None, :]
        self._render(np.ones(self.E, dtype=bool))
        return self.reward, self.done, self.finished

    def snapshot(self) -> dict:
        """Everything ``check`` compares, copied."""
        return {n: getattr(self, n).copy() for n in CHECKED}


CHECKED = ("state", "k", "ep_return", "reward", "done", "finished", "frames")


def check(got: dict, ref: dict) -> int:
    """Bit-for-bit comparison of a kernel's (or another oracle's) arrays with the oracle's
    ``snapshot``: same dtype, shape and bytes (NaN included) for every name of ``CHECKED``.
    Raises AssertionError naming the first array and element that differ; returns the number of
    arrays compared."""
    for name in CHECKED:
        g, r = np.ascontiguousarray(got[name]), np.ascontiguousarray(ref[name])
        assert g.dtype == r.dtype and g.shape == r.shape, f"{name}: {g.dtype}{g.shape} != {r.dtype}{r.shape}"
        gb, rb = g.reshape(-1).view(np.uint8), r.reshape(-1).view(np.uint8)
        if not np.array_equal(gb, rb):
            i = int(np.nonzero(gb != rb)[0][0]) // g.dtype.itemsize
            raise AssertionError(f"{name}: element {i} of {g.size} is {g.reshape(-1)[i]!r}, "
                                 f"the oracle has {r.reshape(-1)[i]!r}")
    return len(CHECKED)
