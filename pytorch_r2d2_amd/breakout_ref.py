"""A Breakout-like game in integers: the normative definition of csrc/kernels/breakout.hip.

This is NOT the Atari 2600 game and claims no ALE pixel parity (that needs the ROM): it is a
native one-paddle game with a brick wall, rendered directly at 84x84 gray, with the reference's
action repeat and frame stack (env.py: repeat 4, the stack holds the frames of the agent step),
Atari Pong's 6 actions (as pong_ref.py; FIRE does nothing), rewards of 7 / 4 / 1 by brick row,
lives and a long horizon.  Everything in the dynamics is an int32 (positions and velocities in Q8
fixed point, 256 = one pixel), every random draw is pong_ref's counter hash, so the kernel is
compared with this module bit for bit.  An opt-in ``flicker`` blanks each shown plane with a set
probability (the flickering-Atari set-up of the recurrent-DQN literature) without touching the game.

Field (one uint8 plane per raw frame; every luma is distinct and non-zero)
    rows 0-3          status strip, background 24; 4 columns of 200 per remaining life from the left
    rows 4-5          top wall, 142
    columns 0-3 and 80-83 from row 4 down: side walls, 142
    columns 4-79      play area, background 24; the bottom is open
    bricks            6 rows x 19 columns, each 4 px wide and 2 px tall: brick row r is rows 16+2r
                      and 17+2r, brick column j is columns 4+4j .. 7+4j (one aligned 4-byte word of
                      a row); lumas by row from the top 98 119 133 151 129 90
    paddle            12 px wide on rows 78-79, left column PX in 4..68, 110
    ball              2x2, 236, drawn last (clipped at the bottom edge)

State of env e: ``state[e]`` (int32, columns X Y VX VY PX LIVES TIMER T B0..B5), ``k[e]`` (int64,
the env's RNG counter), ``ep_return[e]`` (float32).  X / Y are the Q8 position of the ball's
top-left pixel, PX the paddle's left column, TIMER the serve timer in raw frames, T the agent steps
of the episode, B0..B5 one word per brick row from the top (bit j set: brick j stands; a full row
is 0x7FFFF).

One raw frame (``BreakoutRef._frame``), in this order:
 1. ``k += 1``.  A draw is ``pong_ref.env_hash(seed, k, salt * 2^32 + e)``.
 2. paddle: +3 px on actions 2 / 4, -3 on 3 / 5, clamped to columns 4..68.
 3. ``TIMER > 0``: it counts down, the ball rests (steps 4-7 are skipped).
 4. ``X += VX, Y += VY``; ``X < 4*256`` reflects to ``2*4*256 - X``, ``X > 78*256`` to
    ``2*78*256 - X``, ``VX`` flips; then ``Y < 6*256`` reflects to ``2*6*256 - Y``, ``VY`` flips.
    A position exactly on a wall is not reflected.
 5. brick hit: the leading row is ``Y >> 8`` when ``VY < 0``, else ``(Y >> 8) + 1`` (``VY`` as step
    4 left it).  If it lies in the brick band (rows 16..27) its brick row is
    ``r = (row - 16) >> 1`` and the columns ``X >> 8``, then ``(X >> 8) + 1`` are tested (a column
    c outside 4..79 holds no brick; its brick column is ``(c - 4) >> 2``): the first standing
    brick found is removed, the frame's reward is its row's value (7 7 4 4 1 1 from the top),
    ``VY`` flips, and in rows 0-3 a ``|VY|`` below 320 becomes 320 (the sign kept; a ``VY`` of 0
    counts as upward-positive, +320).  At most one brick goes per raw frame; ``Y`` is not moved.
 6. paddle hit, a swept test on the ball's bottom edge ``Y + 512`` and the face 78*256: ``VY > 0``
    (after step 5), the edge was at or above the face before step 4 and is past it now, and the
    ball's columns ``X>>8 .. +1`` overlap the paddle's ``PX .. PX+11``.  Then the edge is reflected
    about the face (``Y = 2*76*256 - Y``), ``|VY| = min(|VY| + 8, 448)`` now upward, and
    ``VX = ((X + 256 - (PX + 6) * 256) * 40 >> 8) + spin``, spin one of -32 / 0 / 32 (draw % 3).
 7. ``Y >= 84*256``: a life is lost; the ball is served again from (41, 40) with ``VY`` = +160,
    ``VX`` one of -144 / -72 / 72 / 144 (draw % 4), ``TIMER`` = 16.

One agent step: ``action_repeat`` raw frames with one action, rewards summed; the loop stops
after the frame in which the last life is lost or the last brick falls.  Then ``T += 1``; the
episode is done when lives are 0, the wall is empty or ``T >= max_steps``; a done env resets in
place (full wall, ``lives`` lives, paddle at column 36, a serve drawn at the env's present ``k``,
T = 0).  Plane p (oldest first) shows the state after raw frame ``action_repeat - n_stacks + p``;
after a reset every plane shows the reset state.

Flicker (``flicker`` in 0..256): plane p of a step is all zero bytes when the draw with the
flicker's salt at that raw frame's ``k`` has ``(draw & 255) < flicker``.  The draw does not move
``k`` and touches no state, so a run with flicker and the same run without it have identical
``state``, ``k``, rewards and dones.  Planes written by a reset (in ``step`` or ``reset_all``) are
never blank.

``check`` (pong_ref's) is the comparison the GPU test applies after every step; ``BreakoutRules``
holds the few constants the mutation control changes (tests/test_breakout_ref_cpu.py).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .pong_ref import CHECKED, check, device_seed, env_hash  # noqa: F401  (check / CHECKED re-exported)

H = W = 84
N_ACTIONS = 6
BG, WALL, LIFE, PADDLE, BALL = 24, 142, 200, 110, 236
ROW_LUMA = (98, 119, 133, 151, 129, 90)
ROW_VALUE = (7, 7, 4, 4, 1, 1)
X, Y, VX, VY, PX, LIVES, TIMER, T, B0 = range(9)
ROWS, COLS = 6, 19
NS = B0 + ROWS
FULL_ROW = (1 << COLS) - 1
Q = 256
BRICK_TOP, BRICK_H, BRICK_W = 16, 2, 4
UPPER_ROWS = 4                            # brick rows whose hit raises |VY| to SPEED_UPPER
PLAY_LEFT, PLAY_RIGHT = 4, 80             # play area columns 4..79
PAD_W, PAD_ROW, PAD_STEP = 12, 78, 3
PAD_MIN, PAD_MAX = PLAY_LEFT, PLAY_RIGHT - PAD_W
PAD_HOME = 36                             # centred: columns 36..47
X_MIN, X_MAX = PLAY_LEFT * Q, (PLAY_RIGHT - 2) * Q
Y_MIN, Y_OUT = 6 * Q, H * Q
FACE = PAD_ROW * Q
X_SERVE, Y_SERVE = 41 * Q, 40 * Q
SERVE_VY, SERVE_VX = 160, (-144, -72, 72, 144)
SPEED_UPPER, SPEED_UP, SPEED_MAX = 320, 8, 448
ANGLE, SPIN, SERVE_FRAMES = 40, 32, 16
START_SPREAD = 128                        # randomize_start: up to this many extra timer frames
MAX_LIVES = 5                             # the status strip's lives stay left of the field's middle
MAX_STACKS = 8
MAX_REPEAT = 64                           # the kernel draws a step's flicker bits in one wave


@dataclass(frozen=True)
class BreakoutRules:
    """What the mutation control varies; the kernel has the defaults built in."""
    brick_top: int = BRICK_TOP
    salt_spin: int = 2
    salt_serve: int = 3
    salt_start: int = 5
    salt_flicker: int = 6


def check_params(n_envs, n_actions, action_repeat, n_stacks, lives, max_steps, flicker, shape=(H, W)):
    """The launcher's refusals (breakout.hip r2_breakout_env_step), as a ValueError."""
    if n_envs <= 0:
        raise ValueError("breakout_device: n_envs must be positive")
    if n_actions != N_ACTIONS:
        raise ValueError(f"breakout_device has Atari Pong's {N_ACTIONS} actions, not n_actions={n_actions}")
    if not 1 <= n_stacks <= MAX_STACKS or n_stacks > action_repeat or action_repeat > MAX_REPEAT:
        raise ValueError(f"breakout_device: n_stacks={n_stacks} must lie in 1..{MAX_STACKS} and not exceed "
                         f"action_repeat={action_repeat} (the stack holds frames of one agent step), "
                         f"itself at most {MAX_REPEAT}")
    if tuple(shape) != (H, W):
        raise ValueError(f"breakout_device renders {H}x{W} gray frames, not {tuple(shape)}")
    if not 1 <= lives <= MAX_LIVES or max_steps <= 0 or not 0 <= flicker <= 256:
        raise ValueError(f"breakout_device: breakout_lives in 1..{MAX_LIVES}, breakout_max_steps > 0, "
                         "breakout_flicker in 0..256")


def render_plane(out: np.ndarray, bx: int, by: int, px: int, lives: int, bricks,
                 brick_top: int = BRICK_TOP) -> None:
    """One (84, 84) uint8 plane from a record: ball pixel position, paddle column, lives and the
    six brick words."""
    out[:] = BG
    out[0:4, :4 * lives] = LIFE
    out[4:6] = WALL
    out[4:, :PLAY_LEFT] = WALL
    out[4:, PLAY_RIGHT:] = WALL
    bits = (np.asarray(bricks, dtype=np.int64)[:, None] >> np.arange(COLS)) & 1          # (6, 19)
    luma = np.where(bits == 1, np.asarray(ROW_LUMA)[:, None], BG).astype(np.uint8)
    out[brick_top:brick_top + ROWS * BRICK_H, PLAY_LEFT:PLAY_RIGHT] = luma.repeat(BRICK_H, 0).repeat(BRICK_W, 1)
    out[PAD_ROW:PAD_ROW + 2, px:px + PAD_W] = PADDLE
    out[max(by, 0):max(by + 2, 0), max(bx, 0):max(bx + 2, 0)] = BALL


class BreakoutRef:
    """E games, numpy, one agent step per ``step``.  ``frames`` (E, n_stacks*84*84) uint8,
    ``reward`` / ``done`` / ``finished`` are rewritten in place.  ``render=False`` skips the planes
    (the play control); ``events`` counts what happened, for the tests' coverage checks."""

    def __init__(self, n_envs: int, seed: int = 0, action_repeat: int = 4, n_stacks: int = 4,
                 lives: int = 5, max_steps: int = 5000, flicker: int = 0,
                 randomize_start: bool = False, render: bool = True,
                 rules: BreakoutRules = BreakoutRules()):
        check_params(n_envs, N_ACTIONS, action_repeat, n_stacks, lives, max_steps, flicker)
        self.E, self.A, self.C = int(n_envs), N_ACTIONS, int(n_stacks)
        self.action_repeat, self.lives, self.max_steps = int(action_repeat), int(lives), int(max_steps)
        self.flicker, self.randomize_start, self.render, self.rules = int(flicker), randomize_start, render, rules
        self.seed = device_seed(seed)
        E = self.E
        self.state = np.zeros((E, NS), dtype=np.int32)
        self.k = np.zeros(E, dtype=np.int64)
        self.ep_return = np.zeros(E, dtype=np.float32)
        self.reward = np.zeros(E, dtype=np.float32)
        self.done = np.zeros(E, dtype=bool)
        self.finished = np.full(E, np.nan, dtype=np.float32)
        self.frames = np.zeros((E, self.C * H * W), dtype=np.uint8)
        self.rec = np.zeros((E, self.C, 4 + ROWS), dtype=np.int32)
        self.blank = np.zeros((E, self.C), dtype=bool)    # planes of the last step that flicker blanked
        self.frames_run = np.zeros(E, dtype=np.int32)     # raw frames of the last agent step
        self._e = np.arange(E, dtype=np.uint64)
        self._rows = np.arange(E)
        self.events = dict(brick=0, brick_upper=0, paddle=0, side=0, top=0, lost=0,
                           done_lives=0, done_clear=0, done_cap=0, done_mid_repeat=0)
        self.reset_all()

    # ------------------------------------------------------------------ draws
    def _draw(self, salt: int, k=None) -> np.ndarray:
        return env_hash(self.seed, self.k if k is None else k, (np.uint64(salt) << np.uint64(32)) + self._e)

    def _serve_vx(self) -> np.ndarray:
        return np.asarray(SERVE_VX, dtype=np.int32)[self._draw(self.rules.salt_serve) % 4]

    def _reset(self, m: np.ndarray) -> None:
        """Reset the envs of mask ``m`` in place, with a draw at their current ``k``."""
        fresh = np.zeros((self.E, NS), dtype=np.int32)
        fresh[:, X], fresh[:, Y] = X_SERVE, Y_SERVE
        fresh[:, VX], fresh[:, VY] = self._serve_vx(), SERVE_VY
        fresh[:, PX], fresh[:, LIVES], fresh[:, TIMER] = PAD_HOME, self.lives, SERVE_FRAMES
        fresh[:, B0:] = FULL_ROW
        self.state[m] = fresh[m]

    def reset_all(self):
        """Every env at the start of an episode.  ``k`` moves on by one, so a second call starts
        other episodes; ``randomize_start`` lengthens each env's first serve timer by a drawn
        0..127 frames, which de-synchronises the envs.  No plane is blank."""
        self.k += 1
        every = np.ones(self.E, dtype=bool)
        self._reset(every)
        if self.randomize_start:
            self.state[:, TIMER] += (self._draw(self.rules.salt_start) % START_SPREAD).astype(np.int32)
        self.ep_return[:] = 0
        self.rec[:] = self._record()[:, None, :]
        self.blank[:] = False
        self._render()
        return self.frames

    # ------------------------------------------------------------------ one raw frame
    def _frame(self, act: np.ndarray, live: np.ndarray) -> np.ndarray:
        """Advance the envs of mask ``live`` by one raw frame; the reward of the frame (int)."""
        R, s = self.rules, self.state
        self.k += live
        x, y, vx, vy = (s[:, i].astype(np.int64) for i in (X, Y, VX, VY))
        px, lives, timer = (s[:, i].astype(np.int64) for i in (PX, LIVES, TIMER))
        bricks = s[:, B0:].astype(np.int64)
        # 2. paddle
        dx = np.where((act == 2) | (act == 4), PAD_STEP, np.where((act == 3) | (act == 5), -PAD_STEP, 0))
        px = np.clip(px + dx, PAD_MIN, PAD_MAX)
        # 3. serve timer
        move = timer <= 0
        timer = np.where(move, timer, timer - 1)
        # 4. motion and walls
        x2, y2 = x + vx, y + vy
        left, right = x2 < X_MIN, x2 > X_MAX
        x2 = np.where(left, 2 * X_MIN - x2, np.where(right, 2 * X_MAX - x2, x2))
        vx2 = np.where(left | right, -vx, vx)
        top = y2 < Y_MIN
        y2 = np.where(top, 2 * Y_MIN - y2, y2)
        vy2 = np.where(top, -vy, vy)
        # 5. brick hit
        lead = np.where(vy2 < 0, y2 >> 8, (y2 >> 8) + 1) - R.brick_top
        in_band = (lead >= 0) & (lead < ROWS * BRICK_H)
        r = np.clip(lead >> 1, 0, ROWS - 1)
        word = bricks[self._rows, r]
        c0 = x2 >> 8
        j0, j1 = np.clip((c0 - PLAY_LEFT) >> 2, 0, COLS - 1), np.clip((c0 + 1 - PLAY_LEFT) >> 2, 0, COLS - 1)
        h0 = in_band & (c0 >= PLAY_LEFT) & (c0 < PLAY_RIGHT) & (((word >> j0) & 1) == 1)
        h1 = in_band & ~h0 & (c0 + 1 >= PLAY_LEFT) & (c0 + 1 < PLAY_RIGHT) & (((word >> j1) & 1) == 1)
        hit = h0 | h1
        word = np.where(hit, word & ~(1 << np.where(h0, j0, j1)), word)
        value = np.asarray(ROW_VALUE, dtype=np.int64)[r]
        vy3 = np.where(hit, -vy2, vy2)
        raised = hit & (r < UPPER_ROWS) & (np.abs(vy3) < SPEED_UPPER)
        vy3 = np.where(raised, np.where(vy3 < 0, -SPEED_UPPER, SPEED_UPPER), vy3)
        # 6. paddle hit
        bx = x2 >> 8
        pad = (vy3 > 0) & (y + 2 * Q <= FACE) & (y2 + 2 * Q > FACE) & (bx + 1 >= px) & (bx <= px + PAD_W - 1)
        y3 = np.where(pad, 2 * (FACE - 2 * Q) - y2, y2)
        spin = (self._draw(R.salt_spin) % 3 - 1) * SPIN
        vy4 = np.where(pad, -np.minimum(np.abs(vy3) + SPEED_UP, SPEED_MAX), vy3)
        vx3 = np.where(pad, (((x2 + Q - (px + PAD_W // 2) * Q) * ANGLE) >> 8) + spin, vx2)
        # 7. a life lost
        lost = y3 >= Y_OUT
        x3, y4 = np.where(lost, X_SERVE, x2), np.where(lost, Y_SERVE, y3)
        vx4, vy5 = np.where(lost, self._serve_vx(), vx3), np.where(lost, SERVE_VY, vy4)
        # the resting ball keeps its place; everything is written back for live envs only
        m = live & move
        new = s.copy()
        new[:, PX] = px
        new[:, TIMER] = np.where(m & lost, SERVE_FRAMES, timer)
        for col, val in ((X, x3), (Y, y4), (VX, vx4), (VY, vy5), (LIVES, lives - lost)):
            new[:, col] = np.where(m, val, s[:, col])
        new[self._rows, B0 + r] = np.where(m, word, s[self._rows, B0 + r])
        s[live] = new[live]
        ev = self.events
        for name, mask in (("brick", hit), ("brick_upper", raised), ("paddle", pad), ("side", left | right),
                           ("top", top), ("lost", lost)):
            ev[name] += int((mask & m).sum())
        return np.where(m & hit, value, 0)

    # ------------------------------------------------------------------ one agent step
    def _record(self) -> np.ndarray:
        s = self.state
        return np.concatenate([np.stack([s[:, X] >> 8, s[:, Y] >> 8, s[:, PX], s[:, LIVES]], axis=1), s[:, B0:]], axis=1)

    def _render(self) -> None:
        if not self.render:
            return
        planes = self.frames.reshape(self.E, self.C, H, W)
        for e in range(self.E):
            for p in range(self.C):
                if self.blank[e, p]:
                    planes[e, p] = 0
                else:
                    rec = self.rec[e, p]
                    render_plane(planes[e, p], int(rec[0]), int(rec[1]), int(rec[2]), int(rec[3]), rec[4:],
                                 self.rules.brick_top)

    def step(self, actions):
        """actions (E,) -> (reward float32, done bool, finished float32), rewritten in place."""
        act = np.asarray(actions).reshape(-1).astype(np.int64)
        if act.shape != (self.E,):
            raise ValueError(f"{self.E} actions expected")
        s, first = self.state, self.action_repeat - self.C
        live = np.ones(self.E, dtype=bool)
        total = np.zeros(self.E, dtype=np.int64)
        self.frames_run[:] = 0
        for p in range(self.C):      # plane p shows raw frame first + p, whose counter is k + 1 + first + p
            draw = self._draw(self.rules.salt_flicker, self.k + (1 + first + p))
            self.blank[:, p] = (draw & 255) < self.flicker
        for f in range(self.action_repeat):
            total += self._frame(act, live)
            self.frames_run += live
            if f >= first:
                self.rec[live, f - first] = self._record()[live]
            live &= (s[:, LIVES] > 0) & (s[:, B0:] != 0).any(axis=1)
        s[:, T] += 1
        on_lives, on_clear = s[:, LIVES] <= 0, ~(s[:, B0:] != 0).any(axis=1)
        done = on_lives | on_clear | (s[:, T] >= self.max_steps)
        self.reward[:] = total.astype(np.float32)
        self.ep_return += self.reward
        self.done[:] = done
        self.finished[:] = np.where(done, self.ep_return, np.float32(np.nan))
        ev = self.events
        ev["done_lives"] += int(on_lives.sum())
        ev["done_clear"] += int((on_clear & ~on_lives).sum())
        ev["done_mid_repeat"] += int((~live & (self.frames_run < self.action_repeat)).sum())
        ev["done_cap"] += int((done & ~on_lives & ~on_clear).sum())
        if done.any():
            self._reset(done)
            self.ep_return[done] = 0
            self.rec[done] = self._record()[done, None, :]
            self.blank[done] = False
        self._render()
        return self.reward, self.done, self.finished

    def snapshot(self) -> dict:
        """Everything ``check`` compares, copied."""
        return {n: getattr(self, n).copy() for n in CHECKED}
