"""The native Breakout-like game (``env.name = "breakout_device"``).

The game is defined by ``pytorch_r2d2_amd/breakout_ref.py`` (read its docstring for the rules): a
paddle, a ball, a wall of 6 x 19 bricks worth 7 / 4 / 1 by row, ``breakout_lives`` lives, rendered
directly at 84x84 gray with the reference's action repeat and frame stack, and an opt-in
``breakout_flicker`` that blanks each shown plane with probability flicker/256.  It is a game of
this project's own, not the Atari 2600 one: no ROM, no ALE, no pixel parity.

``VecBreakout`` runs E games on a torch device with the ``VecSyntheticAtari`` contract.  On a GPU
one agent step of all E games is ONE kernel (csrc/kernels/breakout.hip: dynamics + render,
counter-hash RNG, graph-safe); on a CPU device it steps through the numpy oracle, which gives the
same bits.  ``DeviceBreakoutEnv`` is a single game with the ``PongEnv`` API for the host actors.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from .. import breakout_ref as br

_VP = ctypes.c_void_p


class BreakoutArgs(ctypes.Structure):
    """Mirror of ``struct BreakoutArgs`` (csrc/kernels/breakout.hip); size checked against the .so."""
    _fields_ = [(n, _VP) for n in ("action", "state", "k", "ep_return", "reward", "done", "finished",
                                   "frames")] + [
        ("seed", ctypes.c_ulonglong)] + [
        (n, ctypes.c_int) for n in ("E", "A", "C", "H", "W", "action_repeat", "lives", "max_steps",
                                    "flicker")]


class VecBreakout:
    """E games on a torch device.  ``frames`` (E, C*84*84) uint8 is rewritten in place by
    ``reset_all``/``step`` (the actor's torso kernel reads it directly)."""

    capture_safe = True   # step() is device-only and in place (BatchedActor.capture)

    def __init__(self, n_envs: int, device, seed: int = 0, n_actions: int = 6, action_repeat: int = 4,
                 n_stacks: int = 4, lives: int = 5, max_steps: int = 5000, flicker: int = 0,
                 shape=(84, 84), randomize_start: bool = True):
        br.check_params(n_envs, n_actions, action_repeat, n_stacks, lives, max_steps, flicker, shape)
        self.E, self.A = int(n_envs), int(n_actions)
        self.device = torch.device(device)
        self.C, (self.h, self.w) = int(n_stacks), shape
        self.action_repeat, self.lives, self.max_steps = int(action_repeat), int(lives), int(max_steps)
        self.flicker, self.randomize_start = int(flicker), randomize_start
        self.max_episode_len = self.max_steps     # episodes vary; the evaluator's default step budget
        self.fused = self.device.type == "cuda"
        # the oracle: the CPU env itself, and the host side of reset_all on a GPU
        self.ref = br.BreakoutRef(n_envs, seed, action_repeat, n_stacks, lives, max_steps, flicker,
                                  randomize_start=randomize_start, render=True)
        self._seed = self.ref.seed
        host = dict(frames=self.ref.frames, state=self.ref.state, k=self.ref.k,
                    ep_return=self.ref.ep_return, _reward=self.ref.reward, _done=self.ref.done,
                    _finished=self.ref.finished)
        for name, arr in host.items():
            t = torch.from_numpy(arr)       # shares the oracle's memory
            setattr(self, name, t.to(self.device) if self.fused else t)
        self._act = torch.zeros(n_envs, dtype=torch.int64, device=self.device)

    def reset_all(self):
        """Every game at the start of an episode (``BreakoutRef.reset_all``).  On a GPU the draws
        are made on the host from the device's counters and the result is copied over: a host
        round trip, not for the step path."""
        if self.fused:
            self.ref.k[:] = self.k.cpu().numpy()
        self.ref.reset_all()
        if self.fused:
            for name in ("frames", "state", "k", "ep_return"):
                getattr(self, name).copy_(torch.from_numpy(getattr(self.ref, name)))
        return self.frames

    def _args(self, act: torch.Tensor) -> BreakoutArgs:
        a = BreakoutArgs()
        for name, t in (("action", act), ("state", self.state), ("k", self.k),
                        ("ep_return", self.ep_return), ("reward", self._reward), ("done", self._done),
                        ("finished", self._finished), ("frames", self.frames)):
            setattr(a, name, t.data_ptr())
        a.seed = self._seed
        a.E, a.A, a.C, a.H, a.W = self.E, self.A, self.C, self.h, self.w
        a.action_repeat, a.lives, a.max_steps, a.flicker = (self.action_repeat, self.lives,
                                                            self.max_steps, self.flicker)
        return a

    def step(self, actions: torch.Tensor):
        """actions (E,) int on device -> (reward (E,) f32, done (E,) bool, finished_returns).

        Games that ended are reset in place (all planes show the new serve, none blank)."""
        if not self.fused:
            self.ref.step(actions.reshape(-1).numpy())
            return self._reward, self._done, self._finished
        from ..ops._lib import check, kernels, stream_handle
        k = kernels()
        if ctypes.sizeof(BreakoutArgs) != k.r2_breakout_args_bytes():
            raise RuntimeError("BreakoutArgs layout differs from csrc/kernels/breakout.hip")
        act = actions
        if act.dtype != torch.int64 or not act.is_contiguous():
            self._act.copy_(actions.reshape(-1))
            act = self._act
        a = self._args(act)
        check(k.r2_breakout_env_step(ctypes.byref(a), _VP(stream_handle())), "breakout_env_step")
        return self._reward, self._done, self._finished


class DeviceBreakoutEnv:
    """One game with the ``PongEnv`` API (step -> (state float32 (C,84,84)/255, reward, done,
    info), reset -> state), on the oracle: the env of the compat / inproc topologies."""

    def __init__(self, seed: int = 0, action_repeat: int = 4, n_stacks: int = 4, lives: int = 5,
                 max_steps: int = 5000, flicker: int = 0):
        self.ref = br.BreakoutRef(1, seed, action_repeat, n_stacks, lives, max_steps, flicker)
        self.action_repeat, self.n_stacks = action_repeat, n_stacks
        self._fresh = True      # the game stands at the start of an episode
        rng = np.random.default_rng(seed)

        class _Space:
            n = br.N_ACTIONS

            def sample(s):
                return int(rng.integers(s.n))

        self.action_space = _Space()

    def _obs(self) -> np.ndarray:
        return self.ref.frames.reshape(self.n_stacks, br.H, br.W).astype(np.float32) / 255.0

    def step(self, action: int):
        reward, done, _ = self.ref.step([int(action)])
        self._fresh = bool(done[0])     # a finished game has already been reset in place
        return self._obs(), float(reward[0]), bool(done[0]), {}

    def reset(self):
        if not self._fresh:
            self.ref.reset_all()
            self._fresh = True
        return self._obs()
