"""The native Pong-like game (``env.name = "pong_device"``).

The game is defined by ``pytorch_r2d2_amd/pong_ref.py`` (read its docstring for the rules): two
paddles, a ball, +-1 rewards, first to ``pong_points``, rendered directly at 84x84 gray with the
reference's action repeat and frame stack.  It is a game of this project's own, not the Atari
2600 one: no ROM, no ALE, no pixel parity with ``PongEnv``.

``VecPong`` runs E games on a torch device with the ``VecSyntheticAtari`` contract.  On a GPU one
agent step of all E games is ONE kernel (csrc/kernels/pong.hip: dynamics + render, counter-hash
RNG, graph-safe); on a CPU device it steps through the numpy oracle, which gives the same bits.
``DevicePongEnv`` is a single game with the ``PongEnv`` API for the host actors.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from .. import pong_ref as pr

_VP = ctypes.c_void_p


class PongArgs(ctypes.Structure):
    """Mirror of ``struct PongArgs`` (csrc/kernels/pong.hip); size checked against the .so."""
    _fields_ = [(n, _VP) for n in ("action", "state", "k", "ep_return", "reward", "done", "finished",
                                   "frames")] + [
        ("seed", ctypes.c_ulonglong)] + [
        (n, ctypes.c_int) for n in ("E", "A", "C", "H", "W", "action_repeat", "points", "max_steps",
                                    "lapse")]


class VecPong:
    """E games on a torch device.  ``frames`` (E, C*84*84) uint8 is rewritten in place by
    ``reset_all``/``step`` (the actor's torso kernel reads it directly)."""

    capture_safe = True   # step() is device-only and in place (BatchedActor.capture)

    def __init__(self, n_envs: int, device, seed: int = 0, n_actions: int = 6, action_repeat: int = 4,
                 n_stacks: int = 4, points: int = 21, max_steps: int = 5000, lapse: int = 64,
                 shape=(84, 84), randomize_start: bool = True):
        pr.check_params(n_envs, n_actions, action_repeat, n_stacks, points, max_steps, lapse, shape)
        self.E, self.A = int(n_envs), int(n_actions)
        self.device = torch.device(device)
        self.C, (self.h, self.w) = int(n_stacks), shape
        self.action_repeat, self.points, self.max_steps = int(action_repeat), int(points), int(max_steps)
        self.lapse, self.randomize_start = int(lapse), randomize_start
        self.max_episode_len = self.max_steps     # episodes vary; the evaluator's default step budget
        self.fused = self.device.type == "cuda"
        # the oracle: the CPU env itself, and the host side of reset_all on a GPU
        self.ref = pr.PongRef(n_envs, seed, action_repeat, n_stacks, points, max_steps, lapse,
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
        """Every game at the start of an episode (``PongRef.reset_all``).  On a GPU the draws are
        made on the host from the device's counters and the result is copied over: a host round
        trip, not for the step path."""
        if self.fused:
            self.ref.k[:] = self.k.cpu().numpy()
        self.ref.reset_all()
        if self.fused:
            for name in ("frames", "state", "k", "ep_return"):
                getattr(self, name).copy_(torch.from_numpy(getattr(self.ref, name)))
        return self.frames

    def _args(self, act: torch.Tensor) -> PongArgs:
        a = PongArgs()
        for name, t in (("action", act), ("state", self.state), ("k", self.k),
                        ("ep_return", self.ep_return), ("reward", self._reward), ("done", self._done),
                        ("finished", self._finished), ("frames", self.frames)):
            setattr(a, name, t.data_ptr())
        a.seed = self._seed
        a.E, a.A, a.C, a.H, a.W = self.E, self.A, self.C, self.h, self.w
        a.action_repeat, a.points, a.max_steps, a.lapse = (self.action_repeat, self.points,
                                                           self.max_steps, self.lapse)
        return a

    def step(self, actions: torch.Tensor):
        """actions (E,) int on device -> (reward (E,) f32, done (E,) bool, finished_returns).

        Games that ended are reset in place (all planes show the new serve)."""
        if not self.fused:
            self.ref.step(actions.reshape(-1).numpy())
            return self._reward, self._done, self._finished
        from ..ops._lib import check, kernels, stream_handle
        k = kernels()
        if ctypes.sizeof(PongArgs) != k.r2_pong_args_bytes():
            raise RuntimeError("PongArgs layout differs from csrc/kernels/pong.hip")
        act = actions
        if act.dtype != torch.int64 or not act.is_contiguous():
            self._act.copy_(actions.reshape(-1))
            act = self._act
        a = self._args(act)
        check(k.r2_pong_env_step(ctypes.byref(a), _VP(stream_handle())), "pong_env_step")
        return self._reward, self._done, self._finished


class DevicePongEnv:
    """One game with the ``PongEnv`` API (step -> (state float32 (C,84,84)/255, reward, done,
    info), reset -> state), on the oracle: the env of the compat / inproc topologies."""

    def __init__(self, seed: int = 0, action_repeat: int = 4, n_stacks: int = 4, points: int = 21,
                 max_steps: int = 5000, lapse: int = 64):
        self.ref = pr.PongRef(1, seed, action_repeat, n_stacks, points, max_steps, lapse)
        self.action_repeat, self.n_stacks = action_repeat, n_stacks
        self._fresh = True      # the game stands at the start of an episode
        rng = np.random.default_rng(seed)

        class _Space:
            n = pr.N_ACTIONS

            def sample(s):
                return int(rng.integers(s.n))

        self.action_space = _Space()

    def _obs(self) -> np.ndarray:
        return self.ref.frames.reshape(self.n_stacks, pr.H, pr.W).astype(np.float32) / 255.0

    def step(self, action: int):
        reward, done, _ = self.ref.step([int(action)])
        self._fresh = bool(done[0])     # a finished game has already been reset in place
        return self._obs(), float(reward[0]), bool(done[0]), {}

    def reset(self):
        if not self._fresh:
            self.ref.reset_all()
            self._fresh = True
        return self._obs()
