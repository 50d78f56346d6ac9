"""Environments.

* ``PongEnv`` -- reference-compatible Atari adapter (``/root/reference/env.py:14-37``): gym
  ``Pong-v0``, gray 84x84, action repeat 4, stack of the 4 frames of the agent step.  Needs
  ``gym`` + ``cv2`` (absent in this image: construction raises a clear error).
* ``SyntheticAtariEnv`` -- deterministic Atari-shaped (4,84,84) uint8 frames, configurable
  episode length and reward; same step/reset API.  Used by tests and benchmarks.
* ``VecSyntheticAtari`` -- the same dynamics for E environments at once on the GPU (frames are
  produced on device, written straight into the actor's input buffer).
* ``VecPong`` / ``DevicePongEnv`` -- a native Pong-like game (``env.name = "pong_device"``,
  pong_ref.py; not ALE): E games per kernel launch on the GPU, or one on the host.
* ``VecBreakout`` / ``DeviceBreakoutEnv`` -- a native Breakout-like game with optional frame
  flicker (``env.name = "breakout_device"``, breakout_ref.py; not ALE), built the same way.
* ``CartPoleEnv`` / ``VecCartPole`` -- CartPole-v1 dynamics (numpy / torch vectorised).
* ``DMLabSynthEnv`` -- 96x72 RGB synthetic frames for the DMLab-30 preset.
"""
from .breakout_device import DeviceBreakoutEnv, VecBreakout
from .cartpole import CartPoleEnv, VecCartPole
from .pong import PongEnv, preprocess
from .pong_device import DevicePongEnv, VecPong
from .synthetic import DMLabSynthEnv, SyntheticAtariEnv, VecSyntheticAtari


def make_env(cfg, seed: int = 0):
    e = cfg.env
    if e.name == "pong":
        return PongEnv(e.action_repeat, e.n_stacks)
    if e.name == "pong_device":
        return DevicePongEnv(seed=seed, action_repeat=e.action_repeat, n_stacks=e.n_stacks,
                             points=e.pong_points, max_steps=e.pong_max_steps, lapse=e.pong_opp_lapse)
    if e.name == "breakout_device":
        if e.channels_per_frame != 1:
            raise ValueError("breakout_device renders gray frames (env.channels_per_frame = 1)")
        return DeviceBreakoutEnv(seed=seed, action_repeat=e.action_repeat, n_stacks=e.n_stacks,
                                 lives=e.breakout_lives, max_steps=e.breakout_max_steps,
                                 flicker=e.breakout_flicker)
    if e.name == "cartpole":
        return CartPoleEnv(seed=seed, max_steps=e.episode_len)
    if e.name == "dmlab_synth":
        return DMLabSynthEnv(seed=seed, episode_len=e.episode_len, n_actions=e.n_actions,
                             switch=e.switch, cue_only_first=e.cue_only_first)
    return SyntheticAtariEnv(seed=seed, episode_len=e.episode_len, n_actions=e.n_actions,
                             action_repeat=e.action_repeat, n_stacks=e.n_stacks, switch=e.switch,
                             cue_only_first=e.cue_only_first)


def make_device_env(cfg, n_envs: int, device, seed: int = 0, randomize_start: bool = True):
    """The vectorised env of the native drivers (``run_native``, ``run_split``, the evaluator, the
    actor benchmark): ``VecPong`` for ``env.name = "pong_device"``, ``VecBreakout`` for
    ``"breakout_device"``, for every other name the ``VecSyntheticAtari`` of ``cfg``'s geometry."""
    e = cfg.env
    if e.name == "pong_device":
        if e.channels_per_frame != 1:
            raise ValueError("pong_device renders gray frames (env.channels_per_frame = 1)")
        return VecPong(n_envs, device, seed=seed, n_actions=cfg.model.n_actions,
                       action_repeat=e.action_repeat, n_stacks=e.n_stacks, points=e.pong_points,
                       max_steps=e.pong_max_steps, lapse=e.pong_opp_lapse,
                       shape=(e.frame_h, e.frame_w), randomize_start=randomize_start)
    if e.name == "breakout_device":
        if e.channels_per_frame != 1:
            raise ValueError("breakout_device renders gray frames (env.channels_per_frame = 1)")
        return VecBreakout(n_envs, device, seed=seed, n_actions=cfg.model.n_actions,
                           action_repeat=e.action_repeat, n_stacks=e.n_stacks, lives=e.breakout_lives,
                           max_steps=e.breakout_max_steps, flicker=e.breakout_flicker,
                           shape=(e.frame_h, e.frame_w), randomize_start=randomize_start)
    return VecSyntheticAtari(n_envs, device, seed=seed, episode_len=e.episode_len,
                             n_actions=cfg.model.n_actions,
                             n_stacks=e.channels_per_frame * e.n_stacks,
                             shape=(e.frame_h, e.frame_w), switch=e.switch,
                             cue_only_first=e.cue_only_first, randomize_start=randomize_start)


__all__ = ["PongEnv", "preprocess", "SyntheticAtariEnv", "VecSyntheticAtari", "CartPoleEnv",
           "VecCartPole", "DMLabSynthEnv", "VecPong", "DevicePongEnv", "VecBreakout", "DeviceBreakoutEnv",
           "make_env", "make_device_env"]
