"""The Breakout-like game's kernel (csrc/kernels/breakout.hip) against its oracle (pytorch_r2d2_amd/
breakout_ref.py), bit for bit after every agent step: state, counters, returns, outputs and every
frame byte.  The kernel under the batched actor, the evaluator and the drivers is in
test_vec_breakout_gpu.py.

The launches go through the ctypes entry point on the test's own tensors.  Every buffer the kernel
writes sits between two runs of guard elements; the outputs start poisoned (NaN floats, 0xAB
bytes).  The scripted runs, the proof that they cover every event and that the comparison rejects
wrong games live in test_breakout_ref_cpu.py."""
import ctypes

import numpy as np
import pytest
import torch

from gpu_support import DEV, NAN, Buf
from gpu_support import stop_after_a_gpu_error  # noqa: F401
from pytorch_r2d2_amd import breakout_ref as br
from pytorch_r2d2_amd.envs.breakout_device import BreakoutArgs
from pytorch_r2d2_amd.ops._lib import kernels, stream_handle
from test_breakout_ref_cpu import CHANNEL_RUN, CLEAR_RUN, EVENTS, RUN, SEED, STEPS, compare_run, scripted_case

pytestmark = pytest.mark.gpu

PLANE = 84 * 84


class Launch:
    """The kernel on guarded buffers that start as the oracle's arrays (state, counter, return)
    or poisoned (reward, done, finished, frames: the kernel writes every element of them)."""

    def __init__(self, ref):
        self.ref, E = ref, ref.E
        self.b = dict(state=Buf(ref.state, -1), k=Buf(ref.k, -1), ep_return=Buf(ref.ep_return, NAN),
                      reward=Buf.poisoned(E, torch.float32, NAN), done=Buf.poisoned(E, torch.uint8, 0xAB),
                      finished=Buf.poisoned(E, torch.float32, NAN),
                      frames=Buf.poisoned(E * ref.C * PLANE, torch.uint8, 0xAB))
        self.act = torch.zeros(E, dtype=torch.int64, device=DEV)

    def args(self, **over):
        ref, a = self.ref, BreakoutArgs()
        for name, buf in self.b.items():
            setattr(a, name, buf.p)
        a.action = self.act.data_ptr()
        a.seed = ref.seed
        a.E, a.A, a.C, a.H, a.W = ref.E, 6, ref.C, 84, 84
        a.action_repeat, a.lives, a.max_steps, a.flicker = ref.action_repeat, ref.lives, ref.max_steps, ref.flicker
        for k, v in over.items():
            setattr(a, k, v)
        return a

    def __call__(self, act):
        self.act.copy_(torch.from_numpy(np.ascontiguousarray(act, dtype=np.int64)))
        a = self.args()
        assert kernels().r2_breakout_env_step(ctypes.byref(a), stream_handle()) == 0
        torch.cuda.synchronize()
        for name, buf in self.b.items():
            buf.assert_guards(name)
        snap = self.ref.snapshot()
        return {n: self.b[n].bits().view(snap[n].dtype).reshape(snap[n].shape) for n in br.CHECKED}

    def assert_untouched(self):
        torch.cuda.synchronize()
        for name, buf in self.b.items():
            buf.assert_untouched(name)


def test_breakout_args_mirror_matches_the_library():
    assert ctypes.sizeof(BreakoutArgs) == kernels().r2_breakout_args_bytes()


def test_bitwise_run_against_the_oracle():
    """E = 3 (the smallest count at which per-env indexing can go wrong), two lives, at most 100
    steps, the 600 scripted steps: bricks, paddle and side-wall hits, lives lost, games ending on
    lives in the middle of a repeat loop and at the step cap."""
    actions, ev = scripted_case(3, STEPS, **RUN)
    assert min(ev[n] for n in ("brick", "paddle", "side", "lost", "done_lives", "done_mid_repeat", "done_cap")) >= 1
    ref = compare_run(Launch, 3, actions, **RUN)
    assert ref.events == ev


def test_bitwise_runs_from_edited_walls():
    """A wall of three bricks that the tracker clears (done_clear), and a wall with a channel
    (top-wall hits, the upper rows' speed-up): with the main run, every event of the game."""
    seen = dict(scripted_case(3, STEPS, **RUN)[1])
    for E, steps, edit, kw in (CLEAR_RUN, CHANNEL_RUN):
        actions, ev = scripted_case(E, steps, edit=edit, policy="tracker", **kw)
        ref = compare_run(Launch, E, actions, edit=edit, **kw)
        assert ref.events == ev
        for n in EVENTS:
            seen[n] += ev[n]
    assert all(seen[n] >= 1 for n in EVENTS), seen


@pytest.mark.parametrize("E,steps,kw", [(1, STEPS, RUN), (256, 8, dict(lives=1, max_steps=5)),
                                         (3, 200, dict(RUN, action_repeat=4, n_stacks=2)),
                                         (2, 120, dict(lives=1, max_steps=30, action_repeat=6, n_stacks=1)),
                                         (3, 200, dict(RUN, flicker=128))],
                         ids=["E1", "E256", "stacks2", "repeat6_stack1", "flicker128"])
def test_bitwise_run_other_shapes(E, steps, kw):
    """One env, more envs than one wave of workgroups has lanes (randomized starts, a step cap of 5
    so that every env resets within the 8 steps), two stacked planes of four frames, one plane of
    six, and half the planes blanked by the flicker."""
    actions, _ = scripted_case(E, steps, **kw)
    ref = compare_run(Launch, E, actions, randomize_start=E == 256, **kw)
    assert ref.events["done_cap"] + ref.events["done_lives"] >= (E if E == 256 else 1)


def test_launcher_refusals_write_nothing():
    ref = br.BreakoutRef(3, seed=SEED, **RUN)
    run = Launch(ref)
    k, s = kernels(), stream_handle()
    bad = dict(E0=dict(E=0), Eneg=dict(E=-3), A4=dict(A=4), A7=dict(A=7), stacks=dict(C=5), C0=dict(C=0),
               C9=dict(C=9, action_repeat=9), repeat=dict(action_repeat=3), repeat65=dict(action_repeat=65),
               H96=dict(H=96), W96=dict(W=96), swapped=dict(H=72, W=96),
               lives0=dict(lives=0), lives6=dict(lives=6), steps0=dict(max_steps=0), flickerneg=dict(flicker=-1),
               flicker257=dict(flicker=257), frames=dict(frames=None), state=dict(state=None), action=dict(action=None),
               k=dict(k=None), ep_return=dict(ep_return=None), reward=dict(reward=None), done=dict(done=None),
               finished=dict(finished=None))
    for name, over in bad.items():
        assert k.r2_breakout_env_step(ctypes.byref(run.args(**over)), s) == -1, name
    assert k.r2_breakout_env_step(None, s) == -1
    run.assert_untouched()
    # the same arguments without the fault are accepted
    ref.step([0, 0, 0])
    assert br.check(run([0, 0, 0]), ref.snapshot()) == len(br.CHECKED)
