"""Serial clear-ahead (actor.clear_ahead, LearnerEngine.cover_writes), host side: the closed form
the device guard evaluates (engine/replay_check.py guard_reference, csrc/kernels/replay.hip
hoist_guard_kernel) against the brute-force window oracle of the same module, and the default."""
import numpy as np

from pytorch_r2d2_amd.engine.replay_check import (bootstrap_violations, check_windows,
                                                  guard_reference, ring_offsets)

T, N = 10, 3


def _oracle(starts, head_now, delta, cap_e, done):
    count = min(delta, cap_e)
    written = ring_offsets(head_now - count, count, cap_e)
    torn, boot = check_windows(np.asarray(starts)[None], cap_e, T, N, [written])
    return len(torn) + len(bootstrap_violations(boot, done, cap_e, T))


def test_guard_reference_equals_the_window_oracle():
    rng = np.random.default_rng(7)
    cases = flagged = 0
    for cap_e in (16, 32, 128):
        n_sub = 3
        every = np.arange(n_sub * cap_e)      # a start on every offset of every sub-ring
        for delta in (0, 1, 4, cap_e, cap_e + 3):
            for rep in range(40):
                head = int(rng.integers(cap_e))
                done = (rng.random(n_sub * cap_e) < (0.5 if rep % 2 else 0.1)).astype(np.uint8)
                if rep == 0:
                    done[:] = 0
                elif rep == 1:
                    done[:] = 1
                starts = every if rep < 4 else rng.integers(n_sub * cap_e, size=8)
                want = _oracle(starts, head, delta, cap_e, done)
                assert guard_reference(starts, head, delta, cap_e, T, N, done) == want, \
                    (cap_e, delta, head, rep)
                # slot by slot as well: equal counts must not hide two opposite mistakes
                if rep < 2:
                    for s in every[:: 3]:
                        assert (guard_reference([s], head, delta, cap_e, T, N, done)
                                == _oracle([s], head, delta, cap_e, done)), (cap_e, delta, head, s)
                        cases += 1
                cases += 1
                flagged += want > 0
    assert cases >= 2000
    assert flagged > 100          # the comparison is not between zeros


def test_guard_reference_hand_cases():
    cap_e = 32
    done = np.zeros(2 * cap_e, dtype=np.uint8)
    # head 20, 4 steps: offsets 16..19 written
    g = lambda s, d=done: guard_reference([s], 20, 4, cap_e, T, N, d)   # noqa: E731
    assert g(20) == 0 and g(cap_e + 21) == 0            # in front of the head: untouched
    assert g(16) == 1 and g(19) == 1                    # first row written
    assert g(7) == 1 and g(6) == 0 + 1                  # last learning row 16 written; 6: bootstrap
    assert g(2) == 0                                    # [2, 15) ends before 16
    assert g(28) == 0 and g(cap_e - 1 + cap_e) == 0     # wraps the ring end, ends before 16
    d1 = done.copy()
    d1[15] = 1                                          # start 6: last learning row 15 terminal
    assert g(6, d1) == 0 and g(5, d1) == 1              # (5: last row 14 not terminal, boot 15..17)
    assert guard_reference([16, 19, 7], 20, 0, cap_e, T, N, done) == 0
    assert guard_reference([3, 40], 20, cap_e + 3, cap_e, T, N, done) == 2


def test_clear_ahead_is_off_by_default():
    from pytorch_r2d2_amd.config import ActorConfig
    assert ActorConfig().clear_ahead == 0
