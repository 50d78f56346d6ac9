"""Negative control of the window-integrity oracle (engine/replay_check.py): hand-built histories
with known torn samples and bootstrap overlaps; every case asserts exactly which samples are
reported.  The GPU tests that use the oracle expect it to report nothing, so this is where it is
shown to fire."""
import numpy as np
import pytest

from pytorch_r2d2_amd.engine.replay_check import (Hit, bootstrap_violations, check_windows,
                                                  last_learning_row, ring_offsets)

CAP_E, T, N = 32, 10, 3


def _ids(hits):
    return [(h.step, h.slot) for h in hits]


def test_clean_history_reports_nothing():
    # rows [2, 15) and sub-ring 1's [8, 21) (window + bootstrap); the writer is at 21..23, 0, 1
    starts = np.array([[2, CAP_E + 8], [2, CAP_E + 8]])
    torn, boot = check_windows(starts, CAP_E, T, N, [[21, 22, 23, 0, 1], []])
    assert torn == [] and boot == []
    # no written sets at all
    torn, boot = check_windows(starts, CAP_E, T, N, [[], []])
    assert torn == [] and boot == []


def test_torn_first_row_is_reported():
    # step 1, slot 2 starts exactly at the written offset; its neighbours end before / start after
    starts = np.array([[0, 1, 2], [0, 20, 5]])
    torn, boot = check_windows(starts, CAP_E, T, N, [[], [20]])
    assert torn == [Hit(1, 1, 20)]
    assert boot == []          # window [5, 15) + bootstrap [15, 18) stays clear of 20


def test_torn_last_row_is_reported():
    # offset 14 is the last learning row of start 5, a bootstrap row of start 2 (rows 12..14) and
    # outside start 15
    starts = np.array([[5, 2, 15]])
    torn, boot = check_windows(starts, CAP_E, T, N, [[14]])
    assert torn == [Hit(0, 0, 5)]
    assert boot == [Hit(0, 1, 2)]


def test_window_straddling_the_wrap_point():
    # start 28 in sub-ring 2: learning rows 28..31, 0..5, bootstrap rows 6..8 (modular)
    s = 2 * CAP_E + 28
    starts = np.array([[s], [s], [s], [s]])
    torn, boot = check_windows(starts, CAP_E, T, N, [[0], [5], [6], [9]])
    assert _ids(torn) == [(0, 0), (1, 0)]
    assert _ids(boot) == [(2, 0)]
    assert last_learning_row(s, CAP_E, T) == 2 * CAP_E + 5
    # a writer that wraps: head 30, 4 rows -> offsets 30, 31, 0, 1
    np.testing.assert_array_equal(ring_offsets(30, 4, CAP_E), [30, 31, 0, 1])
    torn, boot = check_windows(np.array([[2 * CAP_E + 22]]), CAP_E, T, N, [ring_offsets(30, 4, CAP_E)])
    assert _ids(torn) == [(0, 0)]       # learning rows 22..31 meet 30, 31
    torn, boot = check_windows(np.array([[2 * CAP_E + 19]]), CAP_E, T, N, [ring_offsets(30, 4, CAP_E)])
    assert torn == [] and _ids(boot) == [(0, 0)]   # bootstrap rows 29..31


def test_bootstrap_overlap_with_and_without_a_terminal_row():
    # both samples' bootstrap rows [15, 18) / sub-ring 1's [15, 18) are written; only sub-ring 0's
    # last learning row (offset 14) is terminal
    starts = np.array([[5, CAP_E + 5]])
    torn, boot = check_windows(starts, CAP_E, T, N, [[16]])
    assert torn == []
    assert boot == [Hit(0, 0, 5), Hit(0, 1, CAP_E + 5)]
    done = np.zeros(2 * CAP_E, dtype=np.uint8)
    done[14] = 1
    assert bootstrap_violations(boot, done, CAP_E, T) == [Hit(0, 1, CAP_E + 5)]
    done[CAP_E + 14] = 1
    assert bootstrap_violations(boot, done, CAP_E, T) == []
    # a terminal flag on another row of the window does not excuse the overlap
    done[:] = 0
    done[13] = done[15] = 1
    assert _ids(bootstrap_violations(boot, done, CAP_E, T)) == [(0, 0), (0, 1)]


def test_per_subring_written_sets():
    # an ingest writes one sub-ring only: the same offsets elsewhere are untouched
    starts = np.array([[5, CAP_E + 5, 2 * CAP_E + 5]])
    torn, boot = check_windows(starts, CAP_E, T, N, [{1: [7, 8]}])
    assert torn == [Hit(0, 1, CAP_E + 5)] and boot == []
    # a written sub-ring that no sample comes from
    torn, boot = check_windows(starts, CAP_E, T, N, [{5: [7, 8]}])
    assert torn == [] and boot == []


def test_torn_wins_over_bootstrap_overlap():
    # a sample whose window and bootstrap rows are both written is torn, and listed once
    torn, boot = check_windows(np.array([[5]]), CAP_E, T, N, [[14, 15]])
    assert torn == [Hit(0, 0, 5)] and boot == []


def test_argument_checks():
    with pytest.raises(ValueError):
        check_windows(np.zeros(4, dtype=np.int64), CAP_E, T, N, [[]])
    with pytest.raises(ValueError):
        check_windows(np.zeros((2, 4), dtype=np.int64), CAP_E, T, N, [[]])
