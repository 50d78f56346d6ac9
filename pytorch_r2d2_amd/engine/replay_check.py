"""Window-integrity oracle for a replay that is written while the learner samples from it.

Pure host code (numpy).  A learner step trains on sequences it sampled earlier: at its own start
(the plain step), or inside the previous step (the hoisted step, engine/step_driver.py).  A
writer -- the batched actor, an ingest, the concurrent driver's actor round -- may overwrite ring
rows between those two moments.  Given the sampled starts and, per learner step, the ring offsets
written between the sampling of that step's batch and its training, ``check_windows`` reports

* torn samples: the learning window ``[s, s + T)`` meets the written set;
* bootstrap overlaps: the window is whole but its ``n`` bootstrap rows ``[s + T, s + T + n)`` meet
  the written set.  Those rows may belong to the next episode (being written) only when the last
  learning row is terminal, which masks the bootstrap; ``bootstrap_violations`` applies that rule.

Rows are global indices ``sub * cap_e + offset``; a window wraps inside its own sub-ring.
"""
from __future__ import annotations

from typing import Iterable, List, NamedTuple, Sequence, Union

import numpy as np


class Hit(NamedTuple):
    step: int        # learner step (row of ``starts``)
    slot: int        # position in the batch
    start: int       # the sampled global start row


def ring_offsets(head: int, count: int, cap_e: int) -> np.ndarray:
    """The ``count`` ring offsets a writer fills starting at write head ``head`` (modular; a
    count of cap_e or more covers the ring)."""
    count = min(int(count), int(cap_e))
    return (int(head) + np.arange(count, dtype=np.int64)) % int(cap_e)


def _written_mask(written, n_sub: int, cap_e: int) -> np.ndarray:
    """(n_sub, cap_e) bool.  ``written``: ring offsets common to every sub-ring (the batched
    actor: all envs share one write head), or a dict {sub-ring: offsets}."""
    m = np.zeros((n_sub, cap_e), dtype=bool)
    if isinstance(written, dict):
        for sub, offs in written.items():
            offs = np.asarray(list(offs) if not isinstance(offs, np.ndarray) else offs, dtype=np.int64)
            if offs.size:
                m[int(sub), offs % cap_e] = True
    else:
        offs = np.asarray(list(written) if not isinstance(written, np.ndarray) else written,
                          dtype=np.int64)
        if offs.size:
            m[:, offs % cap_e] = True
    return m


def check_windows(starts, cap_e: int, T: int, n: int,
                  written: Sequence[Union[Iterable[int], dict]]):
    """``starts``: (steps, B) sampled global start rows.  ``written[k]``: what was written between
    the sampling of step k's batch and its training (see ``_written_mask``).  Returns
    ``(torn, boot)``, two lists of ``Hit`` in (step, slot) order."""
    starts = np.asarray(starts, dtype=np.int64)
    if starts.ndim != 2:
        raise ValueError("starts must be (steps, B)")
    if len(written) != starts.shape[0]:
        raise ValueError("one written set per learner step")
    cap_e, T, n = int(cap_e), int(T), int(n)
    n_sub = int(starts.max() // cap_e) + 1 if starts.size else 1
    for w in written:
        if isinstance(w, dict) and w:
            n_sub = max(n_sub, max(int(s) for s in w) + 1)
    tt, tn = np.arange(T, dtype=np.int64), np.arange(T, T + n, dtype=np.int64)
    torn: List[Hit] = []
    boot: List[Hit] = []
    for k in range(starts.shape[0]):
        m = _written_mask(written[k], n_sub, cap_e)
        if not m.any():
            continue
        sub, off = starts[k] // cap_e, starts[k] % cap_e
        in_win = m[sub[:, None], (off[:, None] + tt[None, :]) % cap_e].any(1)
        in_ext = m[sub[:, None], (off[:, None] + tn[None, :]) % cap_e].any(1) if n > 0 \
            else np.zeros_like(in_win)
        for b in np.nonzero(in_win)[0]:
            torn.append(Hit(k, int(b), int(starts[k, b])))
        for b in np.nonzero(in_ext & ~in_win)[0]:
            boot.append(Hit(k, int(b), int(starts[k, b])))
    return torn, boot


def last_learning_row(start: int, cap_e: int, T: int) -> int:
    """Global row of the last learning row of the window that starts at ``start``."""
    start = int(start)
    base = start - start % cap_e
    return base + (start % cap_e + T - 1) % cap_e


def _meets_run(off, length: int, first: int, count: int, cap_e: int):
    """Does the modular window of ``length`` rows at ring offset(s) ``off`` meet the run of
    ``count`` offsets that begins at ``first``?  With d = (off - first) mod cap_e: it starts inside
    the run (d < count) or wraps round into it (d + length > cap_e)."""
    d = (np.asarray(off, dtype=np.int64) - int(first)) % int(cap_e)
    if count <= 0 or length <= 0:
        return np.zeros(d.shape, dtype=bool)
    return (d < count) | (d + int(length) > int(cap_e))


def guard_reference(starts, head_now: int, delta: int, cap_e: int, T: int, n: int, done) -> int:
    """The closed form of the device guard (csrc/kernels/replay.hip hoist_guard_kernel): how many
    of the sampled global ``starts`` are torn or in bootstrap violation after a writer whose head
    is now ``head_now`` took ``delta`` steps in every sub-ring, i.e. wrote the
    ``min(delta, cap_e)`` offsets ending just before ``head_now``.  Equals ``check_windows`` +
    ``bootstrap_violations`` on ``ring_offsets(head_now - count, count, cap_e)``."""
    starts = np.asarray(starts, dtype=np.int64).reshape(-1)
    done = np.asarray(done).reshape(-1)
    cap_e, T, n = int(cap_e), int(T), int(n)
    count = max(0, min(int(delta), cap_e))
    first = int(head_now) - count
    base, off = starts - starts % cap_e, starts % cap_e
    torn = _meets_run(off, T, first, count, cap_e)
    ext = _meets_run((off + T) % cap_e, n, first, count, cap_e)
    last = base + (off + T - 1) % cap_e
    return int((torn | (ext & (done[last] != 1))).sum())


def bootstrap_violations(boot: Sequence[Hit], done, cap_e: int, T: int) -> List[Hit]:
    """The bootstrap overlaps that are NOT allowed: the last learning row is not terminal, so the
    bootstrap would read rows that were being written.  ``done``: the replay's per-row flags."""
    done = np.asarray(done).reshape(-1)
    return [h for h in boot if int(done[last_learning_row(h.start, cap_e, T)]) != 1]
