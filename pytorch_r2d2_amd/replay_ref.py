"""Float64 oracle of the replay sampling and priority kernels (csrc/kernels/replay.hip).

Pure host code (numpy float64 and exact 64-bit integers, no torch, no GPU).  Each ``*_ref`` function
is the plain definition of one operation; the ``check_*`` functions compare what a kernel left in
memory with it.  tests/test_replay_oracle_gpu.py runs every entry point of replay.hip through them;
tests/test_replay_ref_cpu.py checks the oracle against brute-force loops and shows that the checks
reject wrong variants.

Bounds (u = 2^-24, the fp32 unit roundoff).  They are derived here, not fitted to a run:

* tree (``check_tree``): a parent is the sum of at most 64 non-negative fp32 children, added
  pairwise six deep (common.h wave_sum_x), so |parent - sum| <= 6 u sum.  The root against the
  float64 sum of the leaves therefore stays within 6 (levels - 1) u (first order).
* draws (``check_samples``): the kernel evaluates u_b = (b + r_b) / B * total in fp32 and walks
  down the tree; the leaf it returns must hold a point within d of the float64 u_b, where
  d = (levels - 1) (1e-5 + 64 * 2^-23) total: per level the ``0.99999 pv`` clamp may move the
  residual by 1e-5 of the chosen child, and the scan (at most 6 adds per lane over at most 64
  partial sums) plus the ``u - excl`` subtraction stay far below 64 * 2^-23 of the level's total.
  No draw is excluded.  prob must be leaf / root within 4 u (one division of two fp32 values,
  with room for the hardware's division expansion).
* eta-mix leaves (``check_refresh``, ``check_edit``): the window sum takes ceil(T / 64) - 1 adds
  per lane and 6 across the wave; the division by T, 1 - eta, the product and the final fma or
  multiply-add round at most 5 more times; all terms are non-negative, so the leaf is within
  (ceil(T / 64) + 10) u of the float64 value.  The maximum is exact.

``mutation`` (tests only): a deliberately wrong variant of one rule, used on the CPU to show that
the matching check rejects it.  ``MUTATIONS`` lists them.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

from .refnum import as_u64, mix64

MUTATIONS = ("wrap_prev_subring", "window_no_wrap", "range_hi_closed", "range_lo_closed",
             "mean_only", "max_only", "mean_64", "next_leaf", "n_valid_per_entry")

U24 = 2.0 ** -24
FANOUT = 64


# ------------------------------------------------------------------ geometry, RNG, CDF
def tree_geometry(cap: int):
    """(offs, sizes) of the 64-ary sum tree over ``cap`` leaves (engine/replay_hbm.py)."""
    sizes = [int(cap)]
    while sizes[-1] > 1:
        sizes.append((sizes[-1] + FANOUT - 1) // FANOUT)
    if len(sizes) < 2:
        sizes.append(1)
    offs = [0]
    for s in sizes[:-1]:
        offs.append(offs[-1] + s)
    return offs, sizes


def uniform(seed: int, ctr: int, idx) -> np.ndarray:
    """common.h r2_uniform(seed, ctr, idx): the exact float32 value in [0, 1), one per ``idx``."""
    z = mix64(as_u64(seed) ^ mix64(as_u64(ctr) * np.uint64(0x100000001B3) + as_u64(idx)))
    # 24 bits: exactly representable in fp32, and so is the product with 2^-24
    return ((z >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def leaf_cdf(leaves) -> np.ndarray:
    """Float64 inclusive cumulative sum of the (fp32) leaves."""
    return np.cumsum(np.asarray(leaves, dtype=np.float64))


def draw_points(leaves, B: int, seed: int, ctr: int) -> np.ndarray:
    """u_b = (b + uniform(seed, ctr, b)) / B * total in float64: the stratified draw points."""
    total = float(np.asarray(leaves, dtype=np.float64).sum())
    b = np.arange(B, dtype=np.float64)
    return (b + uniform(seed, ctr, np.arange(B)).astype(np.float64)) / B * total


def sample_ref(leaves, B: int, seed: int, ctr: int, mutation: Optional[str] = None):
    """The float64 sampler: the positive leaf whose mass interval holds u_b.  Returns (idx, prob).
    A tree without mass returns leaf 0 with probability 0."""
    lv = np.asarray(leaves, dtype=np.float64)
    pos = np.flatnonzero(lv > 0)
    if pos.size == 0:
        return np.zeros(B, dtype=np.int64), np.zeros(B)
    cdf = np.cumsum(lv[pos])
    j = np.minimum(np.searchsorted(cdf, draw_points(lv, B, seed, ctr), side="right"), pos.size - 1)
    if mutation == "next_leaf" and pos.size > 1:
        j = np.where(j + 1 < pos.size, j + 1, j - 1)
    idx = pos[j]
    return idx, lv[idx] / cdf[-1]


def sample_tolerance(levels: int) -> float:
    """d of ``check_samples`` as a share of the total."""
    return (levels - 1) * (1e-5 + 64 * 2.0 ** -23)


class SampleReport(NamedTuple):
    miss: float        # largest distance from u_b to the returned leaf's interval / total
    ambiguous: float   # share of draws for which d admits more than one positive leaf


def check_samples(leaves, levels: int, B: int, seed: int, ctr: int, idx, prob,
                  root=None) -> SampleReport:
    """Every draw of one sampler launch.  ``root``: the fp32 root the kernel divided by (the
    float64 total rounded to fp32 when not given)."""
    lv = np.asarray(leaves, dtype=np.float64)
    idx = np.asarray(idx).astype(np.int64).reshape(-1)
    prob = np.asarray(prob, dtype=np.float64).reshape(-1)
    assert idx.shape == (B,) and prob.shape == (B,)
    cdf = leaf_cdf(lv)
    total = float(cdf[-1])
    assert total > 0, "check_samples needs a tree with mass"
    root = float(np.float32(total)) if root is None else float(root)
    assert ((idx >= 0) & (idx < lv.size)).all(), f"index out of range: {idx[(idx < 0) | (idx >= lv.size)][:8]}"
    assert (lv[idx] > 0).all(), f"draws {np.flatnonzero(lv[idx] <= 0)[:8]} returned a leaf without mass"
    u = draw_points(lv, B, seed, ctr)
    d = sample_tolerance(levels) * total
    hi = cdf[idx]
    lo = hi - lv[idx]
    miss = np.maximum(np.maximum(lo - u, u - hi), 0.0)
    bad = np.flatnonzero(miss > d)
    assert bad.size == 0, (f"{bad.size} of {B} draws off their leaf, first b={bad[:4]} idx={idx[bad[:4]]} "
                           f"miss/total={miss[bad[:4]] / total} (d/total={d / total:.3g})")
    want = lv[idx] / root
    perr = np.abs(prob - want)
    assert (perr <= 4 * U24 * want).all(), f"prob: worst {float((perr / want).max() / U24):.3g} u"
    # positive leaves whose interval meets [u - d, u + d]
    pos = np.flatnonzero(lv > 0)
    phi = cdf[pos]
    plo = phi - lv[pos]
    first = np.searchsorted(phi, u - d, side="left")
    last = np.searchsorted(plo, u + d, side="right") - 1
    amb = float(((last - first) > 0).mean())
    return SampleReport(float(miss.max() / total), amb)


def check_tree(tree, offs, sizes, leaves=None) -> float:
    """Every parent of a sum tree against the float64 sum of its own children (slots past a
    level's size are not children), and the root against the float64 sum of the leaves.  Returns
    the largest relative parent error."""
    t = np.asarray(tree, dtype=np.float64)
    levels = len(sizes)
    assert np.isfinite(t[: offs[-1] + sizes[-1]]).all(), "tree holds non-finite values"
    worst = 0.0
    for l in range(1, levels):
        n_child, n_par = int(sizes[l - 1]), int(sizes[l])
        assert n_par == (n_child + FANOUT - 1) // FANOUT
        child = np.zeros(n_par * FANOUT)
        child[:n_child] = t[offs[l - 1]: offs[l - 1] + n_child]
        assert (child >= 0).all()
        s = child.reshape(n_par, FANOUT).sum(axis=1)
        par = t[offs[l]: offs[l] + n_par]
        err = np.abs(par - s)
        bad = np.flatnonzero(err > 6 * U24 * s)
        assert bad.size == 0, f"level {l}: parents {bad[:8]} are {par[bad[:8]]}, children sum to {s[bad[:8]]}"
        if (s > 0).any():
            worst = max(worst, float((err[s > 0] / s[s > 0]).max()))
    if leaves is not None:
        lv = np.asarray(leaves, dtype=np.float64)
        assert np.array_equal(lv, t[offs[0]: offs[0] + sizes[0]]), "level 0 differs from the leaves"
    s = float(t[offs[0]: offs[0] + sizes[0]].sum())
    root = float(t[offs[-1]])
    assert abs(root - s) <= 6 * (levels - 1) * U24 * s * (1 + 1e-6), f"root {root!r} vs {s!r}"
    return worst


# ------------------------------------------------------------------ ring rows, eta-mix
def ring_row(start, t, cap_e: int, mutation: Optional[str] = None):
    """Row ``t`` steps after ``start`` (any integer ``t``): wraps inside the sub-ring of
    ``start`` (rows [base, base + cap_e), base = start - start % cap_e)."""
    start = np.asarray(start, dtype=np.int64)
    t = np.asarray(t, dtype=np.int64)
    base = start - start % cap_e
    o = start - base + t
    if mutation == "wrap_prev_subring":      # a C remainder: negative offsets leave the sub-ring
        return np.where(o < 0, base - (-o) % cap_e, base + o % cap_e)
    return base + o % cap_e      # numpy's % is the floor modulus: always in [0, cap_e)


def seq_leaf(priority, s: int, T: int, cap_e: int, eta32, mutation: Optional[str] = None) -> float:
    """eta * max + (1 - eta) * mean of the T wrapped rows of the sequence starting at row s;
    ``eta32`` is the float32 the kernel receives, taken as float64."""
    eta = float(np.float32(eta32))
    p = np.asarray(priority, dtype=np.float64)
    t = np.arange(T, dtype=np.int64)
    if mutation == "window_no_wrap":
        rows = (s + t) % p.size
    else:
        rows = ring_row(s, t, cap_e)
    w = p[rows]
    mean = w.mean()
    if mutation == "mean_64":
        mean = p[ring_row(s, np.arange(64), cap_e)].mean()
    if mutation == "mean_only":
        return float(mean)
    if mutation == "max_only":
        return float(w.max())
    return float(eta * w.max() + (1.0 - eta) * mean)


class RefreshRef(NamedTuple):
    leaves: np.ndarray     # float64 leaves after the refresh
    touched: np.ndarray    # sorted distinct rows whose leaf was recomputed
    count: int             # dirty appends: listed candidates summed over the sampled starts


def refresh_ref(starts, is_start, priority, leaves, T: int, upd_lo: int, upd_hi: int, cap_e: int,
                eta32, mutation: Optional[str] = None) -> RefreshRef:
    """Sequence-priority refresh.  For sampled start s_b the learner rewrote the rows at offsets
    [upd_lo, upd_hi); sequence s (T rows) overlaps them iff s = ring_row(s_b, k) with
    upd_lo - T < k < upd_hi.  Every flagged candidate gets a new eta-mix leaf; each listing is one
    dirty append (duplicates across starts, and within one start when cap_e is shorter than the
    candidate range, count)."""
    flags = np.asarray(is_start)
    out = np.asarray(leaves, dtype=np.float64).copy()
    lo, hi = upd_lo - T + 1, upd_hi - 1
    if mutation == "range_hi_closed":
        hi = upd_hi
    if mutation == "range_lo_closed":
        lo = upd_lo - T
    ks = np.arange(lo, hi + 1, dtype=np.int64)
    touched, count = set(), 0
    for sb in np.asarray(starts, dtype=np.int64).reshape(-1):
        rows = ring_row(int(sb), ks, cap_e, mutation)
        rows = rows[(rows >= 0) & (rows < flags.size)]
        hit = rows[flags[rows] != 0]
        count += int(hit.size)
        touched.update(int(r) for r in hit)
    touched = np.asarray(sorted(touched), dtype=np.int64)
    for s in touched:
        out[s] = seq_leaf(priority, int(s), T, cap_e, eta32, mutation)
    return RefreshRef(out, touched, count)


def leaf_bound(T: int) -> float:
    """Relative bound of an fp32 eta-mix leaf (module docstring)."""
    return (-(-T // 64) + 10) * U24


def _bits(x) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)


def _check_leaves(before, after, want, touched, T: int) -> float:
    """Touched leaves within the bound of ``want``; every other element (guards included) keeps
    its bits.  Returns the largest relative error."""
    before, after = np.asarray(before, dtype=np.float32), np.asarray(after, dtype=np.float32)
    assert before.shape == after.shape
    keep = np.ones(after.size, dtype=bool)
    keep[touched] = False
    moved = np.flatnonzero(keep & (_bits(before) != _bits(after)))
    assert moved.size == 0, f"leaves {moved[:8]} changed but are not touched"
    got = after[touched].astype(np.float64)
    w = np.asarray(want, dtype=np.float64)[touched]
    assert np.isfinite(got).all(), f"touched leaves {touched[~np.isfinite(got)][:8]} not written"
    err = np.abs(got - w)
    bad = np.flatnonzero(err > leaf_bound(T) * w)
    assert bad.size == 0, (f"leaves {touched[bad[:6]]}: {got[bad[:6]]} vs {w[bad[:6]]} "
                           f"(bound {leaf_bound(T):.3g} relative)")
    return float((err[w > 0] / w[w > 0]).max()) if (w > 0).any() else 0.0


def _check_dirty(dirty, count: int, want_count: int, touched, max_dirty: int, poison: int = -1):
    dirty = np.asarray(dirty).astype(np.int64)
    assert int(count) == int(want_count), f"dirty count {int(count)}, oracle {int(want_count)}"
    n = min(int(count), max_dirty)
    assert (dirty[n:] == poison).all(), "dirty list written past its count or past max_dirty"
    got = set(dirty[:n].tolist())
    want = set(int(r) for r in touched)
    if count <= max_dirty:
        assert got == want, f"dirty set: extra {sorted(got - want)[:8]} missing {sorted(want - got)[:8]}"
    else:
        assert got <= want, f"dirty set: extra {sorted(got - want)[:8]}"


def check_refresh(ref: RefreshRef, before, after, dirty, count: int, max_dirty: int, T: int,
                  count0: int = 0) -> float:
    """A refresh launch: ``before`` / ``after`` are the leaf buffer (with any guard elements;
    leaf i at index i), ``dirty`` the whole dirty buffer (poisoned with -1 before the launch,
    guards included), ``count`` the counter afterwards, ``count0`` its value before."""
    want = np.zeros(np.asarray(after).size)
    want[: ref.leaves.size] = ref.leaves
    err = _check_leaves(before, after, want, ref.touched, T)
    _check_dirty(dirty, count, count0 + ref.count, ref.touched, max_dirty)
    return err


# ------------------------------------------------------------------ start marking, pending edits
class EditRef(NamedTuple):
    flags: np.ndarray      # uint8 flags afterwards
    leaves: np.ndarray     # float64 leaves afterwards
    touched: np.ndarray    # sorted distinct rows appended to the dirty list
    n_valid: int           # change of n_valid: distinct flags that actually flipped
    count: int             # dirty appends
    err: int               # apply_pending's error word (bit 2: the list overflowed)


def _edit(entries, flags, priority, leaves, T, cap_e, eta32, pending: bool, mutation):
    flags = np.asarray(flags, dtype=np.uint8).copy()
    out = np.asarray(leaves, dtype=np.float64).copy()
    touched, n_valid, count = set(), 0, 0
    for e in (int(v) for v in entries):
        if e >= 0:
            if flags[e] == 0 or mutation == "n_valid_per_entry":
                n_valid += 1
            flags[e] = 1
            out[e] = seq_leaf(priority, e, T, cap_e, eta32, mutation)
            touched.add(e)
            count += 1
        elif pending and e <= -2:
            r = -2 - e
            was = flags[r] != 0
            if was or mutation == "n_valid_per_entry":
                n_valid -= 1
            flags[r] = 0
            if was or out[r] != 0:
                out[r] = 0.0
                touched.add(r)
                count += 1
    return flags, out, np.asarray(sorted(touched), dtype=np.int64), n_valid, count


def mark_starts_ref(rows, n_rows, max_rows: int, is_start, priority, leaves, T: int, cap_e: int,
                    eta32, mutation: Optional[str] = None) -> EditRef:
    """mark_starts_kernel over the first min(n_rows, max_rows) entries (``n_rows`` None: all
    max_rows): an entry >= 0 sets the flag, writes the eta-mix leaf and appends the row; negative
    entries are ignored.  The rows of one list are distinct."""
    n = max_rows if n_rows is None else min(int(n_rows), max_rows)
    f, lv, touched, nv, cnt = _edit(np.asarray(rows).reshape(-1)[:n], is_start, priority, leaves, T,
                                    cap_e, eta32, False, mutation)
    return EditRef(f, lv, touched, nv, cnt, 0)


def apply_pending_ref(pend, pend_cnt: int, pend_cap: int, is_start, priority, leaves, T: int,
                      cap_e: int, eta32, mutation: Optional[str] = None) -> EditRef:
    """apply_pending_kernel over the first min(pend_cnt, pend_cap) entries: e >= 0 marks row e,
    e <= -2 clears row -2 - e (flag and leaf; appended only if the flag was set or the leaf was
    non-zero).  A row appears with one sign only.  Entries are applied in list order; the kernel
    applies them concurrently, which gives the same result except that a repeated clear of a row
    whose leaf is non-zero may be appended once or twice."""
    n = min(int(pend_cnt), pend_cap)
    f, lv, touched, nv, cnt = _edit(np.asarray(pend).reshape(-1)[:n], is_start, priority, leaves, T,
                                    cap_e, eta32, True, mutation)
    return EditRef(f, lv, touched, nv, cnt, 2 if int(pend_cnt) > pend_cap else 0)


def check_edit(ref: EditRef, flags_after, leaves_before, leaves_after, n_valid_delta: int, dirty,
               count: int, max_dirty: int, T: int, count0: int = 0) -> float:
    """A mark_starts / apply_pending launch.  ``flags_after`` and the leaf buffers may carry guard
    elements around the replay: ``ref.flags`` / ``ref.leaves`` are then given with the same
    guards.  Flags, the n_valid change and the dirty set are exact; leaves as in check_refresh
    (a cleared leaf is exactly 0)."""
    fa = np.asarray(flags_after, dtype=np.uint8)
    assert fa.shape == ref.flags.shape
    bad = np.flatnonzero(fa != ref.flags)
    assert bad.size == 0, f"flags {bad[:8]}: {fa[bad[:8]]} vs {ref.flags[bad[:8]]}"
    assert int(n_valid_delta) == ref.n_valid, f"n_valid moved by {int(n_valid_delta)}, oracle {ref.n_valid}"
    err = _check_leaves(leaves_before, leaves_after, ref.leaves, ref.touched, T)
    _check_dirty(dirty, count, count0 + ref.count, ref.touched, max_dirty)
    return err
