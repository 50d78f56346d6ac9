"""The float64 oracle of the replay kernels (pytorch_r2d2_amd/replay_ref.py) against brute-force
loops, an fp32 emulation of the kernel's tree descent against ``check_samples``, and every
``check_*`` against wrong variants (oracle mutations and mutated emulations).

Also holds the case builders the GPU tests (test_replay_oracle_gpu.py) share.

Sampler cases.  d of check_samples is (levels - 1) * 1.76e-5 of the total, and a draw is ambiguous
(d admits a second positive leaf) when it lies within d of a boundary between two positive leaves,
so the expected ambiguous share is 2 (levels - 1) 1.76e-5 (n_positive - 1) whatever the leaf
values.  Cases are marked sparse where that is below 1.2 %; the test asserts below 2 % on them.
The 5-level case with 300 positive leaves expects 4.2 % and rowedges (1,024 positive leaves) 7 %:
every draw of theirs is still checked against d, but the 2 % assertion cannot cover them."""
import math

import numpy as np
import pytest

from pytorch_r2d2_amd import replay_ref as rr
from pytorch_r2d2_amd.refnum import mix64

f32 = lambda x: float(np.float32(x))   # noqa: E731
ETA = f32(0.9)
SEEDS = (0x9E3779B1 * 3 + 12345, 0xD1B54A32D192ED03)
CTRS = (0, 3, 2 ** 33)


# ------------------------------------------------------------------ sampler cases
def _leaves(cap, positive, seed, lo=0.1, hi=1.0):
    """fp32 leaves: (lo, hi] at ``positive`` (indices, or None for all), 0 elsewhere."""
    g = np.random.default_rng(seed)
    v = (hi - (hi - lo) * g.random(cap)).astype(np.float32)
    if positive is None:
        return v
    out = np.zeros(cap, dtype=np.float32)
    positive = np.asarray(positive, dtype=np.int64)
    out[positive] = v[positive]
    return out


def _pick(cap, n, seed, also=()):
    g = np.random.default_rng(seed)
    return np.unique(np.concatenate([g.choice(cap, size=n, replace=False),
                                     np.asarray(also, dtype=np.int64)]))


def _range_case():
    v = np.zeros(4097, dtype=np.float32)
    v[_pick(4000, 50, 21) + 40] = 1e-3
    v[17] = 1e4
    v[4096] = 3.0
    return v


def _rowedges():
    lanes = np.asarray([0, 15, 16, 31, 32, 47, 48, 63])
    return _leaves(8192, (np.arange(128)[:, None] * 64 + lanes[None, :]).reshape(-1), 22)


def _single(cap, i):
    v = np.zeros(cap, dtype=np.float32)
    v[i] = 0.625
    return v


def sampler_cases():
    """name -> dict(leaves, Bs, sparse)."""
    c = {}
    c["cap64_5pos"] = dict(leaves=_leaves(64, [3, 15, 16, 40, 63], 11), Bs=(256,), sparse=True)
    c["cap65"] = dict(leaves=_leaves(65, None, 12), Bs=(512,), sparse=True)
    c["cap4096"] = dict(leaves=_leaves(4096, _pick(4096, 100, 13, also=(0, 4095)), 13), Bs=(1024,),
                        sparse=True)
    c["cap4097"] = dict(leaves=_leaves(4097, _pick(4097, 100, 14, also=(4096,)), 14), Bs=(1024,),
                        sparse=True)
    c["cap262145_300pos"] = dict(leaves=_leaves(262145, _pick(262145, 299, 15, also=(262144,)), 15),
                                 Bs=(2048,), sparse=False)
    c["dense5000"] = dict(leaves=_leaves(5000, None, 16), Bs=(8, 64), sparse=False)
    c["rowedges"] = dict(leaves=_rowedges(), Bs=(2048,), sparse=False)
    c["range"] = dict(leaves=_range_case(), Bs=(2048,), sparse=True)
    c["single_first"] = dict(leaves=_single(4097, 0), Bs=(256,), sparse=True)
    c["single_last"] = dict(leaves=_single(4097, 4096), Bs=(256,), sparse=True)
    for name, v in c.items():
        v["name"] = name
        v["cap"] = v["leaves"].size
        v["offs"], v["sizes"] = rr.tree_geometry(v["cap"])
        v["levels"] = len(v["sizes"])
    return c


SAMPLER_CASES = sampler_cases()


# ------------------------------------------------------------------ fp32 emulation of the kernel
def wave_sum_x(x):
    """common.h wave_sum_x over the last axis (64 fp32 values): pairwise inside every 16-lane
    row (xor 1, xor 2, the other quad, the other half), then (r0 + r1) + (r2 + r3)."""
    x = np.asarray(x, dtype=np.float32)
    while x.shape[-1] > 1:
        x = (x[..., 0::2] + x[..., 1::2]).astype(np.float32)
    return x[..., 0]


def build_tree32(leaves, offs, sizes):
    """The fp32 tree r2_tree_rebuild leaves behind."""
    tree = np.zeros(offs[-1] + sizes[-1], dtype=np.float32)
    tree[: sizes[0]] = leaves
    for l in range(1, len(sizes)):
        child = np.zeros(sizes[l] * 64, dtype=np.float32)
        child[: sizes[l - 1]] = tree[offs[l - 1]: offs[l - 1] + sizes[l - 1]]
        tree[offs[l]: offs[l] + sizes[l]] = wave_sum_x(child.reshape(sizes[l], 64))
    return tree


def wave_incl_scan(v, mutation=None):
    """replay.hip wave_incl_scan on (n, 64) fp32: row_shr 1, 2, 4, 8 inside the 16-lane rows
    (lanes shifted in from outside read 0), row_bcast:15 into rows 1 and 3, row_bcast:31 into
    rows 2 and 3."""
    v = np.asarray(v, dtype=np.float32).reshape(-1, 4, 16).copy()
    for n in (1, 2, 4, 8):
        sh = np.zeros_like(v)
        sh[..., n:] = v[..., :-n]
        v = (v + sh).astype(np.float32)
    c0, c2 = v[:, 0, 15].copy(), v[:, 2, 15].copy()
    v[:, 1, :] += c0[:, None]
    v[:, 3, :] += c2[:, None]
    if mutation != "no_bcast31":
        c1 = v[:, 1, 15].copy()
        v[:, 2, :] += c1[:, None]
        v[:, 3, :] += c1[:, None]
    return v.reshape(-1, 64)


def descend32(tree, offs, sizes, B, seed, ctr, mutation=None):
    """replay.hip tree_descend for b < B in fp32, operation by operation.  Returns (idx, prob).
    mutation: 'no_bcast31' (the scan loses its second row carry), 'ge' (incl >= u in the ballot),
    'no_vpos' (no v > 0 test, in the ballot and in the fallback)."""
    F = np.float32
    levels = len(sizes)
    total = F(tree[offs[levels - 1]])
    b = np.arange(B)
    u = ((b.astype(F) + rr.uniform(seed, ctr, b)).astype(F) / F(B)).astype(F) * total
    u = u.astype(F)
    node = np.zeros(B, dtype=np.int64)
    leaf = np.zeros(B, dtype=F)
    lane = np.arange(64)
    for lvl in range(levels - 1, 0, -1):
        c = node[:, None] * 64 + lane[None, :]
        ok = c < sizes[lvl - 1]
        v = np.where(ok, tree[offs[lvl - 1] + np.where(ok, c, 0)], F(0)).astype(F)
        incl = wave_incl_scan(v, mutation)
        excl = (incl - v).astype(F)
        pos = np.ones_like(v, dtype=bool) if mutation == "no_vpos" else v > 0
        over = incl >= u[:, None] if mutation == "ge" else incl > u[:, None]
        hit = over & pos
        first = hit.argmax(axis=1)
        last_nz = np.where(pos.any(axis=1), 63 - pos[:, ::-1].argmax(axis=1), 0)
        pick = np.where(hit.any(axis=1), first, last_nz)
        ex = excl[b, pick]
        pv = v[b, pick]
        u = np.minimum(np.maximum((u - ex).astype(F), F(0)), (pv * F(0.99999)).astype(F)).astype(F)
        node = node * 64 + pick
        leaf = pv
    with np.errstate(divide="ignore", invalid="ignore"):
        prob = np.where(total > 0, (leaf / total).astype(F), F(0)).astype(F)
    return node, prob


_TREES = {}


def tree32(case):
    if case["name"] not in _TREES:
        _TREES[case["name"]] = build_tree32(case["leaves"], case["offs"], case["sizes"])
    return _TREES[case["name"]]


def emulate(case, B, seed, ctr, mutation=None):
    t = tree32(case)
    return descend32(t, case["offs"], case["sizes"], B, seed, ctr, mutation) + (t[case["offs"][-1]],)


# ------------------------------------------------------------------ refresh / edit cases
TUPD = [(80, 40, 80), (80, 0, 80), (20, 10, 20), (64, 0, 64), (129, 1, 129), (1, 0, 1)]
GEOMS = [(5, 1000), (3, 96), (3, 257)]
FLAG_KINDS = ("every40", "all", "none", "one")


def hand_starts(n_sub, cap_e, T):
    """Sampled starts placed by hand: sub-ring positions 0, 1, cap_e - 1, cap_e - T + 1 and a
    middle one, in the first, a middle and the last sub-ring; the middle start of the first
    sub-ring twice; a start T // 2 + 1 rows after it (overlapping windows)."""
    mid = cap_e // 2
    pos = [0, 1, cap_e - 1, (cap_e - T + 1) % cap_e, mid]
    out = [sub * cap_e + p for sub in sorted({0, n_sub // 2, n_sub - 1}) for p in pos]
    out += [mid, (mid + T // 2 + 1) % cap_e]
    return np.asarray(out, dtype=np.int32)


def make_priority(cap, seed):
    """fp32 priorities over six decades, about 10 % exact zeros."""
    g = np.random.default_rng(seed)
    p = (10.0 ** (-3.0 + 6.0 * g.random(cap))).astype(np.float32)
    p[g.random(cap) < 0.1] = 0.0
    return p


def make_flags(cap, kind):
    f = np.zeros(cap, dtype=np.uint8)
    if kind == "every40":
        f[::40] = 1
    elif kind == "all":
        f[:] = 1
    elif kind == "one":
        f[cap // 2] = 1      # position cap_e / 2 of a sub-ring: the middle start itself
    return f


def make_refresh_case(n_sub, cap_e, T, upd_lo, upd_hi, kind, seed=0):
    cap = n_sub * cap_e
    pr = make_priority(cap, 100 + seed + T)
    pr[2 % cap_e] = 5e3      # the maximum of the window of start cap_e - 1 sits in its wrapped part
    g = np.random.default_rng(200 + seed)
    flags = make_flags(cap, kind)
    # stale leaves: something at every flagged row and at a tenth of the others
    leaves = np.where((flags != 0) | (g.random(cap) < 0.1), g.random(cap) + 0.5, 0.0).astype(np.float32)
    return dict(n_sub=n_sub, cap_e=cap_e, cap=cap, T=T, upd_lo=upd_lo, upd_hi=upd_hi, kind=kind,
                starts=hand_starts(n_sub, cap_e, T), flags=flags, priority=pr, leaves=leaves)


def refresh_of(c, mutation=None):
    return rr.refresh_ref(c["starts"], c["flags"], c["priority"], c["leaves"], c["T"], c["upd_lo"],
                          c["upd_hi"], c["cap_e"], ETA, mutation)


EDIT_T = (20, 80, 129)
EDIT_SUB, EDIT_CAP_E = 3, 300


def make_edit_case(T, seed=0):
    """A 3 x 300 replay for mark_starts / apply_pending.  Flags: every 7th row set.  Leaves: a
    stale value at flagged rows (0 at the rows of ``set_zero_leaf``) and at ``stale``."""
    cap_e, cap = EDIT_CAP_E, EDIT_SUB * EDIT_CAP_E
    g = np.random.default_rng(300 + seed + T)
    flags = np.zeros(cap, dtype=np.uint8)
    flags[::7] = 1
    pr = make_priority(cap, 400 + seed + T)
    leaves = np.where(flags != 0, g.random(cap) + 0.5, 0.0).astype(np.float32)
    word = [400, 401, 402, 403]                      # one flag word, none set (400 % 7 = 1)
    split = [408, 411]                               # a word whose other two bytes stay: 409 0, 410 1
    flags[409], flags[410] = 0, 1
    leaves[409], leaves[410] = 0.0, 0.75
    flagged = [7, 14, 301 - 301 % 7 + 7]             # already set
    wrap = [cap_e - 1, 2 * cap_e - 3, cap - 2]       # windows that wrap (T >= 20)
    assert all(flags[r] for r in flagged) and not any(flags[r] for r in word + split + wrap)
    stale = [500, 503]                               # unset flag, non-zero leaf
    flags[stale] = 0
    leaves[stale] = 0.3
    set_zero_leaf = [21, 28]                         # set flag, leaf 0
    leaves[set_zero_leaf] = 0.0
    marks = word + split + flagged + wrap
    return dict(T=T, cap=cap, cap_e=cap_e, flags=flags, priority=pr, leaves=leaves, marks=marks,
                stale=stale, set_zero_leaf=set_zero_leaf)


def mark_rows(c):
    """rows of a mark_starts launch: the marks with -1 entries between them."""
    rows = []
    for i, r in enumerate(c["marks"]):
        rows.append(r)
        if i % 3 == 1:
            rows.append(-1)
    return np.asarray(rows, dtype=np.int32)


def pending_list(c):
    """Marks and clears in one list; a row appears with one sign only.  Duplicates: a mark, the
    clear of an unset flag with a zero leaf, and the clear of a set flag whose leaf is already 0
    (either order of the two gives one append)."""
    f, lv = c["flags"], c["leaves"]
    clear_set = [35, 42, 406]            # set flags with a leaf (406: beside the word 400..403)
    assert all(f[r] for r in clear_set[:2])
    c["flags"][406], c["leaves"][406] = 1, 0.6
    clear_unset_zero = [5, 9, 409]       # unset flag, zero leaf: no append (409 shares 408's word)
    assert not any(f[r] or lv[r] for r in clear_unset_zero)
    z = c["set_zero_leaf"]
    e = list(c["marks"]) + [c["marks"][0]]
    e += [-2 - r for r in clear_set + c["stale"] + clear_unset_zero + z + [z[0], clear_unset_zero[0]]]
    order = np.random.default_rng(7).permutation(len(e))
    return np.asarray(e, dtype=np.int32)[order]


# ================================================================== tests
def _py_mix64(z):
    m = (1 << 64) - 1
    z = (z + 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


def _py_uniform(seed, ctr, idx):
    m = (1 << 64) - 1
    z = _py_mix64((seed & m) ^ _py_mix64((ctr * 0x100000001B3 + idx) & m))
    return (z >> 40) / 16777216.0


def test_uniform_matches_python_ints_and_stays_in_range():
    for seed in SEEDS + (0, 1, (1 << 64) - 1):
        for ctr in CTRS + (2 ** 63 - 1,):
            got = rr.uniform(seed, ctr, np.arange(4096))
            assert got.dtype == np.float32 and got.shape == (4096,)
            assert (got >= 0).all() and (got < 1).all()
            for i in (0, 1, 2, 63, 64, 1000, 4095):
                assert float(got[i]) == _py_uniform(seed, ctr, i), (seed, ctr, i)
    a, b, c = (rr.uniform(SEEDS[0], k, np.arange(256)) for k in (0, 3, 2 ** 33))
    assert (a != b).mean() > 0.99 and (a != c).mean() > 0.99 and (b != c).mean() > 0.99
    # a counter truncated to 32 bits would repeat step 0 at step 2^32 and 2^33
    assert (rr.uniform(SEEDS[0], 2 ** 33, np.arange(256)) != rr.uniform(SEEDS[0], 0, np.arange(256))).any()
    # the finaliser itself, pinned (splitmix64's first output for state 0)
    assert int(mix64(0)[0]) == 0xE220A8397B1DCDAF == _py_mix64(0)


def test_tree_geometry_is_the_replay_s():
    from pytorch_r2d2_amd.engine.replay_hbm import tree_geometry
    for cap in (1, 2, 64, 65, 4096, 4097, 5000, 262144, 262145, 999936):
        assert rr.tree_geometry(cap) == tree_geometry(cap)
    assert [c["levels"] for c in SAMPLER_CASES.values()] == [2, 3, 3, 4, 5, 4, 4, 4, 4, 4]


def test_ring_row_stays_in_its_subring():
    cap_e = 257
    for start in (0, 1, 256, 257, 3 * 257 - 1, 2 * 257 + 100):
        t = np.arange(-3 * cap_e - 5, 3 * cap_e + 5)
        r = rr.ring_row(start, t, cap_e)
        base = start - start % cap_e
        assert ((r >= base) & (r < base + cap_e)).all()
        assert ((r - start - t) % cap_e == 0).all()
    assert int(rr.ring_row(257, -1, 257)) == 513 and int(rr.ring_row(513, 1, 257)) == 257


def _brute_refresh(c):
    """Every flagged row of the replay against every sampled start: window overlap with the
    physical rows the learner rewrote, row by row."""
    T, lo, hi, cap_e = c["T"], c["upd_lo"], c["upd_hi"], c["cap_e"]
    eta = float(np.float32(ETA))
    pr = [float(x) for x in c["priority"]]
    new = [float(x) for x in c["leaves"]]
    touched, count = set(), 0
    upd = []
    for sb in (int(s) for s in c["starts"]):
        base = sb - sb % cap_e
        upd.append((base, [(sb - base + j) % cap_e for j in range(lo, hi)]))
    for s in np.flatnonzero(c["flags"]):
        s = int(s)
        base = s - s % cap_e
        win = [(s - base + t) % cap_e for t in range(T)]
        at = {}
        for t, w in enumerate(win):
            at.setdefault(w, []).append(t)
        for ubase, rows in upd:
            if ubase != base:
                continue
            # every (updated row, window row) coincidence is one offset k = j - t: one listing
            # per distinct k
            ks = set()
            for j, r in zip(range(lo, hi), rows):
                for t in at.get(r, ()):
                    ks.add(j - t)
            if ks:
                touched.add(s)
                count += len(ks)
        if s in touched:
            w = [pr[base + o] for o in win]
            new[s] = eta * max(w) + (1.0 - eta) * (math.fsum(w) / T)
    return np.asarray(new), sorted(touched), count


@pytest.mark.parametrize("geom", GEOMS)
@pytest.mark.parametrize("tupd", [TUPD[0], TUPD[4], TUPD[5]])
def test_refresh_ref_matches_brute_force(geom, tupd):
    for kind in ("every40", "all"):
        c = make_refresh_case(*geom, *tupd, kind)
        ref = refresh_of(c)
        new, touched, count = _brute_refresh(c)
        assert ref.touched.tolist() == touched
        assert ref.count == count
        np.testing.assert_allclose(ref.leaves, new, rtol=1e-14, atol=0)
        assert len(touched) > 0


def test_refresh_cases_cover_what_they_claim():
    c = make_refresh_case(5, 1000, 80, 40, 80, "all")
    s = c["starts"].tolist()
    assert len(s) != len(set(s))                                   # one start twice
    assert {x // 1000 for x in s} == {0, 2, 4}
    w = c["priority"][rr.ring_row(999, np.arange(80), 1000)]
    assert int(w.argmax()) == 3                                    # the maximum, after the wrap
    assert 0.05 < (c["priority"] == 0).mean() < 0.15
    # cap_e shorter than the candidate range: duplicates inside one workgroup
    c = make_refresh_case(3, 96, 129, 1, 129, "all")
    r = refresh_of(c)
    assert r.count == len(c["starts"]) * 256 and r.touched.size == 3 * 96


def _py_edit(entries, c, pending):
    f = [int(x) for x in c["flags"]]
    lv = [float(x) for x in c["leaves"]]
    pr = [float(x) for x in c["priority"]]
    T, cap_e, eta = c["T"], c["cap_e"], float(np.float32(ETA))
    nv, cnt, touched = 0, 0, set()
    for e in (int(x) for x in entries):
        if e >= 0:
            base = e - e % cap_e
            w = [pr[base + (e - base + t) % cap_e] for t in range(T)]
            nv += 1 - f[e]
            f[e] = 1
            lv[e] = eta * max(w) + (1.0 - eta) * (math.fsum(w) / T)
            cnt += 1
            touched.add(e)
        elif pending and e != -1:
            r = -2 - e
            if f[r] or lv[r] != 0.0:
                cnt += 1
                touched.add(r)
            nv -= f[r]
            f[r], lv[r] = 0, 0.0
    return f, lv, sorted(touched), nv, cnt


@pytest.mark.parametrize("T", EDIT_T)
def test_mark_and_pending_refs_match_a_python_loop(T):
    c = make_edit_case(T)
    rows = mark_rows(c)
    assert (rows == -1).sum() >= 3
    for n_rows in (None, len(rows) - 4, len(rows) + 9):
        n = len(rows) if n_rows is None else min(n_rows, len(rows))
        ref = rr.mark_starts_ref(rows, n_rows, len(rows), c["flags"], c["priority"], c["leaves"], T,
                                 c["cap_e"], ETA)
        f, lv, touched, nv, cnt = _py_edit(rows[:n], c, False)
        assert ref.flags.tolist() == f and ref.touched.tolist() == touched
        assert (ref.n_valid, ref.count, ref.err) == (nv, cnt, 0)
        np.testing.assert_allclose(ref.leaves, lv, rtol=1e-14, atol=0)
    assert ref.n_valid == len(c["marks"]) - 3        # three of the marks were set already
    c = make_edit_case(T)
    pend = pending_list(c)
    for cnt_d, cap_p in ((len(pend), len(pend) + 3), (len(pend) + 5, len(pend) - 3)):
        ref = rr.apply_pending_ref(pend, cnt_d, cap_p, c["flags"], c["priority"], c["leaves"], T,
                                   c["cap_e"], ETA)
        f, lv, touched, nv, cnt = _py_edit(pend[: min(cnt_d, cap_p)], c, True)
        assert ref.flags.tolist() == f and ref.touched.tolist() == touched
        assert (ref.n_valid, ref.count) == (nv, cnt)
        assert ref.err == (2 if cnt_d > cap_p else 0)
        np.testing.assert_allclose(ref.leaves, lv, rtol=1e-14, atol=0)
    # the bytes beside edited ones: 409 / 410 keep 0 / 1 while 408 and 411 are marked
    assert c["flags"][408:412].tolist() == [0, 0, 1, 0]


def test_check_tree_accepts_the_fp32_tree_and_rejects_wrong_ones():
    for name in ("cap65", "cap4097", "dense5000", "range"):
        c = SAMPLER_CASES[name]
        t = tree32(c)
        assert rr.check_tree(t, c["offs"], c["sizes"], c["leaves"]) <= 6 * rr.U24
        bad = t.copy()
        bad[c["offs"][1]] *= np.float32(1 + 2e-6)
        with pytest.raises(AssertionError):
            rr.check_tree(bad, c["offs"], c["sizes"])
    # a parent that also summed the slot past its level's size (the next level's first node)
    c = SAMPLER_CASES["cap65"]
    bad = tree32(c).copy()
    bad[c["offs"][1] + 1] += bad[c["offs"][1]]
    with pytest.raises(AssertionError):
        rr.check_tree(bad, c["offs"], c["sizes"])


def _all_draws(case):
    for B in case["Bs"]:
        for seed in SEEDS:
            for ctr in CTRS:
                yield B, seed, ctr


@pytest.mark.parametrize("name", list(SAMPLER_CASES))
def test_fp32_descent_emulation_passes_check_samples(name):
    c = SAMPLER_CASES[name]
    rr.check_tree(tree32(c), c["offs"], c["sizes"], c["leaves"])
    d_rel = rr.sample_tolerance(c["levels"])
    assert 1.7e-5 < d_rel < 7.2e-5
    for B, seed, ctr in _all_draws(c):
        idx, prob, root = emulate(c, B, seed, ctr)
        rep = rr.check_samples(c["leaves"], c["levels"], B, seed, ctr, idx, prob, root)
        assert rep.miss <= d_rel
        if c["sparse"]:
            assert rep.ambiguous < 0.02, (name, B, seed, ctr, rep)
            # where d admits one leaf only, that leaf is the float64 sampler's
            ref_idx, _ = rr.sample_ref(c["leaves"], B, seed, ctr)
            assert (idx != ref_idx).mean() <= rep.ambiguous
    a = emulate(c, c["Bs"][0], SEEDS[0], 0)[0]
    assert np.array_equal(a, emulate(c, c["Bs"][0], SEEDS[0], 0)[0])


def test_sample_ref_passes_and_its_mutation_is_rejected():
    rejected = 0
    for name, c in SAMPLER_CASES.items():
        B = c["Bs"][-1]
        idx, prob = rr.sample_ref(c["leaves"], B, SEEDS[0], 3)
        rr.check_samples(c["leaves"], c["levels"], B, SEEDS[0], 3, idx, prob)
        idx, prob = rr.sample_ref(c["leaves"], B, SEEDS[0], 3, "next_leaf")
        try:
            rr.check_samples(c["leaves"], c["levels"], B, SEEDS[0], 3, idx, prob)
        except AssertionError:
            rejected += 1
    # every case with two positive leaves or more
    assert rejected == len(SAMPLER_CASES) - 2


def _rejects(mutation):
    """Names of the sampler cases on which check_samples rejects the mutated emulation."""
    out = []
    for name, c in SAMPLER_CASES.items():
        for B, seed, ctr in _all_draws(c):
            idx, prob, root = emulate(c, B, seed, ctr, mutation)
            try:
                rr.check_samples(c["leaves"], c["levels"], B, seed, ctr, idx, prob, root)
            except AssertionError:
                out.append(name)
                break
    return out


def test_scan_without_row_carry_is_rejected():
    bad = _rejects("no_bcast31")
    assert "rowedges" in bad and "dense5000" in bad and "cap65" in bad, bad


def test_descent_without_v_positive_test_is_rejected_on_a_tree_without_mass():
    """With the v > 0 tests gone the fallback takes lane 63 at every level.  Where the tree has
    mass the ballot finds a positive child first (an inclusive sum only exceeds u at a lane that
    added something), so the case that shows it is the all-zero tree: the index leaves the
    capacity."""
    c = SAMPLER_CASES["cap65"]
    zero = np.zeros(c["offs"][-1] + 1, dtype=np.float32)
    idx, prob = descend32(zero, c["offs"], c["sizes"], 64, SEEDS[0], 0)
    assert ((idx >= 0) & (idx < c["cap"])).all() and (prob == 0).all()
    idx, prob = descend32(zero, c["offs"], c["sizes"], 64, SEEDS[0], 0, "no_vpos")
    assert (idx >= c["cap"]).all()


def test_ge_ballot_only_moves_draws_that_sit_on_a_boundary():
    """``incl >= u`` for ``incl > u`` differs only where u equals an inclusive sum exactly: the
    draw then sits on the boundary of two leaves and both hold it, so no check of a draw against
    the CDF can tell the two apart, at any tolerance.  What can be shown: the variant's draws
    differ from the kernel's rule only by such ties, all of them inside d."""
    for name, c in SAMPLER_CASES.items():
        for B, seed, ctr in _all_draws(c):
            a, _, root = emulate(c, B, seed, ctr)
            g, pg, _ = emulate(c, B, seed, ctr, "ge")
            rr.check_samples(c["leaves"], c["levels"], B, seed, ctr, g, pg, root)
            if name != "range":     # fp32's grid at 1e4 is as coarse as the 1e-3 leaves: ties occur
                assert np.array_equal(a, g), name


def _fake_launch(ref, leaves, n_guard=4):
    """What a correct fp32 kernel would leave behind for an oracle result: rounded leaves with
    guard elements, one dirty entry per touched row padded up to the count."""
    before = np.concatenate([leaves, np.full(n_guard, np.nan, dtype=np.float32)])
    after = before.copy()
    after[ref.touched] = ref.leaves[ref.touched].astype(np.float32)
    dirty = np.full(max(ref.count, 1) + n_guard, -1, dtype=np.int32)
    t = ref.touched
    if t.size:
        dirty[: ref.count] = np.resize(t, ref.count)
    return before, after, dirty


REFRESH_MUT_CASES = [make_refresh_case(5, 1000, 80, 40, 80, "all"),
                     make_refresh_case(5, 1000, 80, 40, 80, "every40"),
                     make_refresh_case(3, 257, 129, 1, 129, "every40"),
                     make_refresh_case(5, 1000, 20, 10, 20, "all")]


def test_check_refresh_accepts_the_oracle():
    for c in REFRESH_MUT_CASES:
        ref = refresh_of(c)
        before, after, dirty = _fake_launch(ref, c["leaves"])
        assert rr.check_refresh(ref, before, after, dirty, ref.count, dirty.size - 4, c["T"]) <= rr.U24
        # a write past max_dirty, a lost touched leaf, a moved untouched leaf
        with pytest.raises(AssertionError):
            rr.check_refresh(ref, before, after, dirty, ref.count, ref.count - 2, c["T"])
        lost = after.copy()
        lost[ref.touched[0]] = before[ref.touched[0]]
        with pytest.raises(AssertionError):
            rr.check_refresh(ref, before, lost, dirty, ref.count, dirty.size - 4, c["T"])
        moved = after.copy()
        moved[-1] = 0.0
        with pytest.raises(AssertionError):
            rr.check_refresh(ref, before, moved, dirty, ref.count, dirty.size - 4, c["T"])


@pytest.mark.parametrize("mutation", rr.MUTATIONS[:7])
def test_check_refresh_rejects_mutated_oracles(mutation):
    rejected = 0
    for c in REFRESH_MUT_CASES:
        good = refresh_of(c)
        before, after, dirty = _fake_launch(good, c["leaves"])
        try:
            rr.check_refresh(refresh_of(c, mutation), before, after, dirty, good.count, dirty.size - 4,
                             c["T"])
        except AssertionError:
            rejected += 1
    assert rejected >= 1, mutation
    if mutation not in ("mean_64",):
        assert rejected >= 2, mutation


@pytest.mark.parametrize("mutation", ("n_valid_per_entry", "mean_only", "window_no_wrap"))
def test_check_edit_rejects_mutated_oracles(mutation):
    for pending in (False, True):
        c = make_edit_case(80)
        if pending:
            e = pending_list(c)
            fn = lambda m: rr.apply_pending_ref(e, len(e), len(e), c["flags"], c["priority"],   # noqa: E731
                                                c["leaves"], 80, c["cap_e"], ETA, m)
        else:
            e = mark_rows(c)
            fn = lambda m: rr.mark_starts_ref(e, None, len(e), c["flags"], c["priority"],        # noqa: E731
                                              c["leaves"], 80, c["cap_e"], ETA, m)
        good = fn(None)
        before, after, dirty = _fake_launch(good, c["leaves"], 0)
        dirty = np.concatenate([dirty, np.full(4, -1, dtype=np.int32)])
        args = (good.flags, before, after, good.n_valid, dirty, good.count, dirty.size - 4, 80)
        assert rr.check_edit(good, *args) <= rr.U24
        with pytest.raises(AssertionError):
            rr.check_edit(fn(mutation), *args)
        flipped = good.flags.copy()
        flipped[409] ^= 1
        with pytest.raises(AssertionError):
            rr.check_edit(good, flipped, *args[1:])


def test_every_mutation_has_a_rejection_test():
    covered = set(rr.MUTATIONS[:7]) | {"next_leaf", "n_valid_per_entry"}
    assert covered == set(rr.MUTATIONS)
