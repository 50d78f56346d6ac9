"""Every entry point of the replay sampling and priority kernels (csrc/kernels/replay.hip)
against the float64 oracle (pytorch_r2d2_amd/replay_ref.py), on trees of a few thousand leaves.

The launches go through the ctypes entry points on the test's own tensors.  Every buffer a kernel
writes sits between two runs of 16 guard elements and starts poisoned (NaN floats, -1 ints, 0xAB
flag bytes); the guards must keep their bits.  The bounds are the oracle's (its module
docstring); the cases and their builders live in test_replay_ref_cpu.py, which also shows on the
CPU that the checks reject wrong kernels.

With R2D2_REPLAY_ORACLE_REPORT=<file> the measured figures are written there
(profiles/replay_oracle_errors.txt)."""
import numpy as np
import pytest
import torch

from gpu_support import DEV, G, NAN, Buf, Tree, i64, report_fixture, word
from gpu_support import stop_after_a_gpu_error  # noqa: F401
from pytorch_r2d2_amd import replay_ref as rr
from pytorch_r2d2_amd.ops._lib import kernels, stream_handle
from test_replay_ref_cpu import (CTRS, EDIT_T, ETA, GEOMS, SAMPLER_CASES, SEEDS, TUPD, FLAG_KINDS,
                                 _leaves, make_edit_case, make_refresh_case, mark_rows, pending_list,
                                 refresh_of)

pytestmark = pytest.mark.gpu

_REPORT, _report = report_fixture(
    "R2D2_REPLAY_ORACLE_REPORT",
    "# replay.hip against replay_ref.py, one line per case\n"
    "# sample : largest miss (distance from the float64 draw point to the returned\n"
    "#          leaf's mass interval / total; the bound is d), share of draws for which\n"
    "#          d admits a second leaf, draws that differ from the float64 sampler\n"
    "# refresh / mark / pending : largest relative leaf error in units of 2^-24, and\n"
    "#          the bound in the same units\n")


_TREES = {}


def case_tree(name):
    if name not in _TREES:
        _TREES[name] = Tree(SAMPLER_CASES[name]["leaves"])
        _TREES[name].check(SAMPLER_CASES[name]["leaves"])
    return _TREES[name]


# ================================================================== sampler
@pytest.mark.parametrize("name", list(SAMPLER_CASES))
def test_tree_sample_draws_against_the_cdf(name):
    c = SAMPLER_CASES[name]
    tree = case_tree(name)
    k = kernels()
    runs = []
    for B in c["Bs"]:
        for seed in SEEDS:
            for ctr in CTRS:
                step = word(ctr, torch.int64)
                idx, prob = Buf.poisoned(B, torch.int32, -1), Buf.poisoned(B, torch.float32, NAN)
                assert k.r2_tree_sample(*tree.geom(), B, seed, step.data_ptr(), idx.p, prob.p,
                                        stream_handle()) == 0
                runs.append((B, seed, ctr, idx, prob, step))
    # the same launch again, and one without a step counter (counter 0)
    B0 = c["Bs"][0]
    again = (Buf.poisoned(B0, torch.int32, -1), Buf.poisoned(B0, torch.float32, NAN))
    nostep = (Buf.poisoned(B0, torch.int32, -1), Buf.poisoned(B0, torch.float32, NAN))
    assert k.r2_tree_sample(*tree.geom(), B0, SEEDS[0], runs[0][5].data_ptr(), again[0].p, again[1].p,
                            stream_handle()) == 0
    assert k.r2_tree_sample(*tree.geom(), B0, SEEDS[0], 0, nostep[0].p, nostep[1].p,
                            stream_handle()) == 0
    torch.cuda.synchronize()
    tree.buf.assert_untouched("tree")
    root = tree.root()
    worst, amb, diff, first = 0.0, 0.0, 0, {}
    for B, seed, ctr, idx, prob, _ in runs:
        idx.assert_guards("idx")
        prob.assert_guards("prob")
        rep = rr.check_samples(c["leaves"], c["levels"], B, seed, ctr, idx.body(), prob.body(), root)
        if c["sparse"]:
            assert rep.ambiguous < 0.02
        ref_idx, _ = rr.sample_ref(c["leaves"], B, seed, ctr)
        diff += int((idx.body() != ref_idx).sum())
        worst, amb = max(worst, rep.miss), max(amb, rep.ambiguous)
        first.setdefault((B, seed), []).append(idx.body())
    _REPORT.append("sample  %-18s levels %d  miss %.3e (d %.3e)  ambiguous %.4f  differ %d" %
                   (name, c["levels"], worst, rr.sample_tolerance(c["levels"]), amb, diff))
    assert np.array_equal(again[0].body(), runs[0][3].body())
    assert np.array_equal(again[1].bits(), runs[0][4].bits())
    assert np.array_equal(nostep[0].body(), runs[0][3].body())          # runs[0] is counter 0
    if (c["leaves"] > 0).sum() >= 60:
        # another counter, other draws (2^33 is not 0 either); with fewer leaves nearly every
        # stratum lies inside one leaf and the rows do not depend on the draw
        for per_ctr in first.values():
            assert not np.array_equal(per_ctr[0], per_ctr[1])
            assert not np.array_equal(per_ctr[0], per_ctr[2])
            assert not np.array_equal(per_ctr[1], per_ctr[2])


@pytest.mark.parametrize("cap", [65, 4097])
def test_tree_without_mass_gives_rows_in_range_and_probability_zero(cap):
    tree = Tree(np.zeros(cap, dtype=np.float32))
    assert tree.root() == 0.0
    B = 64
    idx, prob = Buf.poisoned(B, torch.int32, -1), Buf.poisoned(B, torch.float32, NAN)
    step = word(3, torch.int64)
    assert kernels().r2_tree_sample(*tree.geom(), B, SEEDS[0], step.data_ptr(), idx.p, prob.p,
                                    stream_handle()) == 0
    torch.cuda.synchronize()
    idx.assert_guards()
    prob.assert_guards()
    assert ((idx.body() >= 0) & (idx.body() < cap)).all()
    assert (prob.body() == 0).all()


def _state_setup(cap, H, nstate, h_f32, B, seed=5):
    g = torch.Generator().manual_seed(seed + H)
    src = [torch.randn(cap, 2 * H, generator=g) for _ in range(nstate)]
    dsrc = [s.to(DEV) for s in src]
    h = [Buf.poisoned(B * H, torch.float32 if h_f32 else torch.bfloat16, NAN) for _ in range(nstate)]
    c = [Buf.poisoned(B * H, torch.float32, NAN) for _ in range(nstate)]
    arr = lambda xs: i64(list(xs) + [0])     # noqa: E731
    ptrs = dict(hs=arr(s.data_ptr() for s in dsrc), h=arr(b.p for b in h), c=arr(b.p for b in c))
    return src, dsrc, h, c, ptrs


def _check_rows_and_states(starts, rows, B, Tn, cap_e, offs, src, h, c, H, h_f32, row_off=0):
    starts = np.asarray(starts, dtype=np.int64)
    want = rr.ring_row(starts[None, :], row_off + np.arange(Tn)[:, None], cap_e)
    assert np.array_equal(np.asarray(rows).reshape(Tn, B), want), "row list"
    for j, off in enumerate(offs):
        r = torch.from_numpy(rr.ring_row(starts, off, cap_e))
        hv = src[j][r, :H].contiguous()
        want_h = hv if h_f32 else hv.bfloat16()
        assert np.array_equal(h[j].bits(), Buf._bytes(want_h)), f"h of chain {j}"
        assert np.array_equal(c[j].bits(), Buf._bytes(src[j][r, H:].contiguous())), f"c of chain {j}"
        h[j].assert_guards("h")
        c[j].assert_guards("c")


def _batch_leaves(n_sub, cap_e):
    """About 60 positive leaves, the first and the last two positions of every sub-ring among
    them (row lists and state rows that wrap)."""
    cap = n_sub * cap_e
    edge = [s * cap_e + p for s in range(n_sub) for p in (0, cap_e - 2, cap_e - 1)]
    g = np.random.default_rng(31 + cap)
    return _leaves(cap, np.unique(np.concatenate([g.choice(cap, 45, replace=False), edge])), 32 + cap)


_BATCH_TREES = {}


def batch_tree(n_sub, cap_e):
    if (n_sub, cap_e) not in _BATCH_TREES:
        _BATCH_TREES[(n_sub, cap_e)] = Tree(_batch_leaves(n_sub, cap_e))
    return _BATCH_TREES[(n_sub, cap_e)]


# entry, (n_sub, cap_e), Tn, nstate, H, h_f32, counter
BATCH = [("r2_sample_batch", (5, 1000), 85, 3, 260, 0, 3),
         ("r2_sample_batch", (3, 257), 300, 0, 64, 0, 0),
         ("r2_sample_batch", (3, 257), 1, 1, 64, 0, 2 ** 33),
         ("r2_sample_batch_f32h", (5, 1000), 1, 1, 256, 1, 2 ** 33),
         ("r2_sample_batch_f32h", (3, 257), 300, 3, 260, 1, 3),
         ("r2_sample_batch_q", (5, 1000), 85, 3, 64, 0, 0),
         ("r2_sample_batch_q", (3, 257), 300, 1, 260, 1, 2 ** 33)]


@pytest.mark.parametrize("entry,geom,Tn,nstate,H,h_f32,ctr", BATCH)
def test_sample_batch_draws_rows_and_states(entry, geom, Tn, nstate, H, h_f32, ctr):
    n_sub, cap_e = geom
    tree = batch_tree(*geom)
    cap, B, seed = n_sub * cap_e, 128, SEEDS[1]
    offs = [0, 5, cap_e - 1][:nstate]
    src, dsrc, h, c, ptrs = _state_setup(cap, H, nstate, h_f32, B)
    off = np.asarray(offs + [0], dtype=np.int32)
    starts, probs = Buf.poisoned(B, torch.int32, -1), Buf.poisoned(B, torch.float32, NAN)
    rows = Buf.poisoned(Tn * B, torch.int32, -1)
    step = word(ctr, torch.int64)
    q = Buf(np.full(4, 7, dtype=np.int32), -1)
    args = (*tree.geom(), B, seed, step.data_ptr(), starts.p, probs.p, rows.p, Tn, cap_e, H, nstate,
            ptrs["hs"].ctypes.data, off.ctypes.data, ptrs["h"].ctypes.data, ptrs["c"].ctypes.data)
    if entry == "r2_sample_batch_q":
        rc = kernels().r2_sample_batch_q(*args, h_f32, q.p, stream_handle())
    else:
        rc = getattr(kernels(), entry)(*args, stream_handle())
    assert rc == 0
    torch.cuda.synchronize()
    for b in (starts, probs, rows, q):
        b.assert_guards(entry)
    tree.buf.assert_untouched("tree")
    rep = rr.check_samples(tree.leaves, tree.levels, B, seed, ctr, starts.body(), probs.body(),
                           tree.root())
    _check_rows_and_states(starts.body(), rows.body(), B, Tn, cap_e, offs, src, h, c, H, h_f32)
    assert q.body().tolist() == ([0, 0, 7, 7] if entry == "r2_sample_batch_q" else [7, 7, 7, 7])
    wrapped = (rr.ring_row(starts.body().astype(np.int64), Tn - 1, cap_e) < starts.body()).sum()
    assert Tn == 1 or wrapped > 0, "no sampled window wraps: the case checks nothing at the ring's end"
    _REPORT.append("sample  %-18s levels %d  miss %.3e (d %.3e)  ambiguous %.4f  differ %d" %
                   ("%s/%dx%d" % (entry[3:], n_sub, cap_e), tree.levels, rep.miss,
                    rr.sample_tolerance(tree.levels), rep.ambiguous,
                    int((starts.body() != rr.sample_ref(tree.leaves, B, seed, ctr)[0]).sum())))


@pytest.mark.parametrize("levels", [1, 9])
def test_sampler_refuses_a_tree_depth_it_cannot_hold(levels):
    tree = batch_tree(3, 257)
    offs, sizes = i64(list(tree.offs) + [0] * 9), i64(list(tree.sizes) + [1] * 9)
    geom = (tree.buf.p, offs.ctypes.data, sizes.ctypes.data, levels)
    B, Tn, H = 8, 4, 64
    idx, prob = Buf.poisoned(B, torch.int32, -1), Buf.poisoned(B, torch.float32, NAN)
    rows = Buf.poisoned(Tn * B, torch.int32, -1)
    step = word(0, torch.int64)
    assert kernels().r2_tree_sample(*geom, B, 1, step.data_ptr(), idx.p, prob.p, stream_handle()) == -1
    z = i64([0])
    zi = np.zeros(1, dtype=np.int32)
    for entry in ("r2_sample_batch", "r2_sample_batch_f32h"):
        assert getattr(kernels(), entry)(*geom, B, 1, step.data_ptr(), idx.p, prob.p, rows.p, Tn, 257, H,
                                         0, z.ctypes.data, zi.ctypes.data, z.ctypes.data, z.ctypes.data,
                                         stream_handle()) == -1
    assert kernels().r2_tree_rebuild(*geom, stream_handle()) == -1
    torch.cuda.synchronize()
    for b in (idx, prob, rows):
        b.assert_untouched()
    tree.buf.assert_untouched("tree")


@pytest.mark.parametrize("cap_e,Tn,off", [(1000, 85, 7), (257, 300, 250), (257, 1, 0)])
def test_make_rows_and_gather_state(cap_e, Tn, off):
    n_sub, B, H = 3, 37, 260
    cap = n_sub * cap_e
    g = np.random.default_rng(cap_e + Tn)
    starts = g.integers(0, cap, B).astype(np.int32)
    starts[:4] = [0, cap_e - 1, cap - 1, cap_e]
    ds = torch.from_numpy(starts).to(DEV)
    rows = Buf.poisoned(Tn * B, torch.int32, -1)
    assert kernels().r2_make_rows(ds.data_ptr(), B, Tn, off, cap_e, rows.p, stream_handle()) == 0
    for with_h32 in (False, True):
        src, dsrc, h, c, _ = _state_setup(cap, H, 1, 0, B, seed=Tn)
        h32 = Buf.poisoned(B * H, torch.float32, NAN)
        assert kernels().r2_gather_state(dsrc[0].data_ptr(), ds.data_ptr(), B, off, cap_e, H, h[0].p,
                                         c[0].p, h32.p if with_h32 else 0, stream_handle()) == 0
        torch.cuda.synchronize()
        rows.assert_guards("rows")
        _check_rows_and_states(starts, rows.body(), B, Tn, cap_e, [off], src, h, c, H, 0, row_off=off)
        r = torch.from_numpy(rr.ring_row(starts.astype(np.int64), off, cap_e))
        if with_h32:
            assert np.array_equal(h32.bits(), Buf._bytes(src[0][r, :H].contiguous()))
            h32.assert_guards("h32")
        else:
            h32.assert_untouched("h32")


# ================================================================== refresh
MAX_DIRTY = 8192


class RefreshRun:
    """Device state of one refresh case: the tree over the case's stale leaves, flags, priorities,
    a poisoned dirty list and a zero counter."""

    def __init__(self, c, max_dirty=MAX_DIRTY):
        self.c = c
        self.tree = Tree(c["leaves"])
        self.flags = Buf(c["flags"], 0xAB)
        self.priority = Buf(c["priority"], NAN)
        self.starts = torch.from_numpy(c["starts"]).to(DEV)
        self.dirty = Buf.poisoned(max_dirty, torch.int32, -1)
        self.count = word(0)
        self.max_dirty = max_dirty

    def refresh_args(self, leaves_p, T=None, upd=None):
        c = self.c
        lo, hi = upd if upd else (c["upd_lo"], c["upd_hi"])
        return (self.starts.data_ptr(), len(c["starts"]), self.flags.p, self.priority.p, leaves_p,
                c["T"] if T is None else T, lo, hi, c["cap_e"], ETA, self.dirty.p,
                self.count.data_ptr(), self.max_dirty)

    def check_inputs_kept(self):
        self.flags.assert_untouched("flags")
        self.priority.assert_untouched("priority")


def _refresh_and_check(run, ref, what):
    """r2_seqprio_refresh, the leaf / dirty checks, then r2_tree_update and the tree check."""
    c, tree = run.c, run.tree
    assert kernels().r2_seqprio_refresh(*run.refresh_args(tree.buf.p), stream_handle()) == 0
    torch.cuda.synchronize()
    tree.buf.assert_guards(what)
    run.dirty.assert_guards(what)
    run.check_inputs_kept()
    count = int(run.count.item())
    # the whole tree buffer: nothing but the touched leaves may change (the levels above are
    # repaired by the next launch)
    err = rr.check_refresh(ref, tree.buf.tail(init=True), tree.buf.tail(), run.dirty.tail(), count,
                           run.max_dirty, c["T"])
    assert kernels().r2_tree_update(*tree.geom(), run.dirty.p, run.count.data_ptr(), run.max_dirty,
                                    stream_handle()) == 0
    torch.cuda.synchronize()
    tree.check()
    assert int(run.count.item()) == count
    return err


@pytest.mark.parametrize("geom", GEOMS)
@pytest.mark.parametrize("tupd", TUPD)
def test_seqprio_refresh_against_the_oracle(geom, tupd):
    worst = 0.0
    for kind in FLAG_KINDS:
        c = make_refresh_case(*geom, *tupd, kind)
        ref = refresh_of(c)
        assert (ref.touched.size > 0) == (kind != "none")
        worst = max(worst, _refresh_and_check(RefreshRun(c), ref, f"{geom} {tupd} {kind}"))
    _REPORT.append("refresh %dx%-5d T %3d upd [%d, %d)  leaf error %.2f u (bound %d u)" %
                   (*geom, *tupd, worst / rr.U24, round(rr.leaf_bound(tupd[0]) / rr.U24)))


@pytest.mark.parametrize("tupd", TUPD)
def test_prio_tail_against_the_oracle(tupd):
    """The one-launch tail on the 5 x 1000 replay (4 levels): leaves, dirty list and the repaired
    tree as above; the step counter advances, the dirty counter is reset, the sync words return
    to 0."""
    worst = 0.0
    for kind in FLAG_KINDS:
        c = make_refresh_case(5, 1000, *tupd, kind)
        ref = refresh_of(c)
        run = RefreshRun(c)
        tree = run.tree
        assert tree.levels == 4
        sync = torch.zeros(8, dtype=torch.int32, device=DEV)
        step = word(41, torch.int64)
        a = run.refresh_args(0)
        rc = kernels().r2_prio_tail(*a[:4], *tree.geom(), *a[5:], sync.data_ptr(), step.data_ptr(), 1,
                                    stream_handle())
        assert rc == 0
        torch.cuda.synchronize()
        tree.buf.assert_guards()
        run.dirty.assert_guards()
        run.check_inputs_kept()
        assert sync.tolist() == [0] * 8 and int(step.item()) == 42 and int(run.count.item()) == 0
        n0 = tree.sizes[0]
        before, after = tree.buf.tail(init=True)[:n0], tree.buf.tail()[:n0]
        worst = max(worst, rr.check_refresh(ref, before, after, run.dirty.tail(), ref.count,
                                            run.max_dirty, c["T"]))
        tree.check()
    _REPORT.append("tail    5x1000  T %3d upd [%d, %d)  leaf error %.2f u (bound %d u)" %
                   (*tupd, worst / rr.U24, round(rr.leaf_bound(tupd[0]) / rr.U24)))


def test_refresh_with_a_candidate_list_just_inside_its_limit():
    """T = 1024 over [0, 1024): 2,047 candidates per workgroup, every one flagged; T = 1025 over
    [0, 1025) is refused and changes nothing."""
    c = make_refresh_case(2, 1500, 1024, 0, 1024, "all")
    c["starts"] = np.asarray([10, 1500 + 700], dtype=np.int32)
    ref = refresh_of(c)
    assert ref.count == 2 * 2047 and ref.touched.size == 3000
    run = RefreshRun(c)
    err = _refresh_and_check(run, ref, "T 1024")
    _REPORT.append("refresh 2x1500  T 1024 upd [0, 1024)  leaf error %.2f u (bound %d u)" %
                   (err / rr.U24, round(rr.leaf_bound(1024) / rr.U24)))
    run = RefreshRun(c)
    rc = kernels().r2_seqprio_refresh(*run.refresh_args(run.tree.buf.p, T=1025, upd=(0, 1025)),
                                      stream_handle())
    assert rc == -2
    sync, step = torch.zeros(8, dtype=torch.int32, device=DEV), word(0, torch.int64)
    a = run.refresh_args(0, T=1025, upd=(0, 1025))
    assert kernels().r2_prio_tail(*a[:4], *run.tree.geom(), *a[5:], sync.data_ptr(), step.data_ptr(), 1,
                                  stream_handle()) == -2
    torch.cuda.synchronize()
    run.tree.buf.assert_untouched("leaves")
    run.dirty.assert_untouched("dirty")
    assert int(run.count.item()) == 0 and int(step.item()) == 0


def test_refresh_clamps_the_dirty_list_not_the_leaves():
    c = make_refresh_case(5, 1000, 80, 40, 80, "all")
    ref = refresh_of(c)
    assert ref.touched.size > 16
    run = RefreshRun(c, max_dirty=16)
    _refresh_and_check_clamped(run, ref)


def _refresh_and_check_clamped(run, ref):
    tree = run.tree
    assert kernels().r2_seqprio_refresh(*run.refresh_args(tree.buf.p), stream_handle()) == 0
    torch.cuda.synchronize()
    tree.buf.assert_guards()
    run.dirty.assert_guards("dirty[16..]")
    # every touched leaf written, the count the oracle's, 16 entries from the touched set
    rr.check_refresh(ref, tree.buf.tail(init=True), tree.buf.tail(), run.dirty.tail(),
                     int(run.count.item()), 16, run.c["T"])
    assert (run.dirty.body() >= 0).all()


# ================================================================== fused tail + sample
def test_prio_tail_sample_draws_from_the_repaired_tree():
    """r2_prio_tail_sample on the 5,000-row tree: the refresh and the repair as above, then the
    next batch drawn inside the launch from the repaired tree with counter step + 1, its row list
    and stored states; the TD flag (pre-set to 1: nothing waits) is consumed."""
    c = make_refresh_case(5, 1000, 80, 40, 80, "every40")
    ref = refresh_of(c)
    run = RefreshRun(c)
    tree = run.tree
    B, Tn, H, nstate, cap_e = len(c["starts"]), 85, 260, 3, 1000
    offs = [0, 5, cap_e - 1]
    src, dsrc, h, cc, ptrs = _state_setup(c["cap"], H, nstate, 1, B)
    off = np.asarray(offs + [0], dtype=np.int32)
    s_starts, s_probs = Buf.poisoned(B, torch.int32, -1), Buf.poisoned(B, torch.float32, NAN)
    s_rows = Buf.poisoned(Tn * B, torch.int32, -1)
    sync = torch.zeros(8, dtype=torch.int32, device=DEV)
    step0 = 2 ** 33 - 1
    step = word(step0, torch.int64)
    wait = word(1)
    q = Buf(np.full(4, 7, dtype=np.int32), -1)
    a = run.refresh_args(0)
    rc = kernels().r2_prio_tail_sample(*a[:4], *tree.geom(), *a[5:], sync.data_ptr(), step.data_ptr(),
                                       SEEDS[0], s_starts.p, s_probs.p, s_rows.p, Tn, H, nstate,
                                       ptrs["hs"].ctypes.data, off.ctypes.data, ptrs["h"].ctypes.data,
                                       ptrs["c"].ctypes.data, 1, q.p, 0, wait.data_ptr(), stream_handle())
    assert rc == 0
    torch.cuda.synchronize()
    for b in (tree.buf, run.dirty, s_starts, s_probs, s_rows, q):
        b.assert_guards()
    run.check_inputs_kept()
    assert sync.tolist() == [0] * 8 and int(wait.item()) == 0
    assert int(step.item()) == step0 + 1 and int(run.count.item()) == 0
    n0 = tree.sizes[0]
    rr.check_refresh(ref, tree.buf.tail(init=True)[:n0], tree.buf.tail()[:n0], run.dirty.tail(),
                     ref.count, run.max_dirty, c["T"])
    tree.check()
    leaves = tree.host()[:n0]
    rep = rr.check_samples(leaves, tree.levels, B, SEEDS[0], step0 + 1, s_starts.body(),
                           s_probs.body(), tree.root())
    _check_rows_and_states(s_starts.body(), s_rows.body(), B, Tn, cap_e, offs, src, h, cc, H, 1)
    assert q.body().tolist() == [0, 0, 7, 7]
    _REPORT.append("sample  %-18s levels %d  miss %.3e (d %.3e)  ambiguous %.4f  differ %d" %
                   ("prio_tail_sample", tree.levels, rep.miss, rr.sample_tolerance(tree.levels),
                    rep.ambiguous,
                    int((s_starts.body() != rr.sample_ref(leaves, B, SEEDS[0], step0 + 1)[0]).sum())))


# ================================================================== marking
class EditRun:
    def __init__(self, c):
        self.c = c
        self.flags = Buf(c["flags"], 0xAB)
        self.leaves = Buf(c["leaves"], NAN)
        self.priority = Buf(c["priority"], NAN)
        self.dirty = Buf.poisoned(256, torch.int32, -1)
        self.count = word(0)
        self.n_valid = word(100)

    def check(self, ref, T):
        self.flags.assert_guards("flags")
        self.leaves.assert_guards("leaves")
        self.dirty.assert_guards("dirty")
        self.priority.assert_untouched("priority")
        want = ref._replace(leaves=np.concatenate([ref.leaves, np.full(G, np.nan)]))
        return rr.check_edit(want, self.flags.body(), self.leaves.tail(init=True), self.leaves.tail(),
                             int(self.n_valid.item()) - 100, self.dirty.tail(), int(self.count.item()),
                             256, T)


@pytest.mark.parametrize("T", EDIT_T)
def test_mark_starts_against_the_oracle(T):
    worst = 0.0
    c = make_edit_case(T)
    rows = mark_rows(c)
    d_rows = torch.from_numpy(rows).to(DEV)
    for n_rows in (None, len(rows) - 4, len(rows) + 9):
        run = EditRun(c)
        n_dev = None if n_rows is None else word(n_rows)
        rc = kernels().r2_mark_starts(d_rows.data_ptr(), 0 if n_dev is None else n_dev.data_ptr(),
                                      len(rows), run.flags.p, run.priority.p, run.leaves.p, T,
                                      c["cap_e"], ETA, run.n_valid.data_ptr(), run.dirty.p,
                                      run.count.data_ptr(), 256, stream_handle())
        assert rc == 0
        torch.cuda.synchronize()
        ref = rr.mark_starts_ref(rows, n_rows, len(rows), c["flags"], c["priority"], c["leaves"], T,
                                 c["cap_e"], ETA)
        worst = max(worst, run.check(ref, T))
    _REPORT.append("mark    3x300   T %3d  leaf error %.2f u (bound %d u)" %
                   (T, worst / rr.U24, round(rr.leaf_bound(T) / rr.U24)))


@pytest.mark.parametrize("T", EDIT_T)
def test_apply_pending_against_the_oracle(T):
    worst = 0.0
    c = make_edit_case(T)
    pend = pending_list(c)
    d_pend = torch.from_numpy(pend).to(DEV)
    for cnt, cap_p in ((len(pend), len(pend) + 3), (len(pend) + 5, len(pend) - 3)):
        run = EditRun(c)
        d_cnt, err = word(cnt), word(0)
        rc = kernels().r2_apply_pending(d_pend.data_ptr(), d_cnt.data_ptr(), cap_p, run.flags.p,
                                        run.priority.p, run.leaves.p, T, c["cap_e"], ETA,
                                        run.n_valid.data_ptr(), run.dirty.p, run.count.data_ptr(), 256,
                                        err.data_ptr(), stream_handle())
        assert rc == 0
        torch.cuda.synchronize()
        ref = rr.apply_pending_ref(pend, cnt, cap_p, c["flags"], c["priority"], c["leaves"], T,
                                   c["cap_e"], ETA)
        assert int(err.item()) == ref.err == (2 if cnt > cap_p else 0)
        assert int(d_cnt.item()) == cnt
        worst = max(worst, run.check(ref, T))
    _REPORT.append("pending 3x300   T %3d  leaf error %.2f u (bound %d u)" %
                   (T, worst / rr.U24, round(rr.leaf_bound(T) / rr.U24)))
