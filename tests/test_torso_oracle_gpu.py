"""The bf16 conv torso launchers (torso.hip r2_torso_fwd_geom, torso_bwd.hip r2_torso_bwd_geom), the
split-precision forward and backward (torso_sp.hip r2_torso_fwd_sp_multi with static jobs,
r2_torso_bwd_sp) and the library path's
elementwise helpers against the float64 oracle (pytorch_r2d2_amd/torso_ref.py):
per-element bounds, write ownership in NaN-poisoned guard-banded buffers, bound-free bit identity
and the launchers' refusals.  The cases and their operands are the ones
tests/test_torso_ref_cpu.py runs through the fp32/bf16 emulation."""
import numpy as np
import pytest
import torch

from gpu_support import DEV, Guarded, dev, dev_bf16
from gpu_support import stop_after_a_gpu_error  # noqa: F401
from pytorch_r2d2_amd import refnum as rn
from pytorch_r2d2_amd import torso_ref as R
from pytorch_r2d2_amd.ops._lib import kernels, ptr, stream_handle

pytestmark = pytest.mark.gpu
PAD = 1024                     # guard elements at each end of an output buffer
FWD = {c["name"]: c for c in R.FWD_CASES}
BWD = {c["name"]: c for c in R.BWD_CASES}
SP = {c["name"]: c for c in R.SP_CASES}
SPB = {c["name"]: c for c in R.SP_BWD_CASES}


def _fig(line):
    print("torso-oracle: " + line)


def _guarded(shape, dtype=torch.float32, pad=PAD):
    return Guarded(shape, dtype, pad)


_WTS = {}


def _dev_weights(geo, wts, key):
    if key not in _WTS:
        _WTS[key] = [dev_bf16(wts["w1_pk"]), dev(wts["b1"]), dev_bf16(wts["w2_pk"]), dev(wts["b2"]),
                     dev_bf16(wts["w3_pk"]), dev(wts["b3"])]
    return _WTS[key]


# ---- forward -----------------------------------------------------------------------------------

class FwdRun:
    """Device operands and poisoned outputs of one r2_torso_fwd_geom launch."""

    def __init__(self, geo, ops, saves=None, null_rows=None):
        self.geo, self.ops = geo, ops
        self.store = dev(ops["store"])
        self.keep, self.outs, words = [], [], []
        for i, job in enumerate(ops["jobs"]):
            n = job["n"]
            rows = None if job["rows"] is None or null_rows else dev(job["rows"])
            w = _dev_weights(geo, job["wts"], (geo.key, job["wts"]["seed"]))
            sv = job["saves"] if saves is None else saves
            o = dict(out=_guarded((n, 32, geo.P3), torch.bfloat16),
                     save1=_guarded((n, geo.P1, 32), torch.bfloat16) if sv else None,
                     save2=_guarded((n, geo.P2, 32), torch.bfloat16) if sv else None)
            words += [ptr(rows), n] + [ptr(t) for t in w] + [
                o["out"].ptr(), o["save1"].ptr() if sv else 0, o["save2"].ptr() if sv else 0, 0]
            self.keep += [rows, job["wts"]]
            self.outs.append(o)
        self.arr = np.asarray(words, dtype=np.int64)

    def launch(self, grid, reserve=(0, 0), njobs=None, row_bytes=None, geom=None):
        rb = self.ops["row_bytes"] if row_bytes is None else row_bytes
        rc = kernels().r2_torso_fwd_geom(ptr(self.store), rb, self.arr.ctypes.data,
                                         len(self.outs) if njobs is None else njobs, grid, reserve[0],
                                         reserve[1], *(geom or self.geo.key), stream_handle())
        torch.cuda.synchronize()
        return rc

    def untouched(self, label):
        for j, o in enumerate(self.outs):
            for name, g in o.items():
                if g is not None:
                    g.untouched(f"{label}/job{j}", name)

    def check(self, label, strides):
        """Ownership of every output, then the teacher-forced oracle on every job that has saves."""
        for j, (job, o) in enumerate(zip(self.ops["jobs"], self.outs)):
            lab = f"{label}/job{j}"
            for name, g in o.items():
                if g is not None:
                    g.owned(lab, name)
            if job["n"] == 0 or o["save1"] is None:
                continue
            stored = {k: o[k].bits() for k in ("save1", "save2", "out")}
            uses = R.check_forward(lab, self.geo, job["frames"], job["wts"], stored, strides[j])
            emu = R.emulate_forward(self.geo, job["frames"], job["wts"])
            eu = R.check_forward(lab + "/emu", self.geo, job["frames"], job["wts"], emu, strides[j])
            _fig(f"fwd {lab:28s} " + "  ".join(f"{k} {uses[k]:.3f} [{eu[k]:.3f}]" for k in uses))

    def out_bits(self, j=0):
        return self.outs[j]["out"].bits()


@pytest.mark.parametrize("name", list(FWD))
def test_forward_case(name):
    """Every element of save1 / save2 / out of every job within its bound, every element written,
    no guard element touched.  A job the table runs without saves is run again with saves: the
    oracle checks that run, and ``out`` must not depend on the saves."""
    case = FWD[name]
    geo, ops = R.GEOMS[case["geom"]], R.forward_operands(case)
    strides = R.forward_strides(case)
    run = FwdRun(geo, ops)
    assert run.launch(case["grid"], case.get("reserve", (0, 0))) == 0
    run.check(name, strides)
    if not all(j["saves"] for j in ops["jobs"]):
        full = FwdRun(geo, ops, saves=True)
        assert full.launch(case["grid"], case.get("reserve", (0, 0))) == 0
        full.check(name + "+saves", strides)
        for j in range(len(ops["jobs"])):
            assert np.array_equal(run.out_bits(j), full.out_bits(j)), f"{name}: job {j} out depends on the saves"


@pytest.mark.parametrize("geom", list(R.GEOMS))
def test_forward_out_is_bitwise_independent_of_the_launch_shape(geom):
    """Bound-free: ``out`` of one job is bit-identical across grids, saves requested or not, job
    position, reserve settings, and rows = 0 against identity rows."""
    geo = R.GEOMS[geom]
    base = dict(name=f"{geom}/bitwise", geom=geom, grid=2, jobs=[dict(n=5, w="a")])
    ops = R.forward_operands(base)
    ref = FwdRun(geo, ops)
    assert ref.launch(2) == 0
    ref.check(base["name"], [2])
    want = ref.out_bits()
    for grid in (1, 3, 5, 8, 0):
        r = FwdRun(geo, ops)
        assert r.launch(grid) == 0
        assert np.array_equal(r.out_bits(), want), f"grid {grid}"
        for k in ("save1", "save2"):
            assert np.array_equal(r.outs[0][k].bits(), ref.outs[0][k].bits()), f"grid {grid} {k}"
    r = FwdRun(geo, ops, saves=False)
    assert r.launch(2) == 0
    assert np.array_equal(r.out_bits(), want), "saves not requested"
    r = FwdRun(geo, ops)
    assert r.launch(256, reserve=(2, 4)) == 0
    assert np.array_equal(r.out_bits(), want), "reserve (2, 4)"
    # job position: the same job second, behind a job of another weight set
    n_store = ops["store"].shape[0]
    other = dict(n=2, saves=True, rows=R.make_rows("other", 2, n_store, "random"), wts=R.make_weights(geo, "b"))
    other["frames"] = R.gather(geo, ops["store"], other["rows"], 2)
    ops2 = dict(ops, jobs=[other, ops["jobs"][0]])
    r = FwdRun(geo, ops2)
    assert r.launch(4) == 0
    r.check(base["name"] + "/second", [c for _, _, c in R.deal_workers([2, 5], 4)])
    assert np.array_equal(r.out_bits(1), want), "job position"
    # rows = 0 against identity rows
    ident = dict(ops["jobs"][0], rows=np.arange(5, dtype=np.int32), frames=R.gather(geo, ops["store"], None, 5))
    ops3 = dict(ops, jobs=[ident])
    a, b = FwdRun(geo, ops3), FwdRun(geo, ops3, null_rows=True)
    assert a.launch(2) == 0 and b.launch(2) == 0
    a.check(base["name"] + "/identity", [2])
    assert np.array_equal(a.out_bits(), b.out_bits()), "rows = 0 vs identity rows"


@pytest.mark.parametrize("geom", list(R.GEOMS))
def test_forward_refusals_write_nothing(geom):
    geo = R.GEOMS[geom]
    case = dict(name=f"{geom}/refuse", geom=geom, grid=2, jobs=[dict(n=1, w="a"), dict(n=1, w="b")])
    ops = R.forward_operands(case)
    run = FwdRun(geo, ops)
    fb = geo.fb
    assert run.launch(2, njobs=0) == -1
    assert run.launch(2, njobs=5) == -1
    assert run.launch(2, reserve=(2, 32)) == -2
    assert run.launch(2, reserve=(9, 4)) == -2
    assert run.launch(2, reserve=(2, -1)) == -2
    assert run.launch(1) == -3                      # two jobs, one worker
    assert run.launch(2, geom=(geo.cin, geo.h, geo.w - 4)) == -6
    assert run.launch(2, geom=(geo.cin + 1, geo.h, geo.w)) == -6
    assert run.launch(2, row_bytes=fb - 16) == -7
    assert run.launch(2, row_bytes=fb + 8) == -7
    run.untouched(case["name"])


# ---- forward, split precision ------------------------------------------------------------------

SP_OUT = ("out", "out_lo", "s1", "s1_lo", "s2", "s2_lo")


def _dev_weights_sp(geo, wts):
    key = ("sp", geo.key, wts["seed"])
    if key not in _WTS:
        _WTS[key] = [dev_bf16(wts["w1_hi"]), dev_bf16(wts["w1_lo"]), dev(wts["b1"]),
                     dev_bf16(wts["w2_hi"]), dev_bf16(wts["w2_lo"]), dev(wts["b2"]),
                     dev_bf16(wts["w3_hi"]), dev_bf16(wts["w3_lo"]), dev(wts["b3"])]
    return _WTS[key]


class SpRun:
    """Device operands and poisoned outputs of one r2_torso_fwd_sp_multi launch (20 words a job)."""

    def __init__(self, geo, ops, saves=None, null_rows=None):
        self.geo, self.ops = geo, ops
        self.store = dev(ops["store"])
        self.keep, self.outs, words = [], [], []
        for job in ops["jobs"]:
            n = job["n"]
            rows = None if job["rows"] is None or null_rows else dev(job["rows"])
            sv = job["saves"] if saves is None else saves
            shapes = dict(out=(n, 32, geo.P3), s1=(n, geo.P1, 32), s2=(n, geo.P2, 32))
            o = {k: _guarded(shapes[k.split("_")[0]], torch.bfloat16) if sv or k.startswith("out") else None
                 for k in SP_OUT}
            words += [ptr(rows), n] + [ptr(t) for t in _dev_weights_sp(geo, job["wts"])] + [
                o[k].ptr() if o[k] is not None else 0 for k in SP_OUT] + [0, 0, 0]
            self.keep.append(rows)
            self.outs.append(o)
        self.arr = np.asarray(words, dtype=np.int64)
        assert self.arr.size == 20 * len(ops["jobs"])

    def launch(self, grid, njobs=None, arr=None):
        arr = self.arr if arr is None else arr
        rc = kernels().r2_torso_fwd_sp_multi(ptr(self.store), arr.ctypes.data,
                                             len(self.outs) if njobs is None else njobs, grid, stream_handle())
        torch.cuda.synchronize()
        return rc

    def untouched(self, label):
        for j, o in enumerate(self.outs):
            for name, g in o.items():
                if g is not None:
                    g.untouched(f"{label}/job{j}", name)

    def check(self, label, strides):
        for j, (job, o) in enumerate(zip(self.ops["jobs"], self.outs)):
            lab = f"{label}/job{j}"
            for name, g in o.items():
                if g is not None:
                    g.owned(lab, name)
            if job["n"] == 0 or o["s1"] is None:
                continue
            stored = {k: o[k].bits() for k in SP_OUT}
            uses = R.check_forward_sp(lab, self.geo, job["frames"], job["wts"], stored, strides[j])
            emu = R.emulate_forward_sp(self.geo, job["frames"], job["wts"])
            eu = R.check_forward_sp(lab + "/emu", self.geo, job["frames"], job["wts"], emu, strides[j])
            _fig(f"fwd {lab:28s} " + "  ".join(f"{k} {uses[k]:.3f} [{eu[k]:.3f}]" for k in uses))
            yield j, job, stored

    def out_bits(self, j=0):
        return np.stack([self.outs[j]["out"].bits(), self.outs[j]["out_lo"].bits()])


@pytest.mark.parametrize("name", list(SP))
def test_split_forward_case(name):
    """Both planes of s1 / s2 / out of every job within their bounds, every element written, no
    guard element touched; W1 = 0 leaves act1 = ReLU(b1) exactly."""
    case = SP[name]
    geo, ops = R.GEOMS[case["geom"]], R.forward_sp_operands(case)
    strides = R.forward_strides(case)
    run = SpRun(geo, ops)
    assert run.launch(case["grid"]) == 0
    for j, job, stored in run.check(name, strides):
        if case["jobs"][j].get("w1") == "zero":
            hi, lo = rn.split_planes(np.maximum(job["wts"]["b1"], 0))
            assert (rn.bf16_val(stored["s1"]) == hi).all() and (rn.bf16_val(stored["s1_lo"]) == lo).all()
    if not all(j["saves"] for j in ops["jobs"]):
        full = SpRun(geo, ops, saves=True)
        assert full.launch(case["grid"]) == 0
        list(full.check(name + "+saves", strides))
        for j in range(len(ops["jobs"])):
            assert np.array_equal(run.out_bits(j), full.out_bits(j)), f"{name}: job {j} out depends on the saves"


def test_split_forward_out_is_bitwise_independent_of_the_launch_shape():
    geo = R.GEOMS["atari"]
    base = dict(name="sp/atari/bitwise", geom="atari", grid=2, jobs=[dict(n=5, w="a")])
    ops = R.forward_sp_operands(base)
    ref = SpRun(geo, ops)
    assert ref.launch(2) == 0
    list(ref.check(base["name"], [2]))
    want = ref.out_bits()
    for grid in (1, 3, 5, 8, 0):
        r = SpRun(geo, ops)
        assert r.launch(grid) == 0
        assert np.array_equal(r.out_bits(), want), f"grid {grid}"
        for k in ("s1", "s1_lo", "s2", "s2_lo"):
            assert np.array_equal(r.outs[0][k].bits(), ref.outs[0][k].bits()), f"grid {grid} {k}"
    r = SpRun(geo, ops, saves=False)
    assert r.launch(2) == 0
    assert np.array_equal(r.out_bits(), want), "saves not requested"
    n_store = ops["store"].shape[0]
    other = dict(n=2, saves=True, rows=R.make_rows("other", 2, n_store, "random"), wts=R.make_weights_sp(geo, "b"))
    other["frames"] = R.gather(geo, ops["store"], other["rows"], 2)
    r = SpRun(geo, dict(ops, jobs=[other, ops["jobs"][0]]))
    assert r.launch(4) == 0
    list(r.check(base["name"] + "/second", [c for _, _, c in R.deal_workers([2, 5], 4)]))
    assert np.array_equal(r.out_bits(1), want), "job position"
    ident = dict(ops["jobs"][0], rows=np.arange(5, dtype=np.int32), frames=R.gather(geo, ops["store"], None, 5))
    ops3 = dict(ops, jobs=[ident])
    a, b = SpRun(geo, ops3), SpRun(geo, ops3, null_rows=True)
    assert a.launch(2) == 0 and b.launch(2) == 0
    list(a.check(base["name"] + "/identity", [2]))
    assert np.array_equal(a.out_bits(), b.out_bits()), "rows = 0 vs identity rows"


def test_split_forward_refusals_write_nothing():
    """-1 (job count), -3 (two jobs, one workgroup), -4 (a missing lo plane), -5 (a queue job with
    saves or an unknown queue mode): each returns before any launch."""
    geo = R.GEOMS["atari"]
    case = dict(name="sp/atari/refuse", geom="atari", grid=2, jobs=[dict(n=1, w="a"), dict(n=1, w="b")])
    run = SpRun(geo, R.forward_sp_operands(case))
    assert run.launch(2, njobs=0) == -1
    assert run.launch(2, njobs=5) == -1
    assert run.launch(1) == -3
    for word in (3, 6, 9, 12, 14, 16):               # w1l, w2l, w3l, out_l, s1l, s2l
        arr = run.arr.copy()
        arr[20 + word] = 0
        assert run.launch(2, arr=arr) == -4, word
    q = torch.zeros(4, dtype=torch.int32, device=DEV)
    arr = run.arr.copy()
    arr[17], arr[18] = ptr(q), 1                      # a queue job that asks for saves
    assert run.launch(2, arr=arr) == -5
    arr[13:17] = 0
    arr[18] = 3                                       # no saves, unknown mode
    assert run.launch(2, arr=arr) == -5
    run.untouched(case["name"])
    assert int(q.sum().item()) == 0


# ---- backward ----------------------------------------------------------------------------------

class BwdRun:
    """Device operands and poisoned outputs of one r2_torso_bwd_geom launch."""

    def __init__(self, case):
        self.case, self.ops = case, R.backward_operands(case)
        o, self.geo = self.ops, self.ops["geo"]
        n = case["n"]
        self.G = R.effective_grid(case["grid"], n)
        self.t = dict(store=dev(o["store"]), rows=dev(o["rows"]), act1=dev_bf16(o["act1"]),
                      act2=dev_bf16(o["act2"]), dx3=dev_bf16(o["dx3"]), out3=dev_bf16(o["out3"]),
                      w3dg=dev_bf16(o["w3_dg"]), w2dg=dev_bf16(o["w2_dg"]), dst=dev(o["dst"]),
                      scale=dev(o["scale"]))
        self.slab_rows = max(case["grid"], n) + 1
        self.slab = _guarded((self.slab_rows, self.geo.SLAB))
        self.grad = _guarded((o["grad_numel"],))

    def args(self, **over):
        t, o = self.t, self.ops
        a = dict(frames=ptr(t["store"]), row_bytes=o["row_bytes"], rows=ptr(t["rows"]), n=self.case["n"],
                 act1=ptr(t["act1"]), act2=ptr(t["act2"]), dx3=ptr(t["dx3"]), out3=ptr(t["out3"]),
                 w3dg=ptr(t["w3dg"]), w2dg=ptr(t["w2dg"]), slab=self.slab.ptr(), grid=self.case["grid"],
                 dst=ptr(t["dst"]), scale=ptr(t["scale"]), grad=self.grad.ptr(), cin=self.geo.cin,
                 h=self.geo.h, w=self.geo.w)
        a.update(over)
        return list(a.values())

    def launch(self, **over):
        rc = kernels().r2_torso_bwd_geom(*self.args(**over), stream_handle())
        torch.cuda.synchronize()
        return rc

    def check(self, label):
        geo, o = self.geo, self.ops
        valid = np.zeros((self.slab_rows, geo.SLAB), bool)
        valid[:self.G] = True                       # rows >= min(grid, n) stay untouched
        self.slab.owned(label, "slab", valid)
        torso = np.zeros(o["grad_numel"], bool)
        torso[o["dst"]] = True                      # every foreign element keeps its poison
        self.grad.owned(label, "grad", torso)
        slab = self.slab.host()[:self.G]
        u_slab = R.check_slab(label, geo, o, self.case["grid"], slab)
        u_grad = R.check_reduce(label, slab, o["dst"], o["scale"], self.grad.host())
        emu = R.emulate_backward(geo, o, self.case["grid"])
        e_slab = R.check_slab(label + "/emu", geo, o, self.case["grid"], emu)
        e_grad = R.check_reduce(label + "/emu", emu, o["dst"], o["scale"],
                                R.emulate_reduce(emu, o["dst"], o["scale"], np.zeros(o["grad_numel"], np.float32)))
        _fig(f"bwd {label:28s} slab {u_slab:.3f} [{e_slab:.3f}]  grad {u_grad:.3f} [{e_grad:.3f}]")


@pytest.mark.parametrize("name", list(BWD))
def test_backward_case(name):
    """Each slab row and the reduced gradient per element, ownership of slab and grad, and two
    runs bit for bit."""
    a, b = BwdRun(BWD[name]), BwdRun(BWD[name])
    assert a.launch() == 0 and b.launch() == 0
    a.check(name)
    assert np.array_equal(a.slab.bits()[:a.G], b.slab.bits()[:a.G]), "two runs differ (slab)"
    ga, gb = a.grad.bits(), b.grad.bits()
    assert np.array_equal(ga[a.ops["dst"]], gb[a.ops["dst"]]), "two runs differ (grad)"


@pytest.mark.parametrize("geom", list(R.GEOMS))
def test_backward_refusals_write_nothing(geom):
    """-6, -7, and -1 for a missing rows list or operand: each returns before any launch."""
    run = BwdRun(BWD[f"{geom}/n2g2"])
    fb = run.geo.fb
    assert run.launch(w=run.geo.w - 4) == -6
    assert run.launch(cin=run.geo.cin + 1) == -6
    assert run.launch(row_bytes=fb - 16) == -7
    assert run.launch(row_bytes=fb + 8) == -7
    for name in ("frames", "rows", "act1", "act2", "dx3", "out3", "w3dg", "w2dg", "slab", "dst", "scale", "grad"):
        assert run.launch(**{name: 0}) == -1, name
    run.slab.untouched(geom, "slab")
    run.grad.untouched(geom, "grad")
    assert run.launch(n=0) == 0
    run.slab.untouched(geom, "slab")


# ---- backward, split precision -----------------------------------------------------------------

class SpBwdRun(BwdRun):
    """Device operands and poisoned outputs of one r2_torso_bwd_sp launch."""

    def __init__(self, case):
        self.case, self.ops = case, R.backward_sp_operands(case)
        o, self.geo = self.ops, self.ops["geo"]
        n = case["n"]
        self.G = R.effective_grid(case["grid"], n)
        self.t = dict(store=dev(o["store"]), rows=dev(o["rows"]), out3=dev_bf16(o["out3"]),
                      dst=dev(o["dst"]), scale=dev(o["scale"]))
        for k in ("act1", "act2", "dx3"):
            self.t[k], self.t[k + "l"] = dev_bf16(o[k + "_hi"]), dev_bf16(o[k + "_lo"])
        for k in ("w3", "w2"):
            self.t[k + "dg"], self.t[k + "dgl"] = dev_bf16(o[k + "_dg"]), dev_bf16(o[k + "_dg_lo"])
        self.slab_rows = max(case["grid"], n) + 1
        self.slab = _guarded((self.slab_rows, self.geo.SLAB))
        self.grad = _guarded((o["grad_numel"],))

    def launch(self, **over):
        t = self.t
        a = dict(frames=ptr(t["store"]), rows=ptr(t["rows"]), n=self.case["n"])
        for k in ("act1", "act1l", "act2", "act2l", "dx3", "dx3l", "out3", "w3dg", "w3dgl", "w2dg", "w2dgl"):
            a[k] = ptr(t[k])
        a.update(slab=self.slab.ptr(), grid=self.case["grid"], dst=ptr(t["dst"]), scale=ptr(t["scale"]),
                 grad=self.grad.ptr())
        a.update(over)
        rc = kernels().r2_torso_bwd_sp(*a.values(), stream_handle())
        torch.cuda.synchronize()
        return rc

    def check(self, label):
        geo, o = self.geo, self.ops
        valid = np.zeros((self.slab_rows, geo.SLAB), bool)
        valid[:self.G] = True
        self.slab.owned(label, "slab", valid)
        torso = np.zeros(o["grad_numel"], bool)
        torso[o["dst"]] = True
        self.grad.owned(label, "grad", torso)
        slab = self.slab.host()[:self.G]
        u_slab = R.check_slab(label, geo, o, self.case["grid"], slab, sp=True)
        u_grad = R.check_reduce(label, slab, o["dst"], o["scale"], self.grad.host())
        emu = R.emulate_backward_sp(geo, o, self.case["grid"])
        e_slab = R.check_slab(label + "/emu", geo, o, self.case["grid"], emu, sp=True)
        e_grad = R.check_reduce(label + "/emu", emu, o["dst"], o["scale"],
                                R.emulate_reduce(emu, o["dst"], o["scale"], np.zeros(o["grad_numel"], np.float32)))
        _fig(f"bwd {label:28s} slab {u_slab:.3f} [{e_slab:.3f}]  grad {u_grad:.3f} [{e_grad:.3f}]")


@pytest.mark.parametrize("name", list(SPB))
def test_split_backward_case(name):
    a, b = SpBwdRun(SPB[name]), SpBwdRun(SPB[name])
    assert a.launch() == 0 and b.launch() == 0
    a.check(name)
    assert np.array_equal(a.slab.bits()[:a.G], b.slab.bits()[:a.G]), "two runs differ (slab)"
    assert np.array_equal(a.grad.bits()[a.ops["dst"]], b.grad.bits()[a.ops["dst"]]), "two runs differ (grad)"


def test_split_backward_refusals_write_nothing():
    """-1 for a missing rows list or lo plane, before any launch."""
    run = SpBwdRun(SPB["sp/atari/n2g2"])
    for name in ("rows", "act1l", "act2l", "dx3l", "w3dgl", "w2dgl"):
        assert run.launch(**{name: 0}) == -1, name
    assert run.launch(n=0) == 0
    run.slab.untouched("sp", "slab")
    run.grad.untouched("sp", "grad")


# ---- elementwise helpers of the library path ---------------------------------------------------

def _frames_ref(fr):
    """bf16(fl32(u8) * fl32(1/255)): one rounding per element."""
    return rn.bf16_bits((fr.astype(np.float32) * np.float32(1.0 / 255.0)).astype(np.float32))


@pytest.mark.parametrize("rows_mode", ["dup_desc", "null"])
@pytest.mark.parametrize("nhwc", [False, True])
def test_frames_to_bf16_bit_exact(nhwc, rows_mode):
    geo, n = R.GEOMS["atari"], 3
    store = R.make_store(geo, "helpers", 6, 0, "random")
    store[0, :256] = np.arange(256, dtype=np.uint8)          # every byte value
    rows = R.make_rows("helpers", n, 6, rows_mode)
    fr = R.gather(geo, store, rows, n)
    want = _frames_ref(fr.transpose(0, 2, 3, 1) if nhwc else fr).reshape(n, geo.fb)
    out = _guarded((n, geo.fb), torch.bfloat16)
    s, r = dev(store), (None if rows is None else dev(rows))
    fn = kernels().r2_frames_to_bf16_nhwc if nhwc else kernels().r2_frames_to_bf16
    assert fn(ptr(s), ptr(r), n, out.ptr(), stream_handle()) == 0
    torch.cuda.synchronize()
    out.owned("frames_to_bf16", "out")
    assert np.array_equal(out.bits(), want)
    idle = _guarded((n, geo.fb), torch.bfloat16)
    assert fn(ptr(s), ptr(r), 0, idle.ptr(), stream_handle()) == 0
    torch.cuda.synchronize()
    idle.untouched("frames_to_bf16 n=0", "out")


def test_bias_relu_nhwc_bit_exact_and_refusals():
    """In place on a guarded buffer, C = 32, a length whose last block is partial (n / 8 = 308)."""
    Cc, n = 32, 32 * 77
    r = np.random.default_rng(3)
    x = rn.bf16_round(r.standard_normal(n))
    x[:8] = [0.0, -0.0, 1.0, -1.0, 2.0 ** -126, -2.0 ** -126, 3.0, -3.0]
    bias = r.standard_normal(Cc).astype(np.float32)
    bias[1] = 0.0
    want = rn.bf16_bits(np.maximum((x.reshape(-1, Cc) + bias).astype(np.float32), np.float32(0))).reshape(-1)
    buf = _guarded((n,), torch.bfloat16)
    buf.body.copy_(dev_bf16(x))
    b = dev(bias)
    k = kernels()
    for bad in ((buf.ptr(), 12, 24), (buf.ptr(), Cc, n - 8), (buf.ptr() + 8, Cc, n)):   # C % 8, n % C, alignment
        assert k.r2_bias_relu_nhwc_bf16(bad[0], ptr(b), bad[1], bad[2], stream_handle()) == -1
    torch.cuda.synchronize()
    assert np.array_equal(buf.bits(), rn.bf16_bits(x)), "a refused launch wrote"
    assert k.r2_bias_relu_nhwc_bf16(buf.ptr(), ptr(b), Cc, n, stream_handle()) == 0
    torch.cuda.synchronize()
    buf.owned("bias_relu", "x")
    got = buf.bits()
    got = np.where(got == 0x8000, 0, got)            # max(-0, 0) may keep either zero
    assert np.array_equal(got, np.where(want == 0x8000, 0, want))


def test_relu_mask_bit_exact_and_refusals():
    """n = 8 k with k odd (333), so the last vector of the last block is the tail."""
    n = 8 * 333
    r = np.random.default_rng(4)
    g = rn.bf16_round(r.standard_normal(n))
    act = rn.bf16_round(r.standard_normal(n)) * (r.random(n) < 0.7)
    act[:4] = [0.0, -0.0, 2.0 ** -126, -2.0 ** -126]
    gb = rn.bf16_bits(g)
    want = np.where(act > 0, gb, np.uint16(0))
    gd, ad = dev_bf16(g), dev_bf16(act)
    out = _guarded((n,), torch.bfloat16)
    k = kernels()
    assert k.r2_relu_mask_bf16(ptr(gd), ptr(ad), out.ptr(), n - 4, stream_handle()) == -1     # n % 8
    for i in range(3):                                                                        # alignment
        p = [ptr(gd), ptr(ad), out.ptr()]
        p[i] += 8
        assert k.r2_relu_mask_bf16(*p, n - 8, stream_handle()) == -1
    torch.cuda.synchronize()
    out.untouched("relu_mask refused", "out")
    assert k.r2_relu_mask_bf16(ptr(gd), ptr(ad), out.ptr(), n, stream_handle()) == 0
    torch.cuda.synchronize()
    out.owned("relu_mask", "out")
    assert np.array_equal(out.bits(), want)
