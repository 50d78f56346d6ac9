"""Every recurrence entry point of lstm.hip, lstm_persist.hip and lstm_bptt.hip against the
teacher-forced float64 oracle (pytorch_r2d2_amd/lstm_ref.py): per-element bounds, bound-free
consistency, write ownership, launch-site state and the launchers' refusals.  The cases and their
operands are the ones tests/test_lstm_ref_cpu.py runs through the fp32 emulation."""
import numpy as np
import pytest
import torch

from gpu_support import DEV, NAN, Guarded, dev, dev_bf16
from gpu_support import stop_after_a_gpu_error  # noqa: F401
from pytorch_r2d2_amd import lstm_ref as R
from pytorch_r2d2_amd import refnum as rn
from pytorch_r2d2_amd.ops._lib import bptt_opts, kernels, ptr, stream_handle

pytestmark = pytest.mark.gpu
PAD = 256                      # guard elements at each end of an output buffer (a multiple of 8)
EPOCH_FWD, EPOCH_BWD = 3072 + 32, 3072 + 64     # lstm_common.h PT_EPOCH_*


def _fig(line):
    print("lstm-oracle: " + line)


# ---- buffers ---------------------------------------------------------------------------------

def _guarded(shape, dtype=torch.float32, pad=PAD):
    return Guarded(shape, dtype, pad)


class Site:
    """One launch site: a counter block + error word (+ ring), as the kernels require."""

    def __init__(self, ring_bytes=0):
        k = kernels()
        self.ctr = torch.zeros(int(k.r2_lstm_persist_ctr_words()), dtype=torch.int32, device=DEV)
        self.err = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.ring = torch.zeros(max(ring_bytes, 16) // 4, dtype=torch.int32, device=DEV)
        self.launches = 0

    def check(self, label, tagged, epoch_word):
        torch.cuda.synchronize()
        assert int(self.err.item()) == 0, f"{label}: a spin timed out (err word set)"
        if tagged:
            self.launches += 1
            c = self.ctr.cpu().numpy().copy()
            other = EPOCH_BWD if epoch_word == EPOCH_FWD else EPOCH_FWD
            assert c[epoch_word] == self.launches, f"{label}: epoch {c[epoch_word]} after {self.launches} launches"
            assert c[other] == 0
            c[epoch_word] = 0
            assert not c.any(), f"{label}: counter words {np.flatnonzero(c)[:8]} not returned to zero"


# ---- forward ---------------------------------------------------------------------------------

FWD_ENTRIES = ("step", "persist", "tag", "tag_sp")


def _fwd_expected_rc(entry, H, B, nch):
    """The launchers' documented refusals for shapes of the case table."""
    cus = int(kernels().r2_get_num_cus())
    nwg = H // 16
    if entry == "step":
        return -1 if B > 128 else 0
    if entry == "persist":
        mb = (B + 31) // 32
        return -3 if nwg * mb * nch > cus or mb > 8 else 0
    if entry == "tag_sp" and H > 256:
        return -2
    groups = nch * ((B + 15) // 16)
    return -3 if groups * nwg > cus or groups > 32 else 0


class FwdRun:
    """Device operands and poisoned outputs of one forward launch."""

    def __init__(self, entry, chains, B, T, H, drop_lo=False):
        self.entry, self.sp = entry, entry == "tag_sp"
        self.B, self.T, self.H = B, T, H
        G = 4 * H
        self.keep, self.outs, words = [], [], []
        for ch in chains:
            ops = R.forward_operands(ch, self.sp)
            w_hi = dev_bf16(ops["w_hi"])
            x, c0 = dev(ch["xproj"]), dev(ch["c0"])
            h0 = dev(ops["h0"]) if self.sp else dev_bf16(ops["h0"])
            sf = int(ch["save_from"])
            o = dict(h_seq=_guarded((T, B, H), torch.bfloat16), c_seq=_guarded((T, B, H)),
                     h32=_guarded((T, B, H)) if ch["h32"] else None,
                     gates=_guarded((max(T - sf, 0), B, G), pad=max(PAD, B * G)) if ch["gates"] else None)
            w = [ptr(x), ptr(w_hi), ptr(h0), ptr(c0), o["h_seq"].ptr(), o["c_seq"].ptr(),
                 o["h32"].ptr() if o["h32"] else 0, o["gates"].ptr() if o["gates"] else 0, sf]
            self.keep += [w_hi, x, c0, h0]
            if self.sp:
                w_lo = dev_bf16(ops["w_lo"])
                o["h_seq_lo"] = _guarded((T, B, H), torch.bfloat16)
                w += [0 if drop_lo else ptr(w_lo), o["h_seq_lo"].ptr()]
                self.keep.append(w_lo)
            self.outs.append(o)
            words += w
        self.arr = np.asarray(words, dtype=np.int64)

    def launch(self, site, n_chains, B=None):
        k, a, B = kernels(), self.arr.ctypes.data, self.B if B is None else B
        if self.entry == "step":
            return k.r2_lstm_fwd(a, n_chains, B, self.T, self.H, 0, stream_handle())
        args = (a, n_chains, B, self.T, self.H, ptr(site.ctr), ptr(site.err))
        if self.entry == "persist":
            return k.r2_lstm_fwd_persist(*args, stream_handle())
        fn = k.r2_lstm_fwd_tag_sp if self.sp else k.r2_lstm_fwd_tag
        return fn(*args, ptr(site.ring), stream_handle())

    def device_outputs(self):
        return [g.full.clone() for o in self.outs for g in o.values() if g is not None]

    def assert_untouched(self, label, chains=None):
        for c, o in enumerate(self.outs):
            if chains is None or c in chains:
                for name, g in o.items():
                    if g is not None:
                        g.untouched(f"{label}/chain{c}", name)

    def check(self, label, chains):
        """Ownership, then every oracle check; returns the largest use of each bound."""
        worst = dict(gates=0.0, c=0.0, h=0.0, h_seq=0.0)
        for c, (ch, o) in enumerate(zip(chains, self.outs)):
            lab = f"{label}/chain{c}"
            for name, g in o.items():
                if g is not None:
                    g.owned(lab, name)
            bits = o["h_seq"].bits()
            out = dict(h_seq_bits=bits, h_seq=rn.bf16_val(bits), c_seq=o["c_seq"].host())
            if o["h32"]:
                out["h32"] = o["h32"].host()
            if o["gates"]:
                out["gates"] = o["gates"].host()
            if self.sp:
                out["h_seq_lo_bits"] = o["h_seq_lo"].bits()
                out["h_seq_lo"] = rn.bf16_val(out["h_seq_lo_bits"])
            uses = R.check_forward(lab, ch, out, self.sp)
            worst = {n: max(worst[n], uses[n]) for n in worst}
        return worst


def _fwd_site(entry, nch, B, H):
    k = kernels()
    return Site(int(k.r2_lstm_tag_ring_bytes(nch, B, H)) if entry.startswith("tag") else 0)


@pytest.mark.parametrize("entry", FWD_ENTRIES)
@pytest.mark.parametrize("name", list(R.FORWARD_CASES))
def test_forward_case(name, entry):
    k = kernels()
    spec, chains0 = R.forward_case(name, 0)
    _, chains1 = R.forward_case(name, 1)
    H, B, T, nch = spec["H"], spec["B"], spec["T"], len(chains0)
    label = f"{name}/{entry}"
    site = _fwd_site(entry, nch, B, H)
    tagged = entry.startswith("tag")
    want_rc = _fwd_expected_rc(entry, H, B, nch)
    run0 = FwdRun(entry, chains0, B, T, H)
    rc = run0.launch(site, nch)
    assert rc == want_rc, f"{label}: return code {rc}, documented {want_rc}"
    if rc != 0:
        torch.cuda.synchronize()
        run0.assert_untouched(label)
        _fig(f"{label:22s} refused with {rc}, nothing written")
        return
    if entry != "step":
        site.check(label, tagged, EPOCH_FWD)
    uses = run0.check(label, chains0)
    first = run0.device_outputs()
    # a second launch of the site with other inputs: stale words of the first must not be taken
    run1 = FwdRun(entry, chains1, B, T, H)
    assert run1.launch(site, nch) == 0
    if entry != "step":
        site.check(label + "/launch1", tagged, EPOCH_FWD)
    u1 = run1.check(label + "/launch1", chains1)
    uses = {n: max(uses[n], u1[n]) for n in uses}
    # repeated on the same inputs, and on the placement-independent paths: bit-identical
    modes = [0] if entry == "step" else ([0, 1, 2] if tagged else [0, 1])
    try:
        for mode in modes:
            k.r2_lstm_persist_force_slow(mode)
            again = FwdRun(entry, chains0, B, T, H)
            assert again.launch(site, nch) == 0
            if entry != "step":
                site.check(f"{label}/force_slow{mode}", tagged, EPOCH_FWD)
            for a, b in zip(first, again.device_outputs()):
                assert torch.equal(a.view(torch.int16), b.view(torch.int16)), \
                    f"{label}: outputs differ on a repeated launch (force_slow {mode})"
    finally:
        k.r2_lstm_persist_force_slow(0)
    _fig(f"{label:22s} gates {uses['gates']:.3f}  c {uses['c']:.3f}  h32 {uses['h']:.3f}  h_seq {uses['h_seq']:.3f}")


@pytest.mark.parametrize("entry", FWD_ENTRIES)
def test_forward_leaves_a_neighbouring_chain_alone(entry):
    """f_tail launched with one chain: the second chain's buffers (present in the chain array) stay
    poison, the first chain's results pass the checks."""
    spec, chains = R.forward_case("f_tail")
    H, B, T = spec["H"], spec["B"], spec["T"]
    run = FwdRun(entry, chains, B, T, H)
    site = _fwd_site(entry, 1, B, H)
    assert run.launch(site, 1) == 0
    if entry != "step":
        site.check(f"f_tail/{entry}/one chain", entry.startswith("tag"), EPOCH_FWD)
    torch.cuda.synchronize()
    run.assert_untouched(f"f_tail/{entry}/one chain", chains=(1,))
    run.outs = run.outs[:1]
    run.check(f"f_tail/{entry}/one chain", chains[:1])


@pytest.mark.parametrize("entry", ("step", "tag"))
def test_activation_sweep(entry):
    """W_hh = 0, h0 = 0, T 1, H 64, B 128: the saved gates are the activations of the 8192 grid
    values, within eps_act of float64, saturating cleanly."""
    grid = R.activation_grid()
    H, B = 64, 128
    col = R.gate_cols(H)
    x = np.empty((1, B, 4 * H), np.float32)
    for q in range(4):
        x[0][:, col[q]] = grid.reshape(B, H)
    ch = dict(w=np.zeros((4 * H, H), np.float32), xproj=x, h0=np.zeros((B, H), np.float32),
              c0=np.zeros((B, H), np.float32), save_from=0, h32=True, gates=True)
    run = FwdRun(entry, [ch], B, 1, H)
    site = _fwd_site(entry, 1, B, H)
    assert run.launch(site, 1) == 0
    if entry != "step":
        site.check(f"sweep/{entry}", True, EPOCH_FWD)
    torch.cuda.synchronize()
    us, ut = R.check_activations(f"sweep/{entry}", run.outs[0]["gates"].host()[0], grid)
    uses = run.check(f"sweep/{entry}", [ch])
    _fig(f"{'sweep/' + entry:22s} sigmoid {us:.3f}  tanh {ut:.3f}  (c {uses['c']:.3f}  h32 {uses['h']:.3f})")


def _rand_chains(H, B, T, n, seed=5):
    rng = np.random.default_rng(seed)
    return [dict(w=R._weights(rng, H), xproj=rng.standard_normal((T, B, 4 * H)).astype(np.float32),
                 h0=(0.3 * rng.standard_normal((B, H))).astype(np.float32),
                 c0=(0.5 * rng.standard_normal((B, H))).astype(np.float32),
                 save_from=0, h32=True, gates=True) for _ in range(n)]


FWD_REFUSALS = [
    # what, entries, H, B allocated, B passed, chains allocated, chains passed, drop lo, code
    ("n_chains 0", FWD_ENTRIES, 64, 4, 4, 1, 0, False, -1),
    ("n_chains 5", FWD_ENTRIES, 64, 4, 4, 5, 5, False, -1),
    ("B 0", FWD_ENTRIES, 64, 1, 0, 1, 1, False, -1),
    ("H 96", FWD_ENTRIES, 96, 4, 4, 1, 1, False, -2),
    ("33 groups", ("tag", "tag_sp"), 64, 528, 528, 1, 1, False, -3),
    ("H 512 B 256 4 chains", ("persist",), 512, 256, 256, 4, 4, False, -3),
    ("missing lo pointer", ("tag_sp",), 64, 4, 4, 1, 1, True, -5),
]


@pytest.mark.parametrize("what", [r[0] for r in FWD_REFUSALS])
def test_forward_refusals(what):
    """Host-side returns before any launch: the documented code, and nothing written."""
    _, entries, H, B_alloc, B_pass, n_alloc, n_pass, drop_lo, code = next(r for r in FWD_REFUSALS if r[0] == what)
    chains = _rand_chains(H, B_alloc, 1, n_alloc)
    for entry in entries:
        run = FwdRun(entry, chains, B_alloc, 1, H, drop_lo=drop_lo)
        site = _fwd_site(entry, max(n_alloc, 1), B_alloc, H)
        rc = run.launch(site, n_pass, B=B_pass)
        assert rc == code, f"{what}/{entry}: return code {rc}, documented {code}"
        torch.cuda.synchronize()
        run.assert_untouched(f"{what}/{entry}")
        assert not site.ctr.any() and int(site.err.item()) == 0


# ---- backward --------------------------------------------------------------------------------

BWD_ENTRIES = ("step", "persist", "tag", "tag_sp")


def _bwd_expected_rc(entry, H, B):
    cus = int(kernels().r2_get_num_cus())
    nwg = H // 16
    if entry == "step":
        return -1 if B > 128 else 0
    if entry == "persist":
        mb = (B + 31) // 32
        return -3 if nwg * mb > cus or mb > 8 else 0
    mb = (B + 15) // 16
    if mb * nwg > cus or mb > 32:
        return -3
    return -11 if entry == "tag_sp" and H > 256 else 0


class BwdRun:
    """Device operands and poisoned outputs of one backward launch."""

    def __init__(self, entry, bw, drop_dgates_lo=False):
        self.entry, self.sp, self.bw = entry, entry == "tag_sp", bw
        H, B, T, t0 = bw["H"], bw["B"], bw["T"], bw["t0"]
        K, G, nwg = T - t0, 4 * H, H // 16
        ops = R.backward_operands(bw, self.sp)
        self.whhT = dev_bf16(R.pack_whh_t(ops["w_hi"]))
        self.whhT_lo = dev_bf16(R.pack_whh_t(ops["w_lo"])) if self.sp else None
        self.gates, self.cseq, self.c0 = dev(bw["gates"]), dev(bw["c_seq"]), dev(bw["c0"])
        self.dz = None
        if bw.get("dz_hi") is not None:
            # dh_ext is not read on the dz path: a NaN buffer shows it
            self.dh = torch.full((K, B, H), NAN, device=DEV)
            self.dz = [dev_bf16(bw[n]) for n in ("dz_hi", "dz_lo", "w1t_hi", "w1t_lo")]
        else:
            self.dh = dev(bw["dh_ext"]) if bw["dh_ext"] is not None else None
        row = max(PAD, B * G)      # one more step's rows of guard: dgates beyond T - t0 steps
        self.out = dict(dgates=_guarded((K, B, G), torch.bfloat16, pad=row))
        if self.sp and not drop_dgates_lo:
            self.out["dgates_lo"] = _guarded((K, B, G), torch.bfloat16, pad=row)
        if entry.startswith("tag"):
            self.out["db1"], self.out["db2"] = _guarded((G,)), _guarded((G,))
            self.bias_ws = torch.zeros((B + 15) // 16, G, device=DEV)
            self.perm = dev(R.gate_perm(H).astype(np.int32))
        elif entry == "step":
            self.s0 = torch.zeros(nwg, B, H, device=DEV)
            self.s1 = torch.zeros(nwg, B, H, device=DEV)
            self.dc = torch.zeros(B, H, device=DEV)
        else:
            self.slab = torch.zeros(2, nwg, B, H, device=DEV)

    def launch(self, site, opts=None, hg=None, no_perm=False, T=None, t0=None):
        k, bw, o = kernels(), self.bw, self.out
        B, H = bw["B"], bw["H"]
        T, t0 = bw["T"] if T is None else T, bw["t0"] if t0 is None else t0
        head = (ptr(self.dh), ptr(self.gates), ptr(self.cseq), ptr(self.c0), ptr(self.whhT))
        if self.entry == "step":
            return k.r2_lstm_bwd(*head, ptr(self.s0), ptr(self.s1), ptr(self.dc), o["dgates"].ptr(),
                                 B, T, t0, H, stream_handle())
        if self.entry == "persist":
            return k.r2_lstm_bwd_persist(*head, ptr(self.slab), o["dgates"].ptr(), B, T, t0, H,
                                         ptr(site.ctr), ptr(site.err), stream_handle())
        tail = (B, T, t0, H, ptr(site.ctr), ptr(site.err), ptr(site.ring), ptr(self.bias_ws),
                0 if no_perm else ptr(self.perm), o["db1"].ptr(), o["db2"].ptr())
        opts = opts if opts is not None else 0
        if self.sp:
            lo = o["dgates_lo"].ptr() if "dgates_lo" in o else 0
            if hg is not None:
                return k.r2_lstm_bwd_tag_sp_hg(*head, ptr(self.whhT_lo), o["dgates"].ptr(), lo, *tail,
                                               *hg, opts, stream_handle())
            return k.r2_lstm_bwd_tag_sp(*head, ptr(self.whhT_lo), o["dgates"].ptr(), lo, *tail, opts,
                                        stream_handle())
        return k.r2_lstm_bwd_tag(*head, o["dgates"].ptr(), *tail, *(hg if hg is not None else [0] * 11),
                                 opts, stream_handle())

    def dz_opts(self, kd=R.DZ_K):
        return bptt_opts(dz=ptr(self.dz[0]), dz_lo=ptr(self.dz[1]), w1t=ptr(self.dz[2]),
                         w1t_lo=ptr(self.dz[3]), kd=kd)

    def device_outputs(self):
        return [g.full.clone() for g in self.out.values()]

    def assert_untouched(self, label):
        for name, g in self.out.items():
            g.untouched(label, name)

    def check(self, label):
        o = self.out
        for name, g in o.items():
            g.owned(label, name)
        bits = o["dgates"].bits()
        out = dict(dgates_bits=bits, dgates=rn.bf16_val(bits))
        if self.sp:
            out["dgates_lo_bits"] = o["dgates_lo"].bits()
            out["dgates_lo"] = rn.bf16_val(out["dgates_lo_bits"])
        use, ref = R.check_backward(label, self.bw, out, self.sp)
        ub = 0.0
        if "db1" in o:
            out["db1"], out["db2"] = o["db1"].host(), o["db2"].host()
            ub = R.check_bias_grad(label, self.bw, out, ref)
        if self.bw["dh_ext"] is None and self.dz is None:     # b_nodh: exactly zero
            assert not out["dgates"].any() and ("db1" not in out or not out["db1"].any())
        return use, ub


def _bwd_site(entry, B, H):
    return Site(int(kernels().r2_lstm_bwd_tag_ring_bytes(B, H)) if entry.startswith("tag") else 0)


@pytest.mark.parametrize("entry", BWD_ENTRIES)
@pytest.mark.parametrize("name", [n for n in R.BACKWARD_CASES if n not in ("b_dz", "b_hg")])
def test_backward_case(name, entry):
    k = kernels()
    spec, bw0 = R.backward_case(name, 0)
    _, bw1 = R.backward_case(name, 1)
    H, B = spec["H"], spec["B"]
    label = f"{name}/{entry}"
    tagged = entry.startswith("tag")
    site = _bwd_site(entry, B, H)
    want_rc = _bwd_expected_rc(entry, H, B)
    run0 = BwdRun(entry, bw0)
    rc = run0.launch(site)
    assert rc == want_rc, f"{label}: return code {rc}, documented {want_rc}"
    if rc != 0:
        torch.cuda.synchronize()
        run0.assert_untouched(label)
        _fig(f"{label:22s} refused with {rc}, nothing written")
        return
    if entry != "step":
        site.check(label, tagged, EPOCH_BWD)
    torch.cuda.synchronize()
    use, ub = run0.check(label)
    first = run0.device_outputs()
    run1 = BwdRun(entry, bw1)
    assert run1.launch(site) == 0
    if entry != "step":
        site.check(label + "/launch1", tagged, EPOCH_BWD)
    torch.cuda.synchronize()
    u1, ub1 = run1.check(label + "/launch1")
    use, ub = max(use, u1), max(ub, ub1)
    variants = [(0, 0)] if entry == "step" else [(0, 0), (1, 0)]
    if tagged and name == "b_burn":
        variants.append((0, 1))
    try:
        for slow, pairs in variants:
            k.r2_lstm_persist_force_slow(slow)
            again = BwdRun(entry, bw0)
            assert again.launch(site, opts=bptt_opts(xcd_pairs=1) if pairs else None) == 0
            if entry != "step":
                site.check(f"{label}/force_slow{slow}/pairs{pairs}", tagged, EPOCH_BWD)
            torch.cuda.synchronize()
            for a, b in zip(first, again.device_outputs()):
                assert torch.equal(a.view(torch.int16), b.view(torch.int16)), \
                    f"{label}: outputs differ on a repeated launch (force_slow {slow}, xcd_pairs {pairs})"
    finally:
        k.r2_lstm_persist_force_slow(0)
    _fig(f"{label:22s} dgates {use:.3f}  db " + (f"{ub:.3f}" if tagged else "-    (not computed here)"))


def test_backward_dz_path():
    """b_dz: split precision with BpttOpts::dz (kd 512); dh_ext is a NaN buffer."""
    worst = [0.0, 0.0]
    site = _bwd_site("tag_sp", 17, 256)
    first = None
    for launch in (0, 1, 0):
        _, bw = R.backward_case("b_dz", launch)
        run = BwdRun("tag_sp", bw)
        assert run.launch(site, opts=run.dz_opts()) == 0
        site.check(f"b_dz/launch{launch}", True, EPOCH_BWD)
        use, ub = run.check(f"b_dz/tag_sp/launch{launch}")
        worst = [max(worst[0], use), max(worst[1], ub)]
        if first is None:
            first = run.device_outputs()
    for a, b in zip(first, run.device_outputs()):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), "b_dz: a repeated launch differs"
    _fig(f"{'b_dz/tag_sp':22s} dgates {worst[0]:.3f}  db {worst[1]:.3f}")


@pytest.mark.parametrize("A", [1, 9])
@pytest.mark.parametrize("entry", ("tag", "tag_sp"))
def test_backward_head_gradient_job(entry, A):
    """b_hg: the dueling head's gradient reduction on the launch's idle workgroups."""
    k = kernels()
    assert k.r2_lstm_bwd_tag_hg_ok(16, 256, 64) == 1
    sp = entry == "tag_sp"
    _, bw = R.backward_case("b_hg")
    hc = R.head_case(A)
    label = f"b_hg/{entry}/A{A}"
    plain = BwdRun(entry, bw)
    site = _bwd_site(entry, 16, 256)
    assert plain.launch(site) == 0
    site.check(label + "/plain", True, EPOCH_BWD)
    dva = dev(hc["dva"])
    if sp:
        hi, lo = rn.split_planes(hc["dz"])
        ins = [dva, dev(hc["zr"]), dev_bf16(hi), dev_bf16(lo)]
    else:
        ins = [dva, dev_bf16(rn.bf16_round(hc["zr"])), dev_bf16(rn.bf16_round(hc["dz"]))]
    outs = dict(gw2=_guarded((1 + A, 64)), gb2=_guarded((1 + A,)), gb1=_guarded((128,)))
    ws = torch.zeros(int(k.r2_gradsum_ws_floats()), device=DEV)
    ticket = torch.zeros(64, dtype=torch.int32, device=DEV)
    hg = [ptr(t) for t in ins] + [g.ptr() for g in outs.values()] + [hc["N"], A, 64, ptr(ws), ptr(ticket)]
    run = BwdRun(entry, bw)
    rc = run.launch(site, hg=hg)
    assert rc >= 0 and rc & 1, f"{label}: return value {rc}, bit 0 must be set"
    site.check(label, True, EPOCH_BWD)
    assert not ticket.any()
    use, ub = run.check(label)
    for a, b in zip(plain.device_outputs(), run.device_outputs()):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"{label}: the side job changed dgates / db"
    for name, g in outs.items():
        g.owned(label, name)
    uh = R.check_head_grads(label, hc, {n: g.host() for n, g in outs.items()}, sp)
    _fig(f"{label:22s} dgates {use:.3f}  db {ub:.3f}  head {uh:.3f}")


BWD_REFUSALS = ("t0 >= T", "stop_at < 0", "bias_ws without perm", "dz with kd 256", "dz at H 128",
                "dz through the bf16 entry", "sp without dgates_lo", "head job with HD 96")


@pytest.mark.parametrize("what", BWD_REFUSALS)
def test_backward_refusals(what):
    """Host-side returns before any launch: the code as written in lstm_bptt.hip, nothing written."""
    _, bw = R.backward_case("b_dz" if what.startswith("dz") and "128" not in what else "b_burn")
    if what == "dz at H 128":      # b_burn's shape with dz operands of the matching width
        rng = np.random.default_rng(3)
        K = bw["T"] - bw["t0"]
        bw["dz_hi"], bw["dz_lo"] = rn.split_planes((0.2 * rng.standard_normal((K * bw["B"], R.DZ_K))).astype(np.float32))
        bw["w1t_hi"], bw["w1t_lo"] = rn.split_planes((0.2 * rng.standard_normal((bw["H"], R.DZ_K))).astype(np.float32))
    entry = "tag" if what in ("dz through the bf16 entry", "bias_ws without perm") else "tag_sp"
    run = BwdRun(entry, bw, drop_dgates_lo=what == "sp without dgates_lo")
    site = _bwd_site(entry, bw["B"], bw["H"])
    extra = {}
    if what == "t0 >= T":
        rc, code = run.launch(site, t0=bw["T"]), -1
    elif what == "stop_at < 0":
        rc, code = run.launch(site, opts=bptt_opts(stop_at=-1)), -1
    elif what == "bias_ws without perm":
        rc, code = run.launch(site, no_perm=True), -1
    elif what == "dz with kd 256":
        rc, code = run.launch(site, opts=run.dz_opts(kd=256)), -1
    elif what in ("dz at H 128", "dz through the bf16 entry"):
        rc, code = run.launch(site, opts=run.dz_opts()), -13
    elif what == "sp without dgates_lo":
        rc, code = run.launch(site), -5
    else:
        _, bw = R.backward_case("b_hg")
        run, site = BwdRun("tag", bw), _bwd_site("tag", 16, 256)
        extra = {n: _guarded((4096,)) for n in ("dva", "zr", "dz", "gw2", "gb2", "gb1", "ws", "ticket")}
        hg = [extra[n].ptr() for n in ("dva", "zr", "dz", "gw2", "gb2", "gb1")] + [40, 9, 96,
                                                                                  extra["ws"].ptr(), extra["ticket"].ptr()]
        rc, code = run.launch(site, hg=hg), -5
    assert rc == code, f"{what}: return code {rc}, lstm_bptt.hip says {code}"
    torch.cuda.synchronize()
    run.assert_untouched(what)
    for name, g in extra.items():
        g.untouched(what, name)
    assert not site.ctr.any() and int(site.err.item()) == 0
