"""The split-precision LSTM step kernel (csrc/kernels/lstm_step_sp.hip, r2_lstm_fwd_sp) against the
teacher-forced float64 oracle (pytorch_r2d2_amd/lstm_ref.py check_forward, sp=True): per-element
bounds, the bound-free checks (the h planes are the roundings of h32 bit for bit, c matches the
saved gates), write ownership under NaN poison, continuation from t_begin, and the launcher's
refusals.  The cases are lstm_ref.STEP_SP_CASES, which tests/test_lstm_step_sp_cpu.py runs through
the fp32 emulation."""
import numpy as np
import pytest
import torch

from gpu_support import Guarded, dev, dev_bf16
from gpu_support import stop_after_a_gpu_error  # noqa: F401
from pytorch_r2d2_amd import lstm_ref as R
from pytorch_r2d2_amd import refnum as rn
from pytorch_r2d2_amd.ops._lib import kernels, ptr, stream_handle

pytestmark = pytest.mark.gpu
PAD = 256


def _fig(line):
    print("lstm-step-sp: " + line)


def _guarded(shape, dtype=torch.float32, pad=PAD):
    return Guarded(shape, dtype, pad)


class StepRun:
    """Device operands and poisoned outputs of one r2_lstm_fwd_sp launch site.  Chains that share
    a net (``halves``) are row ranges of that net's buffers, addressed by pointer offsets."""

    def __init__(self, chains, B, T, H, rows=None, drop=None):
        self.chains, self.B, self.T, self.H = chains, B, T, H
        self.loose = rows is not None
        assert rows is None or T == 1
        G = 4 * H
        nets = sorted({ch.get("net", i) for i, ch in enumerate(chains)})
        self.nets, self.gates, self.inputs, words = {}, [], [], []
        for n in nets:
            mine = [ch for i, ch in enumerate(chains) if ch.get("net", i) == n]
            NR = rows or B * len(mine)
            assert len(mine) == 1 or T == 1, "row halves are pointer offsets into (1, rows, .) buffers"
            pad_rows = [np.zeros((NR - B * len(mine),) + s, np.float32) for s in ((H,), (H,))]
            ops = R.forward_operands(mine[0], True)
            x = np.concatenate([ch["xproj"] for ch in mine] +
                               [np.zeros((T, NR - B * len(mine), G), np.float32)], axis=1)
            self.nets[n] = dict(
                w_hi=dev_bf16(ops["w_hi"]), w_lo=dev_bf16(ops["w_lo"]), x=dev(x),
                h0=dev(np.concatenate([ch["h0"] for ch in mine] + pad_rows[:1])),
                c0=dev(np.concatenate([ch["c0"] for ch in mine] + pad_rows[1:])),
                h_seq=_guarded((T, NR, H), torch.bfloat16), h_seq_lo=_guarded((T, NR, H), torch.bfloat16),
                c_seq=_guarded((T, NR, H)), h32=_guarded((T, NR, H)) if mine[0]["h32"] else None, NR=NR)
            self.inputs += [(f"net{n}/{k}", self.nets[n][k], self.nets[n][k].clone())
                            for k in ("h0", "c0", "x", "w_hi", "w_lo")]
        for i, ch in enumerate(chains):
            N = self.nets[ch.get("net", i)]
            r0, sf = ch.get("row0", 0), int(ch["save_from"])
            g = _guarded((max(T - sf, 0), B, G), pad=max(PAD, B * G)) if ch["gates"] else None
            self.gates.append(g)
            w = [ptr(N["x"]) + r0 * G * 4, ptr(N["w_hi"]), ptr(N["h0"]) + r0 * H * 4,
                 ptr(N["c0"]) + r0 * H * 4, N["h_seq"].ptr(r0 * H), N["c_seq"].ptr(r0 * H),
                 N["h32"].ptr(r0 * H) if N["h32"] else 0, g.ptr() if g else 0, sf,
                 0 if drop == "whh_lo" else ptr(N["w_lo"]),
                 0 if drop == "h_seq_lo" else N["h_seq_lo"].ptr(r0 * H)]
            words += w
        self.arr = np.asarray(words, dtype=np.int64)

    def launch(self, n_chains=None, B=None, T=None, t_begin=0, H=None):
        return kernels().r2_lstm_fwd_sp(self.arr.ctypes.data, len(self.chains) if n_chains is None else n_chains,
                                        self.B if B is None else B, self.T if T is None else T,
                                        self.H if H is None else H, t_begin, stream_handle())

    def buffers(self):
        out = [(f"net{n}/{k}", N[k]) for n, N in self.nets.items()
               for k in ("h_seq", "h_seq_lo", "c_seq", "h32") if N[k] is not None]
        return out + [(f"chain{i}/gates", g) for i, g in enumerate(self.gates) if g is not None]

    def device_outputs(self):
        return [g.full.clone() for _, g in self.buffers()]

    def assert_untouched(self, label, only=None):
        for name, g in self.buffers():
            if only is None or name.startswith(only):
                g.untouched(label, name)

    def assert_inputs_untouched(self, label):
        for name, t, before in self.inputs:
            assert torch.equal(t.view(torch.int16), before.view(torch.int16)), f"{label}: {name} was written"

    def check(self, label, B=None):
        """Ownership (rows >= B of a net's buffers stay poison), then every oracle check; returns
        the largest use of each bound."""
        B = self.B if B is None else B
        worst = dict(gates=0.0, c=0.0, h=0.0, h_seq=0.0)
        for n, N in self.nets.items():
            k = sum(1 for i, ch in enumerate(self.chains) if ch.get("net", i) == n)
            valid = np.zeros((self.T, N["NR"], self.H), bool)
            if self.loose:      # launched with fewer rows than allocated: (T = 1) the first B rows
                valid.reshape(-1)[: B * self.H] = True
            else:
                assert N["NR"] == B * k
                valid[:] = True
            for name in ("h_seq", "h_seq_lo", "c_seq", "h32"):
                if N[name] is not None:
                    N[name].owned(f"{label}/net{n}", name, valid)
        for i, (ch, g) in enumerate(zip(self.chains, self.gates)):
            lab = f"{label}/chain{i}"
            N = self.nets[ch.get("net", i)]
            r0 = ch.get("row0", 0)
            if g is not None:
                g.owned(lab, "gates")

            def cut(a, NR=N["NR"], r0=r0):
                if self.loose:      # launched on the first B rows of a larger (T = 1) buffer
                    return np.ascontiguousarray(a.reshape(-1)[: B * self.H].reshape(1, B, self.H))
                return np.ascontiguousarray(a.reshape(self.T, NR, self.H)[:, r0:r0 + B])
            bits, lo_bits = cut(N["h_seq"].bits()), cut(N["h_seq_lo"].bits())
            out = dict(h_seq_bits=bits, h_seq=rn.bf16_val(bits), h_seq_lo_bits=lo_bits,
                       h_seq_lo=rn.bf16_val(lo_bits), c_seq=cut(N["c_seq"].host()))
            if N["h32"] is not None:
                out["h32"] = cut(N["h32"].host())
            if g is not None:
                out["gates"] = g.host()
            uses = R.check_forward(lab, ch, out, sp=True)
            worst = {m: max(worst[m], uses[m]) for m in worst}
        return worst


@pytest.mark.parametrize("name", list(R.STEP_SP_CASES))
def test_step_case(name):
    spec, chains = R.step_sp_case(name)
    H, B, T = spec["H"], spec["B"], spec["T"]
    run = StepRun(chains, B, T, H)
    assert run.launch() == 0
    torch.cuda.synchronize()
    uses = run.check(name)
    run.assert_inputs_untouched(name)
    again = StepRun(chains, B, T, H)
    assert again.launch() == 0
    torch.cuda.synchronize()
    for a, b in zip(run.device_outputs(), again.device_outputs()):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"{name}: a repeated launch differs"
    _fig(f"{name:10s} gates {uses['gates']:.3f}  c {uses['c']:.3f}  h32 {uses['h']:.3f}  h_seq {uses['h_seq']:.3f}")
    assert max(uses.values()) <= 1.0


def test_continuation_from_t_begin():
    """s_tile2 (T 3): steps 0, 1 in one call and step 2 in a second call (t_begin 2) leave exactly
    what one call over all three steps leaves, and it passes the oracle."""
    spec, chains = R.step_sp_case("s_tile2")
    H, B, T = spec["H"], spec["B"], spec["T"]
    whole = StepRun(chains, B, T, H)
    assert whole.launch() == 0
    parts = StepRun(chains, B, T, H)
    assert parts.launch(T=2) == 0
    torch.cuda.synchronize()
    # after the first call step 2's rows are still poison
    for n, N in parts.nets.items():
        assert torch.isnan(N["c_seq"].body.reshape(T, B, H)[2]).all()
        assert not torch.isnan(N["c_seq"].body.reshape(T, B, H)[:2]).any()
    assert parts.launch(T=3, t_begin=2) == 0
    torch.cuda.synchronize()
    parts.check("s_tile2/continued")
    for (name, _), a, b in zip(whole.buffers(), whole.device_outputs(), parts.device_outputs()):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"continuation: {name} differs"


def test_rows_past_B_and_neighbouring_chain_are_left_alone():
    """s_clamp's operands in 12-row buffers launched with B = 5 (rows 5.. stay poison, the clamped
    tile rows write nothing); s_tile2 launched with one chain (the second chain's buffers stay
    poison)."""
    spec, chains = R.step_sp_case("s_clamp")
    run = StepRun(chains, spec["B"], 1, spec["H"], rows=12)
    assert run.launch() == 0
    torch.cuda.synchronize()
    run.check("s_clamp/12-row buffers")
    run.assert_inputs_untouched("s_clamp/12-row buffers")
    spec, chains = R.step_sp_case("s_tile2")
    run = StepRun(chains, spec["B"], spec["T"], spec["H"])
    assert run.launch(n_chains=1) == 0
    torch.cuda.synchronize()
    run.assert_untouched("s_tile2/one chain", only="net1")
    run.assert_untouched("s_tile2/one chain", only="chain1")
    one = StepRun(chains[:1], spec["B"], spec["T"], spec["H"])
    one.nets, one.gates = {0: run.nets[0]}, run.gates[:1]
    one.check("s_tile2/one chain")


def _rand_chains(H, B, n, seed=5):
    rng = np.random.default_rng(seed)
    return [dict(w=R._weights(rng, H), xproj=rng.standard_normal((1, B, 4 * H)).astype(np.float32),
                 h0=(0.3 * rng.standard_normal((B, H))).astype(np.float32),
                 c0=(0.5 * rng.standard_normal((B, H))).astype(np.float32),
                 save_from=0, h32=True, gates=True) for _ in range(n)]


REFUSALS = [
    # what, H, B allocated, B passed, chains allocated, chains passed, dropped pointer, code
    ("n_chains 0", 64, 4, 4, 1, 0, None, -1),
    ("n_chains 5", 64, 4, 4, 5, 5, None, -1),
    ("B 0", 64, 1, 0, 1, 1, None, -1),
    ("B 129", 64, 129, 129, 1, 1, None, -1),
    ("H 96", 96, 4, 4, 1, 1, None, -2),
    ("H 512", 512, 4, 4, 1, 1, None, -2),
    ("missing whh_lo", 64, 4, 4, 2, 2, "whh_lo", -5),
    ("missing h_seq_lo", 64, 4, 4, 2, 2, "h_seq_lo", -5),
]


@pytest.mark.parametrize("what", [r[0] for r in REFUSALS])
def test_refusals(what):
    """Host-side returns before any launch: the documented code, and nothing written."""
    _, H, B_alloc, B_pass, n_alloc, n_pass, drop, code = next(r for r in REFUSALS if r[0] == what)
    run = StepRun(_rand_chains(H, B_alloc, n_alloc), B_alloc, 1, H, drop=drop)
    rc = run.launch(n_chains=n_pass, B=B_pass)
    assert rc == code, f"{what}: return code {rc}, documented {code}"
    torch.cuda.synchronize()
    run.assert_untouched(what)
    run.assert_inputs_untouched(what)
