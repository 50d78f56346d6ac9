"""Device scaffolding the GPU oracle tests share: poisoned, guard-banded buffers, host <-> device
helpers, the stop-after-a-GPU-error rule, the report files, and the float64 QNet step.

A plain module (not collected, not a conftest).  A new oracle test starts from here and from
pytorch_r2d2_amd/refnum.py: it brings a case table and a reference.  tests/test_gpu_support_cpu.py
pins the buffers' semantics on the CPU device."""
import os

import numpy as np
import pytest
import torch

from pytorch_r2d2_amd import refnum
from pytorch_r2d2_amd import replay_ref as rr
from pytorch_r2d2_amd.actor_batched import PackedWeights
from pytorch_r2d2_amd.config import get_config
from pytorch_r2d2_amd.engine.layout import ParamLayout
from pytorch_r2d2_amd.envs.synthetic import VecSyntheticAtari
from pytorch_r2d2_amd.models import QNet
from pytorch_r2d2_amd.ops._lib import kernels, stream_handle

DEV = "cuda"
NAN = float("nan")
G = 16          # guard elements at each end of a Buf


# ---- fixtures -----------------------------------------------------------------------------------

@pytest.fixture(autouse=True)
def stop_after_a_gpu_error():
    """A launch that faulted leaves the device in an error state: nothing more is launched.
    Autouse in every module that imports it by name."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU error, no further launches: {e}", returncode=3)


def report_fixture(env_var, header, fmt=None):
    """(lines, fixture): a module-scoped autouse fixture that on teardown writes ``header`` and then
    every entry of ``lines`` (through ``fmt % entry`` if given) to the file ``env_var`` names."""
    lines = []

    @pytest.fixture(scope="module", autouse=True)
    def report():
        yield
        path = os.environ.get(env_var)
        if path and lines:
            with open(path, "w") as f:
                f.write(header)
                for line in lines:
                    f.write((fmt % line if fmt else line) + "\n")

    return lines, report


# ---- NaN-poisoned output buffers (write ownership per element) ----------------------------------

class Guarded:
    """An output buffer between two guard bands, all NaN poison before the launch."""

    def __init__(self, shape, dtype, pad, device=DEV):
        self.shape, self.pad = tuple(shape), (pad + 7) // 8 * 8
        self.n = int(np.prod(self.shape))
        self.full = torch.full((self.n + 2 * self.pad,), NAN, dtype=dtype, device=device)
        self.body = self.full[self.pad:self.pad + self.n]

    def ptr(self, elem=0):     # (an empty body still has an address: data_ptr() of an empty view is null)
        return self.full.data_ptr() + (self.pad + elem) * self.full.element_size()

    def host_full(self):
        return self.full.float().cpu().numpy()

    def host(self):
        return self.body.float().cpu().numpy().reshape(self.shape)

    def bits(self):
        if self.full.dtype == torch.bfloat16:
            return self.body.view(torch.int16).cpu().numpy().view(np.uint16).reshape(self.shape)
        return self.body.view(torch.int32).cpu().numpy().view(np.uint32).reshape(self.shape)

    def owned(self, label, name, valid=None):
        refnum.check_ownership(label, name, self.host_full(), self.pad, valid)

    def untouched(self, label, name):
        refnum.check_untouched(label, name, self.host_full())


# ---- bit-exact buffers of any dtype (guards and untouched cells keep their bytes) ---------------

class Buf:
    """A device buffer between two runs of G guard elements; ``p`` points at the body."""

    def __init__(self, body, poison, device=DEV):
        if not torch.is_tensor(body):
            body = torch.from_numpy(np.ascontiguousarray(body))
        body = body.reshape(-1)
        g = torch.full((G,), poison, dtype=body.dtype)
        self.full = torch.cat([g, body, g]).to(device)
        self.init = self.full.clone()
        self.n = body.numel()

    @classmethod
    def poisoned(cls, n, dtype, poison, device=DEV):
        return cls(torch.full((n,), poison, dtype=dtype), poison, device)

    @property
    def p(self):
        return self.full.data_ptr() + G * self.full.element_size()

    @staticmethod
    def _bytes(t):
        return t.detach().cpu().contiguous().view(torch.uint8).reshape(-1).numpy()

    def bits(self):
        """Bytes of the body."""
        return self._bytes(self.full[G: G + self.n])

    def body(self):
        return self.full[G: G + self.n].cpu().numpy()

    def tail(self, init=False):
        """Body and back guard (leaf i at index i)."""
        return (self.init if init else self.full)[G:].cpu().numpy()

    def assert_guards(self, what=""):
        a, b = self._bytes(self.full), self._bytes(self.init)
        e = G * self.full.element_size()
        assert np.array_equal(a[:e], b[:e]), f"{what}: front guard overwritten"
        assert np.array_equal(a[-e:], b[-e:]), f"{what}: back guard overwritten"

    def assert_untouched(self, what=""):
        assert np.array_equal(self._bytes(self.full), self._bytes(self.init)), f"{what}: written"


def buf_from_host(a):
    """A guarded device buffer that starts as the host array ``a`` (guards: the dtype's poison)."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:        # bf16 bit patterns
        return Buf(torch.from_numpy(a.view(np.int16).reshape(-1)).view(torch.bfloat16), NAN)
    poison = NAN if a.dtype.kind == "f" else (0xAB if a.dtype == np.uint8 else -1)
    return Buf(a.reshape(-1), poison)


def i64(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.int64))


def word(v, dtype=torch.int32):
    return torch.tensor([v], dtype=dtype, device=DEV)


class Tree:
    """A guarded device tree over ``leaves``, rebuilt by r2_tree_rebuild and checked."""

    def __init__(self, leaves):
        self.leaves = np.asarray(leaves, dtype=np.float32)
        offs, sizes = rr.tree_geometry(self.leaves.size)
        self.offs, self.sizes, self.levels = i64(offs), i64(sizes), len(sizes)
        body = np.full(offs[-1] + sizes[-1], np.nan, dtype=np.float32)
        body[: self.leaves.size] = self.leaves
        self.buf = Buf(body, NAN)
        assert kernels().r2_tree_rebuild(*self.geom(), stream_handle()) == 0
        torch.cuda.synchronize()
        self.check()
        self.buf.init = self.buf.full.clone()

    def geom(self):
        return self.buf.p, self.offs.ctypes.data, self.sizes.ctypes.data, self.levels

    def host(self):
        return self.buf.body()

    def root(self):
        return float(self.host()[self.offs[-1]])

    def check(self, leaves=None):
        self.buf.assert_guards("tree")
        return rr.check_tree(self.host(), self.offs.tolist(), self.sizes.tolist(), leaves)


# ---- host <-> device ----------------------------------------------------------------------------

def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def dev_bf16(a):
    """fp32 values that are exact in bf16 -> a bf16 tensor with those bits."""
    return dev(refnum.bf16_bits(a).view(np.int16)).view(torch.bfloat16)


def np_copy(t):
    return t.detach().cpu().numpy().copy()


def split_bf16(x):
    """hi / lo bf16 planes of an fp32 tensor (csrc/split.h)."""
    hi = x.to(torch.bfloat16)
    return hi, (x - hi.float()).to(torch.bfloat16)


def rel_err(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


def rand_operand(rows, cols, kmajor, gen):
    """A (rows, cols) fp32 view that is row-contiguous (kmajor) or column-contiguous."""
    x = torch.randn(rows, cols, generator=gen, device=gen.device)
    return x if kmajor else x.t().contiguous().t()


# ---- nets, envs, configs ------------------------------------------------------------------------

def packed_weights(cfg, seed, split=False):
    """(net, w): a seeded CPU QNet and its packed device copy."""
    torch.manual_seed(seed)
    net = QNet("cpu", cfg.model, cfg.env)
    w = PackedWeights(ParamLayout(cfg.model, cfg.env), DEV, split=split)
    w.load(net.state_dict())
    return net, w


class LogEnv(VecSyntheticAtari):
    """The env's outputs stay in its persistent buffers until the next step."""

    def outputs(self):
        return np_copy(self._reward), np_copy(self._done), np_copy(self._finished)


def pong_small(**over):
    kw = {"replay.burn_in": 4, "replay.learn": 6, "replay.overlap": 5, "replay.n_step": 3,
          "learner.batch_size": 8, "actor.envs_per_actor": 16, "env.episode_len": 12,
          "eval.envs": 4, "eval.episodes_per_env": 2}
    kw.update(over)
    return get_config("pong", **kw)


def train_with_evals(evaluate, **over):
    """The engine of smoke() (batch 4, burn-in 4, learn 4, 4 sub-rings, fill_synthetic), 6 learner
    steps; ``evaluate``: an evaluation of the live weights after every step.  Returns
    (replay, engine, the evaluations' mean returns)."""
    from pytorch_r2d2_amd.actor_batched import engine_weights
    from pytorch_r2d2_amd.engine.learner_engine import LearnerEngine
    from pytorch_r2d2_amd.engine.replay_hbm import HBMReplay
    from pytorch_r2d2_amd.evaluator import BatchedEvaluator, make_eval_env
    cfg = get_config("atari57", **{"learner.batch_size": 4, "replay.capacity": 8192, "replay.n_subrings": 4,
                                   "replay.burn_in": 4, "replay.learn": 4, "replay.overlap": 4,
                                   "learner.use_graph": False, "env.episode_len": 8, **over})
    torch.manual_seed(0)
    rp = HBMReplay(cfg, torch.device(DEV, 0))
    rp.fill_synthetic(episode_len=64, seed=0)
    eng = LearnerEngine(cfg, rp, torch.device(DEV, 0))
    ev = None
    if evaluate:
        ev = BatchedEvaluator(cfg, make_eval_env(cfg, DEV, 4), engine_weights(eng)[0], episodes_per_env=1)
        assert ev.infer.sp == (cfg.eval.compute_dtype == "fp32")
    means = []
    for _ in range(6):
        eng.step()
        if ev is not None:
            res = ev.run()
            assert res["complete"] and res["episodes"] == 4
            means.append(res["mean_return"])
    torch.cuda.synchronize()
    assert eng.error_word() == 0
    return rp, eng, means


def engine_state(rp, eng):
    """Everything a learner step leaves behind, by name: weights, moments, priority, tree, step,
    loss and the packed layouts (their alignment padding is never read and not compared)."""
    out = {"master": eng.master, "target": eng.target, "opt_a": eng.opt_a, "opt_b": eng.opt_b,
           "lstm_b": eng.lstm_b, "lstm_b_t": eng.lstm_b_t, "priority": rp.priority,
           "tree": rp.tree, "step": rp.step, "loss": eng.loss}
    for tag, (bf, f32) in {"": (eng.bf, eng.f32), "_t": (eng.bf_t, eng.f32_t)}.items():
        for plane in range(bf.shape[0]):
            for k, v in eng.layout.packed_views(bf[plane], f32).items():
                out["%s%s.%d" % (k, tag, plane)] = v
    return out


def bf16_as_f64(x):
    return x.float().bfloat16().double()


def qnet64(net, frames, h, c, rounded):
    """Q, h', c' of one step of ``net`` in float64; ``rounded``: GEMM operands (conv / LSTM / first
    head layer weights, the activations entering them) and the carried h rounded to bf16 where the
    kernels round them (1 / 255 and every bias applied to the wide accumulator): the emulation of
    the bf16 inference path."""
    sd = {k: v.double() for k, v in net.state_dict().items()}
    w = (lambda k: bf16_as_f64(sd[k])) if rounded else (lambda k: sd[k])
    r = bf16_as_f64 if rounded else (lambda x: x)
    F = torch.nn.functional
    x = frames.double().view(-1, *net.in_shape)
    a = r(torch.relu(F.conv2d(x, w("vis_layers.0.weight"), None, stride=4) / 255.0
                     + sd["vis_layers.0.bias"][None, :, None, None]))
    a = r(torch.relu(F.conv2d(a, w("vis_layers.2.weight"), sd["vis_layers.2.bias"], stride=2)))
    a = r(torch.relu(F.conv2d(a, w("vis_layers.4.weight"), sd["vis_layers.4.bias"], stride=1)))
    feat = a.reshape(a.shape[0], -1)
    bias = (net.lstm.bias_ih.detach() + net.lstm.bias_hh.detach()).double() if rounded else \
        sd["lstm.bias_ih"] + sd["lstm.bias_hh"]
    gates = feat @ w("lstm.weight_ih").t() + bias + r(h.double()) @ w("lstm.weight_hh").t()
    i, f, g, o = gates.chunk(4, dim=1)
    c2 = torch.sigmoid(f) * c.double() + torch.sigmoid(i) * torch.tanh(g)
    h2 = torch.sigmoid(o) * torch.tanh(c2)
    hin = r(h2)
    zv = r(hin @ w("val.0.weight").t())          # the first head layer is stored before its bias
    za = r(hin @ w("adv.0.weight").t())
    v = torch.relu(zv + sd["val.0.bias"]) @ sd["val.2.weight"].t() + sd["val.2.bias"]
    adv = torch.relu(za + sd["adv.0.bias"]) @ sd["adv.2.weight"].t() + sd["adv.2.bias"]
    return v + adv - adv.mean(dim=1, keepdim=True), h2, c2
