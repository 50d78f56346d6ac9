"""The acting path: Q values and the next recurrent state of one or two nets for E envs.

``PolicyInference`` owns the buffers, the settings and the launches that ``BatchedActor`` (nets
"on" and "tg") and ``BatchedEvaluator`` (net "on") share: one launch per stage for ALL nets (torso
multi-job, x-projection GEMM, one LSTM step launch with a chain per net, head GEMM, dueling
epilogue) -- the step is launch-bound at these batch sizes.  It reads weights as ``NetWeights``.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np
import torch

from .config import R2D2Config
from .engine.layout import ParamLayout
from .ops import jobs
from .ops._lib import check, kernels, stream_handle
from .ops.gemm import G5_CFGS, Gemm, gemm, gemm_sp, gemm_sp_ws_bytes
from .ops.torso_lib import (fused_torso_fwd_geom, fused_torso_supported, torso_forward_library,
                            torso_fwd_fused)


@dataclass
class NetWeights:
    """What inference reads of one net (``engine_weights`` returns two; ``PackedWeights`` has the
    same fields): ``pk`` the packed views (the hi planes), ``pk_lo`` the lo planes (``None``
    without split precision), ``lstm_b`` = b_ih + b_hh, ``flat`` the fp32 master."""
    pk: Dict[str, torch.Tensor]
    pk_lo: Optional[Dict[str, torch.Tensor]]
    lstm_b: torch.Tensor
    flat: torch.Tensor


COMPUTE_DTYPES = ("bf16", "fp32")


def check_compute_dtype(knob: str, value, cfg: R2D2Config, nets=()) -> bool:
    """Validate an inference ``compute_dtype`` knob (``actor.compute_dtype`` /
    ``eval.compute_dtype``) against the configuration and the weights it would read; True for
    fp32.  Every refusal is a ``ValueError`` that names the knob."""
    if value not in COMPUTE_DTYPES:
        raise ValueError(f"{knob} must be 'bf16' or 'fp32', not {value!r}")
    if value != "fp32":
        return False
    if not fused_torso_supported(cfg.env, cfg.model):
        e = cfg.env
        raise ValueError(f"{knob}=fp32 needs the fused split-precision torso (conv torso on 4x84x84 "
                         f"frames), not torso {cfg.model.torso!r} on "
                         f"{e.channels_per_frame * e.n_stacks}x{e.frame_h}x{e.frame_w}")
    if cfg.model.hidden not in (64, 128, 256):
        raise ValueError(f"{knob}=fp32: the split-precision LSTM step covers model.hidden 64, 128 "
                         f"or 256, not {cfg.model.hidden}")
    for w in nets:
        if w.pk_lo is None:
            raise ValueError(f"{knob}=fp32 reads hi / lo weight planes; these weights have no lo planes "
                             "(a bf16 learner's live weights, or PackedWeights without split=True)")
    return True


class PolicyInference:
    def __init__(self, cfg: R2D2Config, env, keys, knob: str, device):
        """``keys``: the nets' names (("on", "tg") for the actor, ("on",) for the evaluator);
        ``knob``: "actor.compute_dtype" / "eval.compute_dtype", the setting that picks the
        precision.  The owner has checked it against its weights (``check_compute_dtype``)."""
        self.cfg, self.env, self.keys = cfg, env, tuple(keys)
        self.sp = check_compute_dtype(knob, getattr(cfg, knob.split(".")[0]).compute_dtype, cfg)
        self.device = d = torch.device(device)
        m = cfg.model
        self.E = E = int(env.E)
        self.H, self.A = H, A = m.hidden, m.n_actions
        self.layout = L = ParamLayout(m, cfg.env)
        # fused torso forward: Atari 4x84x84 and DMLab-30 3x72x96 (else the library convs)
        self.fwd_geom = fused_torso_fwd_geom(cfg.env, m) if d.type == "cuda" else None
        self.fused_torso = self.fwd_geom is not None
        # Both may be set after construction; a graph captured before keeps the old value (it is
        # not invalidated), so set them before ``capture``.
        self.lstm_step = False       # bf16: the plain step kernel instead of the persistent one
        self.n_workers = 256         # torso workgroups (grid-stride over frames) / split-GEMM CUs
        bf = torch.bfloat16
        z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=d)  # noqa: E731
        per_key = lambda *s, dt=torch.float32: {k: z(*s, dt=dt) for k in self.keys}  # noqa: E731
        # recurrent state of every net: bf16 h (MFMA operand), fp32 h (stored state), fp32 c
        self.h_bf, self.h32, self.c = per_key(E, H, dt=bf), per_key(E, H), per_key(E, H)
        self.h_bf_new, self.h32_new, self.c_new = per_key(E, H, dt=bf), per_key(E, H), per_key(E, H)
        self.q = per_key(E, A)
        self.Xn, self.xp = per_key(E, L.D, dt=bf), per_key(E, L.G)
        # head pre-activations: fp32 out of the split-precision GEMM, else bf16
        self.zh = per_key(E, 2 * L.HD, dt=torch.float32 if self.sp else bf)
        self.ctr = z(int(kernels().r2_lstm_persist_ctr_words()), dt=torch.int32)
        self.err = z(1, dt=torch.int32)
        # job arrays of the last ``run``: the launchers read them, so they outlive a capture
        self._tjobs = self._chains = self._djobs = None
        if not self.sp:
            return
        # fp32 only: lo planes of the torso features and of the new h, and the split-K workspace +
        # tickets of the two GEMM sites (``gemm_sp`` must not allocate inside a capture)
        self.Xn_lo, self.h_lo_new = per_key(E, L.D, dt=bf), per_key(E, H, dt=bf)
        self.sp_ws = {}
        if d.type != "cuda":
            return
        # sized for the automatic K splits of any CU count the group may be given (n_workers)
        for site, (K, N) in (("xproj", (L.D, L.G)), ("heads", (H, 2 * L.HD))):
            a, b, c = z(E, K, dt=bf), z(N, K, dt=bf).t(), z(E, N)
            probs = [Gemm(a, b, c, a_lo=a, b_lo=b) for _ in self.keys]
            need = max(gemm_sp_ws_bytes(probs, [0] * len(probs), tile, n_cus)
                       for tile in range(len(G5_CFGS)) for n_cus in range(8, 257, 8))
            self.sp_ws[site] = (z(max(need // 4, 1)), z(4096, dt=torch.int32))

    def zero_state(self) -> None:
        """Forget the carried recurrent state of every net."""
        for key in self.keys:
            self.h_bf[key].zero_()
            self.h32[key].zero_()
            self.c[key].zero_()

    def run(self, nets) -> None:
        """Q values (``q``) + next recurrent state (``h_bf_new``, ``h32_new``, ``c_new``) of every
        net of ``nets`` ((key, NetWeights) pairs) for the current observations of the env."""
        if self.sp:
            self._run_fp32(nets)
        else:
            self._run_bf16(nets)

    def _step_chains(self, nets, h0, halves: bool, lo: bool = False) -> int:
        """The LSTM launch's chain rows into ``_chains``: one per net reading ``h0`` (bf16
        ``h_bf`` or fp32 ``h32``), or (``halves``: the step kernels, <= 128 rows per chain) one per
        net and row half when E > 128.  Returns the rows per chain."""
        E, H, G = self.E, self.H, self.layout.G
        Bc = E if E <= 128 or not halves else (E + 1) // 2
        if halves and E > 128 and (E % 2 or Bc > 128):
            raise ValueError("step-kernel LSTM: E <= 128 or an even E <= 256")
        rows = []
        for key, w in nets:
            hb = h0[key].element_size()
            for r0 in range(0, E, Bc):      # byte offsets of row r0 in each (E, .) buffer
                rows.append(jobs.lstm_chain(
                    xproj=self.xp[key].data_ptr() + r0 * G * 4, whh=w.pk["w_hh"].data_ptr(),
                    h0=h0[key].data_ptr() + r0 * H * hb, c0=self.c[key].data_ptr() + r0 * H * 4,
                    h_seq=self.h_bf_new[key].data_ptr() + r0 * H * 2,
                    c_seq=self.c_new[key].data_ptr() + r0 * H * 4,
                    h32=self.h32_new[key].data_ptr() + r0 * H * 4,
                    whh_lo=w.pk_lo["w_hh"].data_ptr() if lo else 0,
                    h_lo=self.h_lo_new[key].data_ptr() + r0 * H * 2 if lo else 0))
        self._chains = np.asarray(rows, dtype=np.int64)
        return Bc

    def _duel_jobs(self, nets) -> None:
        self._djobs = np.asarray(
            [jobs.duel_job(z=self.zh[key].data_ptr(), pk=w.pk, q=self.q[key].data_ptr(), n=self.E)
             for key, w in nets], dtype=np.int64)

    def _run_bf16(self, nets) -> None:
        k = kernels()
        s = stream_handle()
        E, H, L = self.E, self.H, self.layout
        if self.fused_torso:
            self._tjobs = np.asarray([jobs.torso_job(rows=0, n=E, pk=w.pk, out=self.Xn[key].data_ptr())
                                      for key, w in nets], dtype=np.int64)
            torso_fwd_fused(self.env.frames.reshape(E, -1), self._tjobs, self.fwd_geom, self.n_workers, s)
        else:
            for key, w in nets:
                torso_forward_library(self.env.frames.reshape(E, -1), None, L, w.flat, self.cfg.env,
                                      self.cfg.model, self.Xn[key])
        gemm(*[Gemm(self.Xn[key], w.pk["w_ih"].t(), self.xp[key], bias=w.lstm_b) for key, w in nets])
        if self.lstm_step:
            # plain step kernel (lstm.hip): no inter-workgroup hand-off, so it runs on any CU subset
            Bc = self._step_chains(nets, self.h_bf, halves=True)
            check(k.r2_lstm_fwd(self._chains.ctypes.data, len(self._chains), Bc, 1, H, 0, s),
                  "lstm_step_kernel")
        else:
            self._step_chains(nets, self.h_bf, halves=False)
            check(k.r2_lstm_fwd_persist(self._chains.ctypes.data, len(nets), E, 1, H, self.ctr.data_ptr(),
                                        self.err.data_ptr(), s), "lstm_step")
        gemm(*[Gemm(self.h_bf_new[key], w.pk["head1"].t(), self.zh[key]) for key, w in nets])
        self._duel_jobs(nets)
        check(k.r2_dueling_fwd_multi(self._djobs.ctypes.data, len(nets), self.A, L.HD, s), "dueling_fwd")

    def _run_fp32(self, nets) -> None:
        """Split-precision inference (csrc/split.h): the learner's fp32 stages at actor shapes.  The
        recurrence is the hand-off-free step kernel (lstm_step_sp.hip) whatever ``lstm_step`` says:
        no persistent split kernel places an actor group's rows, and the step kernel runs on any CU
        subset.  It reads the carried fp32 state (h32, c) as h0 / c0; ``h_bf`` is not used."""
        k = kernels()
        s = stream_handle()
        E, H, L = self.E, self.H, self.layout
        fr = self.env.frames
        if fr.dtype != torch.uint8 or not fr.is_contiguous():
            raise ValueError("fp32 inference reads the env's frames in place: contiguous uint8")
        self._tjobs = np.asarray(
            [jobs.torso_job_sp(rows=0, n=E, pk=w.pk, pk_lo=w.pk_lo, out=self.Xn[key].data_ptr(),
                               out_lo=self.Xn_lo[key].data_ptr()) for key, w in nets], dtype=np.int64)
        check(k.r2_torso_fwd_sp_multi(fr.data_ptr(), self._tjobs.ctypes.data, len(nets), self.n_workers, s),
              "torso_fwd_sp_multi")
        ws, tk = self.sp_ws["xproj"]
        gemm_sp([Gemm(self.Xn[key], w.pk["w_ih"].t(), self.xp[key], bias=w.lstm_b, a_lo=self.Xn_lo[key],
                      b_lo=w.pk_lo["w_ih"].t()) for key, w in nets],
                splits=[0] * len(nets), ws=ws, tickets=tk, n_cus=self.n_workers)
        Bc = self._step_chains(nets, self.h32, halves=True, lo=True)
        check(k.r2_lstm_fwd_sp(self._chains.ctypes.data, len(self._chains), Bc, 1, H, 0, s), "lstm_step_sp")
        ws, tk = self.sp_ws["heads"]
        gemm_sp([Gemm(self.h_bf_new[key], w.pk["head1"].t(), self.zh[key], a_lo=self.h_lo_new[key],
                      b_lo=w.pk_lo["head1"].t()) for key, w in nets],
                splits=[0] * len(nets), ws=ws, tickets=tk, n_cus=self.n_workers)
        self._duel_jobs(nets)
        check(k.r2_dueling_fwd_multi_f32(self._djobs.ctypes.data, len(nets), self.A, L.HD, s), "dueling_fwd_f32")
