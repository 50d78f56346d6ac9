"""The positional int64 rows that the multi-job launchers take, by name.

Each builder returns the list of ints of ONE row, in the order the launcher copies it into its
C struct; a launch takes ``np.asarray(rows, dtype=np.int64)``.  Pointer words are device addresses
(``ptr(t)``, plus a byte offset for a row range of ``t``); an optional pointer is 0.  The
float64-oracle tests build the same rows by hand, as an independent check of these layouts.
``PolicyInference`` builds its rows here; ``LearnerEngine`` still builds the same rows inline
(``_torso_job``, ``_torso_job_sp``, ``_chain_desc``, ``_duel_fwd``).
"""
from __future__ import annotations

from typing import List


def torso_job(*, rows: int, n: int, pk, out: int, save1: int = 0, save2: int = 0) -> List[int]:
    """``TFJob`` (csrc/kernels/torso.hip), 12 words: frame-row list (0 = frames 0..n-1), n, the
    three conv layers' weight / bias, the (n, D) bf16 features, optional saved act1 / act2;
    word 11 is reserved."""
    return [rows, n, pk["conv1"].data_ptr(), pk["b1"].data_ptr(), pk["conv2"].data_ptr(),
            pk["b2"].data_ptr(), pk["conv3"].data_ptr(), pk["b3"].data_ptr(), out, save1, save2, 0]


def torso_job_sp(*, rows: int, n: int, pk, pk_lo, out: int, out_lo: int, saves=(0, 0, 0, 0),
                 tq: int = 0, qmode: int = 0) -> List[int]:
    """``TSJob`` (csrc/kernels/torso_sp.hip), 20 words: as ``TFJob`` with a lo plane behind every
    bf16 operand; ``saves`` = act1 hi / lo, act2 hi / lo; words 17 / 18 the frame queue ``tq`` and
    its ``qmode`` (both 0 = the static deal); word 19 is reserved."""
    return [rows, n, pk["conv1"].data_ptr(), pk_lo["conv1"].data_ptr(), pk["b1"].data_ptr(),
            pk["conv2"].data_ptr(), pk_lo["conv2"].data_ptr(), pk["b2"].data_ptr(),
            pk["conv3"].data_ptr(), pk_lo["conv3"].data_ptr(), pk["b3"].data_ptr(),
            out, out_lo, *saves, tq, qmode, 0]


def lstm_chain(*, xproj: int, whh: int, h0: int, c0: int, h_seq: int, c_seq: int, h32: int = 0,
               gates: int = 0, save_from: int = 0, whh_lo: int = 0, h_lo: int = 0) -> List[int]:
    """``LstmChain`` (csrc/kernels/lstm.hip) / ``PChain`` (csrc/lstm_common.h), 9 words; with
    ``whh_lo`` the 11-word split-precision form (``h0`` is then fp32, ``h_lo`` the lo plane of
    ``h_seq``)."""
    d = [xproj, whh, h0, c0, h_seq, c_seq, h32, gates, save_from]
    return d + [whh_lo, h_lo] if whh_lo else d


def duel_job(*, z: int, pk, q: int, n: int, zr: int = 0) -> List[int]:
    """``DuelJob`` (csrc/kernels/head.hip), 7 words: layer-1 pre-activations, b1, w2, b2, the Q
    output, the optional ReLU output, the row count."""
    return [z, pk["head_b1"].data_ptr(), pk["head_w2"].data_ptr(), pk["head_b2"].data_ptr(), q, zr, n]
