"""The ctypes signature table (ops/_lib.py _SIGS) against the extern "C" entry points in csrc/:
every declared function exists with the same parameter count (ctypes would pass a surplus
argument through as a C vararg and shift the trailing stream handle), and the loaded library
refuses a call with the wrong count."""
import glob
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _decls():
    src = ""
    for pat in ("csrc/**/*.hip", "csrc/**/*.cpp", "csrc/*.h"):
        for f in glob.glob(os.path.join(ROOT, pat), recursive=True):
            with open(f) as fh:
                src += fh.read()
    out = {}
    for m in re.finditer(r'extern "C" [\w\s\*]+?\b(r2_\w+)\s*\(([^)]*)\)\s*\{', src):
        a = m.group(2).strip()
        out[m.group(1)] = 0 if a in ("", "void") else len(a.split(","))
    return out


def test_ctypes_table_matches_sources():
    from pytorch_r2d2_amd.ops._lib import _SIGS
    d = _decls()
    assert not [k for k in _SIGS if k not in d]
    assert not [(k, len(v), d[k]) for k, v in _SIGS.items() if d[k] != len(v)]


def test_one_shot_setters_are_gone():
    """Per-launch options are arguments of the launch they belong to (BpttOpts, r2_td_duel_dh
    fwd / done_flag, r2_prio_tail_sample wait), not values parked by a call made before it.
    The setters left, in the table and in the sources, are the construction-time process settings
    and the test / probe switches: no BPTT dz, stop-word or XCD-pairs setter, no TD done-flag or
    head-forward setter, no priority-tail wait setter."""
    from pytorch_r2d2_amd.ops._lib import _SIGS
    kept = re.compile(r"r2_set_(num|xcd)_cus|r2_gemm_set_version|r2_gemm5_set_mode|"
                      r"r2_\w+_set_(debug|trace|stamps)")
    names = set(_SIGS) | set(_decls())
    setters = [n for n in names if re.search(r"_set(_|$)|_xcd_pairs$", n)]
    assert setters and not [n for n in setters if not kept.fullmatch(n)]


def test_bptt_opts_mirror_matches_library():
    import ctypes
    from pytorch_r2d2_amd.ops import _lib
    if not _lib.available():
        pytest.skip("kernel library not built")
    assert _lib.kernels().r2_lstm_bptt_opts_bytes() == ctypes.sizeof(_lib.BpttOpts)


def test_strict_wrapper_refuses_wrong_arg_count():
    from pytorch_r2d2_amd.ops import _lib
    if not _lib.available():
        pytest.skip("kernel library not built")
    k = _lib.kernels()
    with pytest.raises(TypeError):
        k.r2_gemm5_set_mode(0, 1)
    assert k.r2_gemm5_set_mode(0) == 0
