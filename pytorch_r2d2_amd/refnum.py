"""Numerics the float64 oracles (``*_ref.py``) share: the bf16 and split-precision number formats,
the splitmix64 finaliser of csrc/common.h, the per-element comparison functions and the
write-ownership checks of NaN-poisoned buffers.

Pure host code (numpy, no torch, no GPU).  A new oracle starts from here and from
tests/gpu_support.py (the device buffers): it brings a reference, its bounds and a case table.
"""
from __future__ import annotations

import numpy as np

_M64 = (1 << 64) - 1


# ------------------------------------------------------------------------------------------
# number formats

def bf16_bits(x) -> np.ndarray:
    """fp32 -> bf16 bit patterns (uint16), round to nearest even; NaN stays NaN."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    b = x.view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(x), np.uint16(0x7FC0), r)


def bf16_val(bits) -> np.ndarray:
    """bf16 bit patterns -> fp32 values."""
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_round(x) -> np.ndarray:
    return bf16_val(bf16_bits(x))


def split_planes(x):
    """csrc/split.h sp_split: hi = bf16(x), lo = bf16(x - hi), as fp32 values."""
    x = np.asarray(x, dtype=np.float32)
    hi = bf16_round(x)
    return hi, bf16_round((x - hi).astype(np.float32))


def as_bytes(x) -> np.ndarray:
    """The bytes of ``x``, flat."""
    return np.ascontiguousarray(x).view(np.uint8).reshape(-1)


def as_u64(x) -> np.ndarray:
    """At least 1-d uint64 array (array arithmetic wraps silently; Python ints are masked)."""
    if isinstance(x, (int, np.integer)):
        return np.asarray([int(x) & _M64], dtype=np.uint64)
    return np.atleast_1d(np.asarray(x)).astype(np.uint64)


def mix64(z) -> np.ndarray:
    """common.h r2_mix64: the splitmix64 finaliser, wrapping 64-bit arithmetic."""
    z = as_u64(z) + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


# ------------------------------------------------------------------------------------------
# comparison plumbing

def compare(label, tensor, got, ref, bound, names=("t", "b", "unit")):
    """Largest |got - ref| / bound; raises naming the first element that is not finite or over its
    bound."""
    got = np.asarray(got, np.float64)
    if got.size == 0:
        return 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        use = np.abs(got - ref) / bound
        use = np.where((got == ref) & np.isfinite(got), 0.0, use)
    bad = ~(use <= 1.0)
    if bad.any():
        idx = tuple(int(i) for i in np.argwhere(bad)[0])
        where = ", ".join(f"{n}={i}" for n, i in zip(names, idx))
        raise AssertionError(f"{label}: {tensor}[{where}] = {got[idx]!r}, oracle {ref[idx]!r}, "
                             f"bound {bound[idx]:.3e} (use {use[idx]:.3g}); {int(bad.sum())} elements fail")
    return float(use.max())


def compare_bf16(label, tensor, bits, ref, bound, names=("t", "b", "unit")):
    """A stored bf16 value against a reference whose *unrounded* value is known to ``bound``: rounding
    is monotone, so the stored value is acceptable exactly when some x in [ref - bound, ref + bound]
    rounds to it.  The use is the share of the bound that x needs: 0 where ref itself rounds to the
    stored value, else the distance from ref to the rounding boundary of the stored value (the
    midpoint between it and its bf16 neighbour on ref's side) over the bound.  Nothing is added
    for the format, so the figure measures the arithmetic and not the rounding."""
    bits = np.asarray(bits, np.uint16)
    if bits.size == 0:
        return 0.0
    got = bf16_val(bits).astype(np.float64)
    b = bits.astype(np.int64)
    key = np.where(b < 0x8000, 0x8000 + b, 0x8000 - (b & 0x7FFF))      # monotone in the value
    toward = np.where(got > ref, key - 1, key + 1)
    nb = np.where(toward >= 0x8000, toward - 0x8000, 0x8000 | (0x8000 - toward)).astype(np.uint16)
    mid = 0.5 * (got + bf16_val(nb).astype(np.float64))
    with np.errstate(invalid="ignore", over="ignore"):
        need = np.where(got > ref, mid - ref, np.where(got < ref, ref - mid, 0.0))
        use = np.where(need <= 0.0, 0.0, need / (bound + 1e-300))
        use = np.where(np.isfinite(got), use, np.inf)
    bad = ~(use <= 1.0)
    if bad.any():
        idx = tuple(int(i) for i in np.argwhere(bad)[0])
        where = ", ".join(f"{n}={i}" for n, i in zip(names, idx))
        raise AssertionError(f"{label}: {tensor}[{where}] = {got[idx]!r} (bf16), oracle {ref[idx]!r} +- "
                             f"{bound[idx]:.3e} before rounding (use {use[idx]:.3g}); {int(bad.sum())} elements fail")
    return float(use.max())


def bits_equal(label, tensor, got, want, names=("t", "b", "unit")):
    bad = np.asarray(got) != np.asarray(want)
    if bad.any():
        idx = tuple(int(i) for i in np.argwhere(bad)[0])
        where = ", ".join(f"{n}={i}" for n, i in zip(names, idx))
        raise AssertionError(f"{label}: {tensor}[{where}] = {got[idx]:#x}, expected {want[idx]:#x} "
                             f"bit for bit; {int(bad.sum())} elements differ")


# ------------------------------------------------------------------------------------------
# write ownership

def check_ownership(label, tensor, full, pad: int, valid=None):
    """``full``: a flat float view of a buffer that was NaN poison before the launch, ``pad`` guard
    elements at each end.  The guards must still be poison, every element of the body where
    ``valid`` (default: everywhere) must be finite, and every other body element still poison."""
    full = np.asarray(full).reshape(-1)
    body = full[pad:full.size - pad]
    for name, g in (("guard before", full[:pad]), ("guard after", full[full.size - pad:])):
        if not np.isnan(g).all():
            i = int(np.argwhere(~np.isnan(g))[0, 0])
            raise AssertionError(f"{label}: {tensor} {name} the buffer was written at {i} ({g[i]!r})")
    v = np.ones(body.shape, bool) if valid is None else np.asarray(valid, bool).reshape(-1)
    if not np.isfinite(body[v]).all():
        i = int(np.argwhere(~np.isfinite(body) & v)[0, 0])
        raise AssertionError(f"{label}: {tensor}[flat {i}] is not finite ({body[i]!r}): not written")
    if not np.isnan(body[~v]).all():
        i = int(np.argwhere(~np.isnan(body) & ~v)[0, 0])
        raise AssertionError(f"{label}: {tensor}[flat {i}] = {body[i]!r} was written; the kernel does not own it")


def check_untouched(label, tensor, full):
    """A refused launch writes nothing: the whole buffer is still poison."""
    check_ownership(label, tensor, full, 0, valid=np.zeros(np.asarray(full).size, bool))
