"""The semantics every GPU oracle test shares, pinned on the CPU device: the poisoned buffers of
tests/gpu_support.py (Guarded, Buf) and the two functions of pytorch_r2d2_amd/refnum.py that
replaced a pair of copies (bf16_bits, mix64)."""
import numpy as np
import pytest
import torch

from gpu_support import Buf, Guarded
from pytorch_r2d2_amd import refnum

PATTERN = {torch.float32: np.array([0, 1, 0x3F800000, 0x80000000, 0x7F7FFFFF, 0xDEADBEEF, 0x00800000, 0x40490FDB],
                                   np.uint32),
           torch.bfloat16: np.array([0, 1, 0x3F80, 0x8000, 0x7F7F, 0xBEEF, 0x0080, 0x4049], np.uint16)}


def _guarded(dtype):
    return Guarded((2, 4), dtype, 8, device="cpu")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_guarded_ownership(dtype):
    g = _guarded(dtype)
    assert g.pad == 8 and g.n == 8 and g.full.numel() == 24
    g.untouched("cpu", "nothing written")
    with pytest.raises(AssertionError, match="not written"):
        g.owned("cpu", "nothing written")
    g.body[:] = 1.0
    g.owned("cpu", "body written")
    with pytest.raises(AssertionError, match="does not own"):
        g.untouched("cpu", "body written")
    # a subset is owned: the rest must still be poison
    half = np.arange(8) < 4
    with pytest.raises(AssertionError, match="does not own"):
        g.owned("cpu", "half", half)
    g.body[4:] = float("nan")
    g.owned("cpu", "half", half)
    for i in range(8):
        h = _guarded(dtype)
        h.body[:] = 1.0
        h.body[i] = float("nan")
        with pytest.raises(AssertionError, match="not written"):
            h.owned("cpu", f"element {i} left out")
    for i in list(range(8)) + list(range(16, 24)):
        h = _guarded(dtype)
        h.body[:] = 1.0
        h.full[i] = 0.0
        with pytest.raises(AssertionError, match="guard (before|after)"):
            h.owned("cpu", f"guard element {i}")
    h = _guarded(dtype)
    h.body[3] = 0.0
    with pytest.raises(AssertionError, match="does not own"):
        h.untouched("cpu", "one write")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_guarded_bits_and_ptr(dtype):
    g = _guarded(dtype)
    pat = PATTERN[dtype]
    signed = {torch.float32: (np.int32, torch.int32), torch.bfloat16: (np.int16, torch.int16)}[dtype]
    g.body.view(signed[1]).copy_(torch.from_numpy(pat.view(signed[0])))
    assert g.bits().dtype == pat.dtype and g.bits().shape == (2, 4)
    assert np.array_equal(g.bits().reshape(-1), pat)
    assert torch.isnan(g.full[:8]).all() and torch.isnan(g.full[16:]).all()
    size = g.full.element_size()
    assert size == pat.itemsize
    assert g.ptr() == g.full.data_ptr() + 8 * size == g.body.data_ptr()
    for elem in (1, 5, 8):
        assert g.ptr(elem) == g.ptr() + elem * size
    assert g.host().shape == (2, 4) and g.host_full().shape == (24,)
    empty = Guarded((0, 4), dtype, 8, device="cpu")
    assert empty.ptr() == empty.full.data_ptr() + 8 * size


@pytest.mark.parametrize("dtype,poison", [(torch.float32, float("nan")), (torch.int32, -1), (torch.uint8, 0xAB)],
                         ids=["f32", "i32", "u8"])
def test_buf_guards(dtype, poison):
    def buf():
        return Buf.poisoned(8, dtype, poison, device="cpu")
    b = buf()
    b.assert_guards("fresh")
    b.assert_untouched("fresh")
    assert b.p == b.full.data_ptr() + 16 * b.full.element_size() and b.body().shape == (8,)
    b.full[16 + 2] = 1
    b.assert_guards("body write")
    with pytest.raises(AssertionError, match="written"):
        b.assert_untouched("body write")
    for i in (0, 15):
        b = buf()
        b.full[i] = 1
        with pytest.raises(AssertionError, match="front guard"):
            b.assert_guards("front")
    for i in (24, 39):
        b = buf()
        b.full[i] = 1
        with pytest.raises(AssertionError, match="back guard"):
            b.assert_guards("back")
    data = Buf(np.arange(8, dtype=np.int64), -1, device="cpu")
    assert data.body().tolist() == list(range(8)) and data.tail().tolist() == list(range(8)) + [-1] * 16


def test_bf16_bits_is_the_actor_oracle_s_formula_off_nan():
    """All 65,536 high halves x five low halves: the function actor_ref used to carry (no NaN
    handling), inlined, gives the same bits wherever the input is not NaN; NaN gives 0x7FC0."""
    hi = np.arange(1 << 16, dtype=np.uint32)[:, None] << 16
    lo = np.array([0, 0x7FFF, 0x8000, 0x8001, 0xFFFF], np.uint32)[None, :]
    x = (hi | lo).reshape(-1).view(np.float32)
    b = np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32).astype(np.uint64)
    old = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)
    new = refnum.bf16_bits(x)
    nan = np.isnan(x)
    assert new.dtype == np.uint16 and nan.sum() == 2 * (127 * 5 + 4) and (~nan).sum() > 326000
    assert np.array_equal(new[~nan], old[~nan])
    assert (new[nan] == 0x7FC0).all()


def _mix64_replay(z):
    if isinstance(z, (int, np.integer)):
        z = np.asarray([int(z) & ((1 << 64) - 1)], dtype=np.uint64)
    z = np.atleast_1d(np.asarray(z)).astype(np.uint64) + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _mix64_pong(z):
    z = z + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def test_mix64_is_both_former_copies():
    """replay_ref's copy (Python ints and arrays) and pong_ref's (uint64 arrays), inlined."""
    rng = np.random.default_rng(64)
    vals = np.concatenate([np.array([0, 2 ** 64 - 1], np.uint64),
                           rng.integers(0, 2 ** 64, 1000, dtype=np.uint64, endpoint=False)])
    got = refnum.mix64(vals)
    assert got.dtype == np.uint64 and got.shape == vals.shape
    assert np.array_equal(got, _mix64_replay(vals)) and np.array_equal(got, _mix64_pong(vals))
    assert int(got[0]) == 0xE220A8397B1DCDAF         # splitmix64's first output for state 0
    for v, g in zip(vals.tolist(), got.tolist()):
        one = refnum.mix64(v)                        # a Python int
        assert one.shape == (1,) and int(one[0]) == g == int(_mix64_replay(v)[0])
        assert int(refnum.mix64(np.uint64(v))[0]) == g
    assert int(refnum.mix64(2 ** 64 + 5)[0]) == int(refnum.mix64(5)[0])      # ints are masked
