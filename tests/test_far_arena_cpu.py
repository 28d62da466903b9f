"""The arena of tests/far_cases.py on CPU tensors, at 16 offset bits in place of 32 (no GPU): a plain numpy stand-in kernel scatters into a
far D, or gathers from a far A and accumulates, by byte offsets from the tensor's pointer.  A correct stand-in passes; four wrong ones — an
offset truncated to the scale's bits, one sign-extended from them, a store one pitch too far, one element not written — are each caught:
by a byte of the arena that is no longer 0xFF, by a NaN in the result, or by the element left poisoned.  The misplaced accesses all stay
inside the arena: that is what its margins are for."""
import numpy as np
import pytest
import torch

import far_cases as fc

BITS = 16
LO31, HI31, LO32, HI32 = fc.targets(BITS, 5)     # (+-2^11 bytes: several 16-byte pitch steps of a 20-row tensor, as 2^21 is at 32 bits)
EXT = [24, 20]          # a [24][20] fp32 tensor, the second mode's pitch inflated


def _offsets(strides, how):
    """byte offsets of every element (first mode fastest) as the stand-in kernel computes them"""
    off = (np.arange(EXT[0])[:, None] * strides[0] + np.arange(EXT[1])[None, :] * strides[1]) * 4
    if how == "truncated":
        off = off & ((1 << BITS) - 1)
    elif how == "sign_extended":
        off = ((off & ((1 << BITS) - 1)) ^ (1 << (BITS - 1))) - (1 << (BITS - 1))
    elif how == "one_pitch_far":
        off = off + strides[1] * 4
    return off


def _scatter(arena, far, src, how):
    """D[i][j] = src[i][j], stored at far.byte0 + offset"""
    mem = arena.raw.numpy()
    off = far.byte0 + _offsets(far.strides, how)
    assert off.min() >= 0 and off.max() + 4 <= arena.size, "a stand-in left the arena: the margins are too small"
    data = src.astype(np.float32).view(np.uint8).reshape(EXT[0], EXT[1], 4)
    for b in range(4):
        mem[off + b] = data[:, :, b]
    if how == "one_missing":
        mem[far.byte0 + (5 * far.strides[0] + 7 * far.strides[1]) * 4:][:4] = 0xFF


def _gather_accumulate(arena, far, how):
    """out[i] = sum_j A[i][j], A read at far.byte0 + offset"""
    mem = arena.raw.numpy()
    off = far.byte0 + _offsets(far.strides, how)
    assert off.min() >= 0 and off.max() + 4 <= arena.size
    data = np.stack([mem[off + b] for b in range(4)], axis=-1).copy().view(np.float32)[:, :, 0]
    return data.sum(axis=1)


@pytest.fixture(scope="module")
def arena():
    return fc.Arena(bits=BITS, device="cpu")


def _src():
    return np.random.default_rng(5).integers(-3, 4, size=EXT).astype(np.float32)


def _far(arena, target, off=3):
    strides = fc.far_strides(EXT, 4, target)
    return arena.place(EXT, strides, "float32", off)


def test_geometry(arena):
    assert arena.size == 3 * ((1 << BITS) + (1 << (BITS - 4))) and arena.base == arena.size // 3
    assert 3 * ((1 << 32) + (1 << 28)) == 13690208256 and fc.HI32 <= (1 << 32) + (1 << 27)
    for tg in (LO31, HI31, LO32, HI32):
        f = _far(arena, tg)
        assert tg - 20 * 16 < f.span_bytes <= tg
        # an offset off by +-2^(bits-1) or +-2^bits from any element stays inside
        assert f.byte0 - (1 << BITS) >= 0 and f.byte0 + f.span_bytes + (1 << BITS) <= arena.size


@pytest.mark.parametrize("target", [LO31, HI31, LO32, HI32])
def test_a_correct_scatter_passes(arena, target):
    far, src = _far(arena, target), _src()
    _scatter(arena, far, src, "correct")
    assert torch.equal(far.get(), torch.from_numpy(src))
    far.check_outside("correct scatter")
    assert arena.sweeps >= 1


@pytest.mark.parametrize("how", ["truncated", "sign_extended", "one_pitch_far", "one_missing"])
def test_a_wrong_scatter_is_caught(arena, how):
    target = HI31 if how == "sign_extended" else HI32          # offsets pass 2^(bits-1) / 2^bits
    far, src = _far(arena, target), _src()
    _scatter(arena, far, src, how)
    got = far.get()
    poisoned = int(torch.isnan(got).sum())
    broken = False
    try:
        far.check_outside(how)
    except AssertionError as e:
        broken = True
        assert "outside the far tensor's elements" in str(e)
    if how == "one_missing":
        assert poisoned == 1 and not broken and bool(torch.isnan(got[5, 7]))
    else:
        assert broken or poisoned >= 1, (how, broken, poisoned)           # a guard byte written, or an element left poisoned
        assert not torch.equal(got, torch.from_numpy(src))
    # the failed check refilled the arena: the next case starts clean
    arena.check_clean("after " + how)


@pytest.mark.parametrize("how", ["correct", "truncated", "sign_extended", "one_pitch_far"])
def test_a_gather_from_a_far_input(arena, how):
    target = HI31 if how == "sign_extended" else HI32
    far, src = _far(arena, target), _src()
    far.set(torch.from_numpy(src))
    out = _gather_accumulate(arena, far, how)
    if how == "correct":
        assert np.array_equal(out, src.sum(axis=1))
    else:
        assert not np.array_equal(out, src.sum(axis=1)), how   # poison, or another element, was read: the exact comparison fails
    assert torch.equal(far.get(), torch.from_numpy(src))       # the input is unchanged
    far.check_outside("gather " + how)


def test_sixteen_byte_elements_are_repoisoned_whole(arena):
    ext = [6, 5]
    far = arena.place(ext, fc.far_strides(ext, 16, HI32), "complex128", 1)
    far.set(torch.ones(ext, dtype=torch.complex128))
    with pytest.raises(AssertionError):
        arena.check_clean("elements set")
    far.set(torch.ones(ext, dtype=torch.complex128))
    far.check_outside("complex128")
