"""The last K-tile of the flat entries of the streaming fp32 GETT (CTAMD_TILE_LAST_EARLY in gett_f32_stream_kloop.inc): its MFMAs are
issued fragment by fragment and each finished group of accumulators is stored to the slice's partial image under the MFMAs of the next
group, instead of all nine stores behind the last MFMA.

Every accumulator still receives its k-steps in the general entry's order and the image has the general entry's layout, so every case
runs one plan on the same buffers through the scalar-parameter entry (the default), the struct entry (CUTENSOR_AMD_FLAT_START=2) — the
two that have the new last tile — and the general entry (=0), which has the old one: the three outputs must be equal bit for bit.  The
data are integers in {-2 .. 2}: every product and partial sum is an integer below 2^24 (K <= 2048: |sum| <= 8192), exact in fp32, so
the result must also EQUAL an int64 reference — a fragment stored before its last k-step, twice, or to another fragment's place cannot.

The cases are shrunk forms of the headline 'abcd,dcbe->ae' with the split forced (CUTENSOR_AMD_F32_SPLITK, hooks flavour): 1 .. 7 and
32 K-tiles per slice reach the three places the last tile is written out — one tile left, two left, a whole turn of the 3-deep ring —
each with and without whole ring turns in front."""
import os

import numpy as np
import pytest

from test_gpu_f32_flat_start import _shape, find_plan

gpu = pytest.mark.gpu

ENTRIES = (None, "2", "0")      # CUTENSOR_AMD_FLAT_START: scalar parameters (the default), the struct entry, the general entry
GUARD = 4096                    # bytes on either side of the workspace in the guarded case
FILL = 0xA5


@pytest.fixture(scope="module")
def env(built):
    import torch
    assert torch.cuda.is_available()
    from cudalibrarysamples_amd import cutensor as ct, ops
    return ct, ops, ops.Handle(), torch


def run_three(env, ext, split, tiles, alpha=1.0, beta=0.0, nt=False, seed=0, mA="dcba", mB="ebcd", swapped=False, guarded=False):
    ct, ops, h, torch = env
    p, d = find_plan(env, ext, mA, mB, split, nt)
    assert d["kPerSlice"] == 32 * tiles and d["blocks"] == split and d["nt"] == int(nt) and d["swapped"] == int(swapped), d
    g = torch.Generator(device="cuda")
    g.manual_seed(4000 + seed)
    shA, subA = _shape(ext, mA)
    shB, subB = _shape(ext, mB)
    A = torch.randint(-2, 3, shA, generator=g, device="cuda").float()
    B = torch.randint(-2, 3, shB, generator=g, device="cuda").float()
    C = torch.randint(-2, 3, (ext["a"], ext["e"]), generator=g, device="cuda").float()
    C0 = C.clone()
    need = p.required_workspace
    assert need >= split * 96 * 96 * 4, d          # one 96 x 96 image per slice, clamped rows included
    pad = GUARD if guarded else 0
    ws = torch.full((pad + max(need, 256) + pad,), FILL, dtype=torch.uint8, device="cuda")
    outs = []
    for switch in ENTRIES:
        D = torch.full((ext["a"], ext["e"]), float("nan"), device="cuda")
        if guarded:
            ws[pad:pad + need] = 0x5A               # stale partials of the run before must not pass for this run's
        if switch is not None:
            os.environ["CUTENSOR_AMD_FLAT_START"] = switch
        try:
            before = ct.flat_start_count()
            p.contract(alpha, A.data_ptr(), B.data_ptr(), beta, C.data_ptr(), D.data_ptr(), ws.data_ptr() + pad, need,
                       torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            took_flat = ct.flat_start_count() - before
        finally:
            os.environ.pop("CUTENSOR_AMD_FLAT_START", None)
        assert took_flat == (0 if switch == "0" else 1), (switch, took_flat, d)
        if guarded:
            assert bool((ws[:pad] == FILL).all()) and bool((ws[pad + need:] == FILL).all()), (switch, d)
        outs.append(D)
    p.destroy()
    assert torch.equal(C, C0)
    for D in outs:
        assert not torch.isnan(D).any(), d
    assert torch.equal(outs[0], outs[1]), (d, float((outs[0] - outs[1]).abs().max()))
    assert torch.equal(outs[0], outs[2]), (d, float((outs[0] - outs[2]).abs().max()))
    ref = np.einsum("%s,%s->ae" % (subA, subB), A.cpu().numpy().astype(np.int64), B.cpu().numpy().astype(np.int64), optimize=True)
    ref = int(alpha) * ref + int(beta) * C0.cpu().numpy().astype(np.int64)
    assert alpha == int(alpha) and beta == int(beta) and np.abs(ref).max() < (1 << 24)
    assert np.array_equal(outs[0].cpu().numpy().astype(np.int64), ref), d
    assert np.array_equal(outs[0].cpu().numpy(), ref.astype(np.float32)), d
    return d


FULL = dict(a=96, e=96)
K16 = dict(FULL, d=32, b=4, c=4)      # 16 K-tiles
K12 = dict(FULL, d=32, b=4, c=3)      # 12
K10 = dict(FULL, d=32, b=2, c=5)      # 10
K14 = dict(FULL, d=32, b=2, c=7)      # 14
K64 = dict(FULL, d=64, b=2, c=16)     # 64: two slices of the headline's own 32 K-tiles

# K-tiles per slice -> (extents, split).  One tile left: 1, 4, 7; two left: 2, 5, 32; a whole turn: 3, 6
CASES = {1: (K16, 16), 2: (K16, 8), 3: (K12, 4), 4: (K16, 4), 5: (K10, 2), 6: (K12, 2), 7: (K14, 2), 32: (K64, 2)}


@gpu
@pytest.mark.parametrize("tiles", list(CASES))
def test_every_end_of_the_k_loop(env, tiles):
    ext, split = CASES[tiles]
    run_three(env, ext, split, tiles, seed=tiles)


@gpu
@pytest.mark.parametrize("tiles", [1, 5, 6])
def test_clamped_rows_and_guarded_workspace(env, tiles):
    """a = 90, e = 70 inside the 96 x 96 tile: the accumulators of clamped rows are stored to the image like the others (and kept out
    of D by the fold), so the image is whole 96 x 96 tiles whatever the extents — and stays inside the workspace the plan asked for:
    guard bytes on both sides are untouched after each of the three entries.
    Both operands K-contiguous: a free-contiguous B of 70-float rows has no 16-byte lanes and has no flat form."""
    ext, split = CASES[tiles]
    run_three(env, dict(ext, a=90, e=70), split, tiles, seed=40 + tiles, mB="dcbe", guarded=True)


@gpu
@pytest.mark.parametrize("tiles", [2, 3, 4])
def test_swapped_orientation(env, tiles):
    """D's fastest mode lives in the caller's A: the kernel's operands are the caller's, exchanged"""
    ext, split = CASES[tiles]
    run_three(env, ext, split, tiles, seed=50 + tiles, mA="ebcd", mB="dcba", swapped=True)


@gpu
@pytest.mark.parametrize("tiles", [3, 7])
def test_scalars_and_a_separate_c(env, tiles):
    ext, split = CASES[tiles]
    run_three(env, ext, split, tiles, alpha=2.0, beta=-3.0, seed=60 + tiles)


@gpu
@pytest.mark.parametrize("tiles", [2, 4, 6])
def test_nontemporal_twin(env, tiles):
    ext, split = CASES[tiles]
    run_three(env, ext, split, tiles, nt=True, seed=70 + tiles)
