"""The flat entries of the streaming fp32 GETT and of its split-K fold on SCALAR kernel parameters (kernel-argument preload:
gett_f32_stream_kernel<StreamCfg<.., 8 | 9>> and splitk_fold_frag_args_kernel) against the flat entries on StreamFlatParams /
FoldFlatParams (CUTENSOR_AMD_FLAT_START=2) and the general entries (CUTENSOR_AMD_FLAT_START=0).

The three share the ring schedule, the K loop's sum order and the fold's tree, so every case runs one plan on the same buffers through
all three and the outputs must be equal bit for bit; ctamdFlatStartCount moves for the first two only.  The data are integers in
{-2 .. 2}: every product and partial sum is an integer below 2^24 (K <= 2048: |sum| <= 8192), exact in fp32 in any order, so the result
must also EQUAL an int64 reference.

The cases are shrunk forms of the headline 'abcd,dcbe->ae' with the split forced (CUTENSOR_AMD_F32_SPLITK, hooks flavour): 1 .. 7 and
32 K-tiles per slice cover every residue of the 3-deep ring — the straight-line one- and two-tile ends of the K loop with and without
whole ring turns in front of them, and the whole-turn end."""
import os

import numpy as np
import pytest

from test_gpu_f32_flat_start import _shape, find_plan

gpu = pytest.mark.gpu

ENTRIES = (None, "2", "0")      # CUTENSOR_AMD_FLAT_START: scalar parameters (the default), the struct entries, the general entries


@pytest.fixture(scope="module")
def env(built):
    import torch
    assert torch.cuda.is_available()
    from cudalibrarysamples_amd import cutensor as ct, ops
    return ct, ops, ops.Handle(), torch


def run_three(env, ext, split, tiles, alpha=1.0, beta=0.0, nt=False, seed=0, mA="dcba", mB="ebcd"):
    ct, ops, h, torch = env
    p, d = find_plan(env, ext, mA, mB, split, nt)
    assert d["kPerSlice"] == 32 * tiles and d["blocks"] == split and d["nt"] == int(nt), d
    g = torch.Generator(device="cuda")
    g.manual_seed(2000 + seed)
    shA, subA = _shape(ext, mA)
    shB, subB = _shape(ext, mB)
    A = torch.randint(-2, 3, shA, generator=g, device="cuda").float()
    B = torch.randint(-2, 3, shB, generator=g, device="cuda").float()
    C = torch.randint(-2, 3, (ext["a"], ext["e"]), generator=g, device="cuda").float()
    C0 = C.clone()
    ws = torch.empty(max(p.required_workspace, 256), dtype=torch.uint8, device="cuda")
    outs = []
    for switch in ENTRIES:
        D = torch.full((ext["a"], ext["e"]), float("nan"), device="cuda")
        if switch is not None:
            os.environ["CUTENSOR_AMD_FLAT_START"] = switch
        try:
            before = ct.flat_start_count()
            p.contract(alpha, A.data_ptr(), B.data_ptr(), beta, C.data_ptr(), D.data_ptr(), ws.data_ptr(), p.required_workspace,
                       torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            took_flat = ct.flat_start_count() - before
        finally:
            os.environ.pop("CUTENSOR_AMD_FLAT_START", None)
        assert took_flat == (0 if switch == "0" else 1), (switch, took_flat, d)
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


@gpu
@pytest.mark.parametrize("ext,split,tiles", [(K16, 16, 1), (K16, 8, 2), (K16, 4, 4), (K12, 4, 3), (K12, 2, 6), (K10, 2, 5), (K14, 2, 7), (K64, 2, 32)],
                         ids=["1", "2", "4", "3", "6", "5", "7", "32"])
def test_every_residue_of_the_ring_depth(env, ext, split, tiles):
    run_three(env, ext, split, tiles, seed=tiles)


@gpu
def test_partial_tile(env):
    """a = 90, e = 50: rows past the extents are clamped on the way in (Mtot and Ntot share one preloaded dword) and kept out of D.
    Both operands K-contiguous: a free-contiguous B of 50-float rows has no 16-byte lanes and runs the ragged twin of the general
    entry, which has no flat form (tests/test_gpu_f32_unaligned.py covers it)."""
    run_three(env, dict(K10, a=90, e=50), 2, 5, seed=40, mB="dcbe")


@gpu
def test_scalars_and_a_separate_c(env):
    """alpha = 2, beta = -3, C != D: C's side of the fold is behind the preloaded parameters"""
    run_three(env, K12, 4, 3, alpha=2.0, beta=-3.0, seed=41)


@gpu
def test_nontemporal_twin(env):
    run_three(env, K10, 2, 5, nt=True, seed=42)
