"""The order of the contracted digits in one-tile split-K plans of the streaming fp32 GETT (plan_contraction.cpp, stream_k_order): the
K-contiguous operand's stride-1 digit first, the others by the OTHER operand's strides.

Any order of the contracted digits is a valid GETT view, and on integer data in {-2 .. 2} every product and partial sum is an integer
below 2^24 (K <= 2560: |sum| <= 10240), exact in fp32 in any order.  So each case runs the plan of the new order through the three
entries of the kernel (scalar parameters, CUTENSOR_AMD_FLAT_START=2: the struct entry, =0: the general entry) and the plan made under
CUTENSOR_AMD_KORDER=A (the order of the K-contiguous operand's strides) on the same buffers: the four outputs must be equal bit for
bit and must EQUAL an int64 reference; ctamdFlatStartCount says which entry ran.

The cases are shrunk forms of the headline 'abcd,dcbe->ae': A is K-contiguous (d first), B is not (e first, then b, c, d), and the
three contracted extents are unequal, so that a digit paired with another digit's stride or extent reads the wrong elements.  The new
order is d, b, c.  First digit 32 and 64 (one and two K-tiles per period), the other two from {2, 3, 5, 8}; the split is forced
(CUTENSOR_AMD_F32_SPLITK, hooks flavour) so that a slice has 1 .. 7 K-tiles — every residue of a 3- and of a 4-deep ring.  Seven
divides none of the K-tile counts these extents give, so that case has a shorter last slice (40 K-tiles as 5 x 7 + 5), which the flat
entry covers.  The same arithmetic leaves no split with 32 K-tiles per slice ((1 | 2) x {6, 10, 15, 16, 24, 40} K-tiles): that case
keeps the headline's own slice, d = 64, b = 2, c = 16 in two slices."""
import os

import numpy as np
import pytest

from test_gpu_f32_flat_start import _shape

gpu = pytest.mark.gpu

ENTRIES = (None, "2", "0")      # CUTENSOR_AMD_FLAT_START: scalar parameters (the default), the struct entry, the general entry


@pytest.fixture(scope="module")
def env(built):
    import torch
    assert torch.cuda.is_available()
    from cudalibrarysamples_amd import cutensor as ct, ops
    return ct, ops, ops.Handle(), torch


def find_plan(env, ext, mA, mB, split, nt, korder):
    """Walk algo = candidate index until the plan runs the 96 x 96 ring-3 streaming kernel split `split` ways"""
    ct, ops, h, _ = env
    kw = dict(workspace_limit=1 << 30, cache_mode=ct.CACHE_MODE_NONE)
    if nt:
        kw["operands_streamed"] = True
    os.environ["CUTENSOR_AMD_F32_SPLITK"] = str(split)
    if korder:
        os.environ["CUTENSOR_AMD_KORDER"] = korder
    try:
        for r in range(256):
            p = ops.contraction_plan(h, [ext[c] for c in mA], mA, [ext[c] for c in mB], mB, [ext["e"], ext["a"]], "ea", algo=r, **kw)
            d = p.describe()
            if d["kname"] == "gett_f32_stream_kernel" and (d["bm"], d["bn"], d["pf"], d["nt"]) == (96, 96, 3, int(nt)):
                assert d["splitK"] == split, d
                return p, d
            p.destroy()
    finally:
        os.environ.pop("CUTENSOR_AMD_F32_SPLITK", None)
        os.environ.pop("CUTENSOR_AMD_KORDER", None)
    raise AssertionError("no 96 x 96 ring-3 streaming split-K candidate for %r %s %s split %d" % (ext, mA, mB, split))


def digits(ext, kernelA, kernelB, order):
    """[extent, stride in kernel-A, stride in kernel-B] of the modes `order`, operands packed with their modes fastest first"""
    def strides(modes):
        s, acc = {}, 1
        for c in modes:
            s[c] = acc
            acc *= ext[c]
        return s
    sA, sB = strides(kernelA), strides(kernelB)
    return [[ext[c], sA[c], sB[c]] for c in order]


def run_orders(env, ext, split, tiles, alpha=1.0, beta=0.0, nt=False, seed=0, swapped=False):
    ct, ops, h, torch = env
    # kernel-A is the K-contiguous tensor (d, c, b, a), kernel-B the free-contiguous one (e, b, c, d); D = (e, a) has its fastest mode in
    # the latter — which the caller passes first when `swapped`
    mK, mF = "dcba", "ebcd"
    mA, mB = (mF, mK) if swapped else (mK, mF)
    pNew, dNew = find_plan(env, ext, mA, mB, split, nt, None)
    pOld, dOld = find_plan(env, ext, mA, mB, split, nt, "A")
    for d in (dNew, dOld):
        assert d["kPerSlice"] == 32 * tiles and d["blocks"] == split and d["nt"] == int(nt) and d["swapped"] == int(swapped), d
        assert (d["layA"], d["layB"]) == (1, 0), d
    assert dNew["Kdigits"] == digits(ext, mK, mF, "dbc"), dNew
    assert dOld["Kdigits"] == digits(ext, mK, mF, "dcb"), dOld
    assert dNew["kernel"] == dOld["kernel"] and pNew.required_workspace == pOld.required_workspace, (dNew, dOld)
    g = torch.Generator(device="cuda")
    g.manual_seed(3000 + seed)
    shA, subA = _shape(ext, mA)
    shB, subB = _shape(ext, mB)
    A = torch.randint(-2, 3, shA, generator=g, device="cuda").float()
    B = torch.randint(-2, 3, shB, generator=g, device="cuda").float()
    C = torch.randint(-2, 3, (ext["a"], ext["e"]), generator=g, device="cuda").float()
    C0 = C.clone()
    ws = torch.empty(max(pNew.required_workspace, 256), dtype=torch.uint8, device="cuda")
    outs = []
    for p, switch in [(pNew, s) for s in ENTRIES] + [(pOld, None)]:
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
        assert took_flat == (0 if switch == "0" else 1), (switch, took_flat, dNew)
        outs.append(D)
    pNew.destroy()
    pOld.destroy()
    assert torch.equal(C, C0)
    for D in outs:
        assert not torch.isnan(D).any(), dNew
    for other, what in zip(outs[1:], ("struct entry", "general entry", "CUTENSOR_AMD_KORDER=A")):
        assert torch.equal(outs[0], other), (what, dNew, float((outs[0] - other).abs().max()))
    ref = np.einsum("%s,%s->ae" % (subA, subB), A.cpu().numpy().astype(np.int64), B.cpu().numpy().astype(np.int64), optimize=True)
    ref = int(alpha) * ref + int(beta) * C0.cpu().numpy().astype(np.int64)
    assert alpha == int(alpha) and beta == int(beta) and np.abs(ref).max() < (1 << 24)
    assert np.array_equal(outs[0].cpu().numpy().astype(np.int64), ref), dNew
    assert np.array_equal(outs[0].cpu().numpy(), ref.astype(np.float32)), dNew
    return dNew


FULL = dict(a=96, e=96)
# (extents, split, K-tiles per slice); the K-tile index runs d / 32 fastest, then b, then c
CASES = {
    "1": (dict(d=32, b=2, c=3), 6, 1),
    "2": (dict(d=32, b=3, c=2), 3, 2),       # slices end at K-tiles 2 and 4: b = 2 of 3, and b = 1 of 3 with c = 1 — inside the second digit
    "3": (dict(d=64, b=3, c=5), 10, 3),      # two K-tiles per period of d: every other slice starts in the middle of d
    "4": (dict(d=32, b=8, c=3), 6, 4),
    "5": (dict(d=32, b=5, c=8), 8, 5),       # slices of one whole run of b: every boundary lies inside the third digit only
    "6": (dict(d=64, b=5, c=3), 5, 6),       # slices end at period 3 of 5, 1 of 5, ...: inside the second digit, carries into the third
    "7": (dict(d=32, b=5, c=8), 6, 7),       # 40 K-tiles as 5 x 7 + 5: the last slice is shorter
    "32": (dict(d=64, b=2, c=16), 2, 32),    # the headline's own slice: eight whole turns of a 4-deep ring, ten and two thirds of a 3-deep one
}


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_every_residue_of_both_ring_depths(env, name):
    ext, split, tiles = CASES[name]
    run_orders(env, dict(FULL, **ext), split, tiles, seed=tiles)


@gpu
@pytest.mark.parametrize("name", ["3", "5"])
def test_clamped_rows(env, name):
    """a = 40, e = 72: rows past the extents are clamped on the way in and kept out of D"""
    ext, split, tiles = CASES[name]
    run_orders(env, dict(ext, a=40, e=72), split, tiles, seed=40 + tiles)


@gpu
@pytest.mark.parametrize("name", ["3", "7"])
def test_swapped_orientation(env, name):
    """D's fastest mode lives in the caller's A: the K-contiguous operand is the caller's B, and the order follows the caller's A"""
    ext, split, tiles = CASES[name]
    run_orders(env, dict(FULL, **ext), split, tiles, seed=50 + tiles, swapped=True)
    run_orders(env, dict(ext, a=40, e=72), split, tiles, seed=60 + tiles, swapped=True)


@gpu
def test_scalars_and_a_separate_c(env):
    ext, split, tiles = CASES["5"]
    run_orders(env, dict(FULL, **ext), split, tiles, alpha=2.0, beta=-3.0, seed=70)


@gpu
@pytest.mark.parametrize("name", ["2", "7"])
def test_nontemporal_twin(env, name):
    ext, split, tiles = CASES[name]
    run_orders(env, dict(FULL, **ext), split, tiles, nt=True, seed=80 + tiles)
