"""The flat entry of the streaming fp32 GETT (gett_f32_stream_kernel on StreamFlatParams: one output tile, one M and one N mode, no
batch, split-K with a separate fold) and the fold's constant-divisor instantiations against the general entry of the same kernels.

Both entries share the ring schedule, the K loop and the sum order of the fold, so every case is run twice on the same plan and the
same buffers — flat entry (ctamdFlatStartCount moves), then CUTENSOR_AMD_FLAT_START=0 (it does not) — and the two outputs must be
equal bit for bit; one case of each group is also checked against an fp64 reference at the headline test's rtol 1e-4.

The cases are shrunk forms of the headline 'abcd,dcbe->ae'.  The planner itself only offers power-of-two splits with at least four
K-tiles per slice; CUTENSOR_AMD_F32_SPLITK (hooks flavour) asks for the split a case names, also below that — the start-up paths
under the ring depth (1, 2 and 3 K-tiles per slice) are what a shrunk case has to reach."""
import os

import pytest

from test_kernel_resources import _code_object, _kernel_notes

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(built):
    import torch
    assert torch.cuda.is_available()
    from cudalibrarysamples_amd import cutensor as ct, ops
    return ct, ops, ops.Handle(), torch


def _shape(ext, modes):
    """torch (row-major) shape and einsum subscripts of a packed tensor whose cuTENSOR modes are `modes`, fastest first"""
    return [ext[c] for c in reversed(modes)], modes[::-1]


def find_plan(env, ext, mA, mB, split, nt=False):
    """Walk algo = candidate index until the plan runs the 96 x 96 ring-3 streaming kernel (the tile that has a flat twin) split `split` ways."""
    ct, ops, h, _ = env
    kw = dict(workspace_limit=1 << 30, cache_mode=ct.CACHE_MODE_NONE)
    if nt:
        kw["operands_streamed"] = True        # ranks the nontemporal twins (one output tile)
    os.environ["CUTENSOR_AMD_F32_SPLITK"] = str(split)
    try:
        last = None
        for r in range(256):
            p = ops.contraction_plan(h, [ext[c] for c in mA], mA, [ext[c] for c in mB], mB, [ext["e"], ext["a"]], "ea", algo=r, **kw)
            d = p.describe()
            if d["kname"] == "gett_f32_stream_kernel" and d["splitK"] > 1 and (d["bm"], d["bn"], d["pf"], d["nt"]) == (96, 96, 3, int(nt)):
                assert d["splitK"] == split, d
                return p, d
            p.destroy()
            if (d["kernel"], d["splitK"]) == last:
                break
            last = (d["kernel"], d["splitK"])
    finally:
        os.environ.pop("CUTENSOR_AMD_F32_SPLITK", None)
    raise AssertionError("no 96 x 96 ring-3 streaming split-K candidate for %r %s %s split %d" % (ext, mA, mB, split))


def run_both(env, ext, mA="dcba", mB="ebcd", split=8, alpha=1.0, beta=0.0, nt=False, seed=0, reference=False, expect_flat=True):
    """One plan, the same buffers, both entries: returns the plan's description.  Asserts which entry ran, bitwise equality of the two
    outputs, that C is left alone when it is not D, and (reference=True) both outputs against fp64."""
    ct, ops, h, torch = env
    p, d = find_plan(env, ext, mA, mB, split, nt)
    g = torch.Generator(device="cuda")
    g.manual_seed(1000 + seed)
    shA, subA = _shape(ext, mA)
    shB, subB = _shape(ext, mB)
    A = torch.rand(shA, generator=g, device="cuda")
    B = torch.rand(shB, generator=g, device="cuda")
    C = torch.rand((ext["a"], ext["e"]), generator=g, device="cuda")
    C0 = C.clone()
    ws = torch.empty(max(p.required_workspace, 256), dtype=torch.uint8, device="cuda")
    outs = []
    for switch in (None, "0"):
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
        assert took_flat == (1 if (switch is None and expect_flat) else 0), (switch, took_flat, d)
        outs.append(D)
    assert torch.equal(C, C0)
    assert not torch.isnan(outs[0]).any() and not torch.isnan(outs[1]).any(), d
    assert torch.equal(outs[0], outs[1]), (d, float((outs[0] - outs[1]).abs().max()))
    if reference:
        ref = alpha * torch.einsum("%s,%s->ae" % (subA, subB), A.double(), B.double()) + beta * C.double()
        for D in outs:
            torch.testing.assert_close(D.double(), ref, rtol=1e-4, atol=0.0)
    p.destroy()
    return d


# K = d c b.  (a): 24 K-tiles in 8 slices of 3 — a slice starts in the middle of d and its carries cross c and b
EXT_A = dict(a=96, e=96, d=64, c=3, b=4)


@gpu
def test_three_tiles_per_slice_start_inside_the_fastest_digit(env):
    d = run_both(env, EXT_A, split=8, reference=True)
    assert d["kPerSlice"] == 96 and d["blocks"] == 8, d


@gpu
def test_slice_spans_two_values_of_the_third_digit(env):
    """(b) d = 64, c = 8, b = 4 in two slices: a slice holds b = 0, 1 / 2, 3 — the carry beyond the second digit re-derives the offsets"""
    d = run_both(env, dict(a=96, e=96, d=64, c=8, b=4), split=2, reference=True, seed=1)
    assert d["kPerSlice"] == 1024, d


@gpu
@pytest.mark.parametrize("split,tiles", [(8, 1), (4, 2)])
def test_fewer_tiles_per_slice_than_the_ring_is_deep(env, split, tiles):
    """(c) K = 256: one and two K-tiles per slice — the start-up paths that never reach the steady loop"""
    d = run_both(env, dict(a=96, e=96, d=64, c=2, b=2), split=split, reference=(split == 8), seed=2)
    assert d["kPerSlice"] == 32 * tiles, d


@gpu
def test_partial_tile_rows_are_clamped_and_not_stored(env):
    """(d) a = 80, e = 72: rows past the extents are clamped on the way in, the fold's Mtot / Ntot guards keep them out of D"""
    run_both(env, dict(EXT_A, a=80, e=72), split=8, reference=True, seed=3)


@gpu
def test_more_than_one_output_tile_takes_the_general_entry(env):
    """(e) a = e = 100 is 2 x 2 tiles of 96: the flat entry covers one-tile launches only, the launcher falls back (the counter says so)"""
    d = run_both(env, dict(EXT_A, a=100, e=100), split=8, reference=True, seed=4, expect_flat=False)
    assert d["blocks"] == 4 * 8, d


@gpu
@pytest.mark.parametrize("mA,mB,lay", [("dcba", "ebcd", (1, 0)), ("adcb", "ebcd", (0, 0)), ("adcb", "dcbe", (0, 1)), ("dcba", "dcbe", (1, 1))])
def test_four_operand_layouts(env, mA, mB, lay):
    """(f) each of A and B K-contiguous (d first) or free-contiguous (a / e first)"""
    d = run_both(env, EXT_A, mA=mA, mB=mB, split=8, reference=(lay == (0, 1)), seed=5)
    assert d["swapped"] == 0 and (d["layA"], d["layB"]) == lay, d


@gpu
def test_scalars_and_a_separate_c(env):
    """(g) alpha = 1.5, beta = -0.5 with C != D: C joins in the fold and is left untouched"""
    run_both(env, EXT_A, split=8, alpha=1.5, beta=-0.5, reference=True, seed=6)


@gpu
def test_nontemporal_twin_has_a_flat_entry_too(env):
    d = run_both(env, EXT_A, split=8, nt=True, reference=True, seed=7)
    assert d["nt"] == 1, d


def test_flat_entries_use_no_scratch_and_stay_within_the_register_budget(built, tmp_path):
    """What tests/test_kernel_resources.py checks for the existing kernels: the eight flat instantiations of the streaming kernel (four
    layouts x default / nontemporal stream) and the fold's instantiations have no private segment and spill nothing; a flat entry stays
    within the register budget of its launch bounds (one 8-wave workgroup per CU = two waves per SIMD: 512 / 2 = 256 vector registers
    per lane) and keeps the general entry's 72-KiB ring."""
    k = _kernel_notes(_code_object(tmp_path, "gett_f32_stream"))
    flat = {n: v for n, v in k.items() if "gett_f32_stream_kernel" in n and n.endswith("StreamFlatParamsE")}
    assert len(flat) == 8, sorted(k)
    fold = {n: v for n, v in k.items() if "splitk_reduce_frag_flat_kernel" in n}
    assert len(fold) == 4, sorted(k)          # 2 x 2, 3 x 3, 4 x 4 fragments per wave, and the run-time decode
    bad = {n: v for n, v in {**flat, **fold}.items()
           if v.get("private_segment_fixed_size", 0) or v.get("vgpr_spill_count", 0) or v.get("sgpr_spill_count", 0)}
    assert not bad, bad
    for name, v in flat.items():
        twin = name.replace("Li3ELi6E", "Li3ELi0E").replace("Li3ELi7E", "Li3ELi5E").replace("NS_16StreamFlatParamsE", "NS_10GettParamsE")
        assert twin in k, (name, twin)
        assert v["vgpr_count"] <= 256, (name, v)
        assert v["group_segment_fixed_size"] == k[twin]["group_segment_fixed_size"] == 3 * 24 * 1024, (name, v)
