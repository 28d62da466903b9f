"""fp32 contractions under a reduced-precision compute descriptor (csrc/kernels/gett_gen_f32x.inc) on the GPU.

COMPUTE_DESC_16BF / _16F: products of the operands rounded once to bf16 / fp16; COMPUTE_DESC_TF32: three bf16 products of a hi / lo
split; fp32 accumulators and epilogue.  Every case but the default-planner ones runs with CUTENSOR_AMD_F32X=force, asserts the element of
the plan's description and that the general family's launch counter went up.

* exact: integer data (tests/exact_data.py) comes back bit for bit in all three modes; the lo planes on A in [-4095, 4095];
* meaning: 16BF / 16F equal the fp64 contraction of the ROUNDED operands within K 2^-23 sum |a^||b^| (a full-fp32 kernel misses that by
  orders of magnitude: the rounding of the operands is 2^-9 / 2^-12 per factor);
* accuracy against the true result: (2.01 u + K 2^-23) mag with u = 2^-8 (16BF), 2^-11 (16F); (3.1 2^-16 + K 2^-23) mag for TF32 —
  worst-case bounds: two roundings of relative u per product (+ u^2), three dropped terms of u^2 each for the split, one fp32 ulp per
  accumulation step.  A one-term kernel misses the TF32 bound at K = 8 / 64 by a factor of about 100 / 25.
Figures are printed before they are asserted (pytest -s)."""
import numpy as np
import pytest

import exact_cases as xc
import exact_data as xd

pytestmark = pytest.mark.gpu

ELEM = {"16BF": 5, "16F": 6, "TF32": 7}
MODES = ("16BF", "16F", "TF32")
U = {"16BF": 2.0 ** -8, "16F": 2.0 ** -11}
LAYOUTS = xc.LAYOUTS


def bound_factor(compute, K):
    head = 3.1 * 2.0 ** -16 if compute == "TF32" else 2.01 * U[compute]
    return head + K * 2.0 ** -23


@pytest.fixture(scope="module")
def env(built):
    import torch
    assert torch.cuda.is_available()
    from cudalibrarysamples_amd import cutensor as ct, ops
    return ct, ops, ops.Handle(), torch


@pytest.fixture
def force(monkeypatch):
    monkeypatch.setenv("CUTENSOR_AMD_F32X", "force")


def make_plan(env, ext, modes, compute, pad=(0, 0, 0), align=128, ws_limit=1 << 28):
    import guarded as gd
    ct, ops, h, torch = env
    e = lambda m: [ext[c] for c in m]   # noqa: E731
    # pad: pitch padding of A, B, D — and of C, when a fourth entry gives C a pitch of its own
    st = [gd.packed_strides(e(modes[min(i, 2)]), pad[i]) for i in range(len(pad))]
    return ops.contraction_plan(h, e(modes[0]), modes[0], e(modes[1]), modes[1], e(modes[2]), modes[2], dtype=ct.R_32F, strideA=st[0], strideB=st[1],
                                strideC=st[-1], strideD=st[2] if len(pad) > 3 else None, alignment=align, compute=compute, workspace_limit=ws_limit)


def contract(env, plan, ext, modes, A, B, C, alpha=1.0, beta=0.0, pad=(0, 0, 0), off=0, inplace=False, on_path=True):
    """A, B, C: logical host tensors (dimensions in the order of the mode strings).  D lives in a NaN-filled buffer; returns (D, description)"""
    ct, ops, h, torch = env
    d = plan.describe()
    inner = d
    e = lambda m: [ext[c] for c in m]   # noqa: E731
    pa, pb = xc.Placed(e(modes[0]), "float32", pad[0], off), xc.Placed(e(modes[1]), "float32", pad[1], off)
    pa.set(A)
    pb.set(B)
    pd = xc.Placed(e(modes[2]), "float32", pad[2], off)
    pc = None
    if beta:
        pc = pd if inplace else xc.Placed(e(modes[2]), "float32", pad[-1], off)
        pc.set(C)
    ws = torch.full((max(plan.required_workspace, 256),), 0xFF, dtype=torch.uint8, device="cuda")
    before = ct.launch_counts()["gen"]
    plan.contract(alpha, pa.ptr, pb.ptr, beta, pc.ptr if pc else 0, pd.ptr, ws.data_ptr(), plan.required_workspace)
    torch.cuda.synchronize()
    if on_path:
        assert ct.launch_counts()["gen"] > before, inner
    pd.check_outside(str(d))
    return pd.get(), d


def on_f32x(d, compute, vec=None, split=None):
    assert d["family"] == 2 and d["kname"] == "gett_gen_f32x_kernel" and d["elem"] == ELEM[compute], d
    if vec is not None:
        assert d["vec"] == vec, d
    if split is not None:
        assert (d["splitK"] > 1) == split, d


# ---- 4. exact, zero tolerance ---------------------------------------------------------------------------------------------------------
def _exact(env, cid, ext, modes, compute, vec=None, split=None, tile=None, alpha=1.0, beta=0.0, pad=(0, 0, 0), off=0, align=128, inplace=False, check=on_f32x):
    ct, ops, h, torch = env
    case = xc.Case(cid, "float32", ext, modes, alpha=alpha, beta=beta, pad=pad, off=off, align=align)
    plan = make_plan(env, ext, modes, compute, pad, align)
    try:
        d = plan.describe()
        check(d, compute, vec, split)
        if tile is not None:
            assert (d["bm"], d["bn"]) == (tile, tile), d
        for swap in (False, True):
            A, B, C = xd.make_exact(case, swap)
            xd.check_draw(case, A, B, C, swap)
            want, _ = xd.expected(case, xd.exact_reference(case, A, B, C, device="cuda"))
            got, _ = contract(env, plan, ext, modes, A, B, C, alpha, beta, pad, off, inplace)
            xd.assert_exact(got, want, "%s %s draw %d %s" % (cid, compute, int(swap), d))
    finally:
        plan.destroy()


@pytest.mark.parametrize("compute", MODES)
@pytest.mark.parametrize("lay", range(4))
def test_exact_layouts_tiles_and_widths(env, force, compute, lay):
    mA, mB = LAYOUTS[lay]
    L = xc.LNAME[(mA, mB)]
    s = xc.SCALARS32
    # the 128 x 128 tile (169 output tiles fill the chip) and the 64 x 64 one, 16-byte loads
    _exact(env, "f32x_big_%s" % L, dict(m=1664, n=1600, k=200), (mA, mB, "mn"), compute, vec=4, tile=128, alpha=s[lay][0], beta=s[lay][1])
    _exact(env, "f32x_small_%s" % L, dict(m=200, n=136, k=1000), (mA, mB, "mn"), compute, vec=4, tile=64, alpha=s[lay + 1][0], beta=s[lay + 1][1])
    # 4-byte gathers: odd extents; an odd element offset at element alignment (both tiles)
    _exact(env, "f32x_odd_%s" % L, dict(m=67, n=45, k=333), (mA, mB, "mn"), compute, vec=1, tile=64, alpha=s[lay + 2][0], beta=s[lay + 2][1])
    _exact(env, "f32x_big_off_%s" % L, dict(m=1664, n=1600, k=72), (mA, mB, "mn"), compute, vec=1, tile=128, off=3, align=4)


@pytest.mark.parametrize("compute", MODES)
def test_exact_groups_pitches_split_k_and_in_place(env, force, compute):
    s = xc.SCALARS32
    # two contracted modes, the fastest one ragged against the K-tile: with 16-byte loads (36) and without (37)
    _exact(env, "f32x_two_k_36", dict(m=136, n=136, k=36, j=25), ("kmj", "kjn", "mn"), compute, vec=4, alpha=s[1][0], beta=s[1][1])
    _exact(env, "f32x_two_k_37", dict(m=136, n=72, k=37, j=25), ("kmj", "kjn", "mn"), compute, vec=1, alpha=s[2][0], beta=s[2][1])
    # a batch mode
    _exact(env, "f32x_batch", dict(m=132, n=68, k=64, l=3), ("mkl", "knl", "mnl"), compute, vec=4, alpha=0.5, beta=1.0)
    _exact(env, "f32x_batch_kfirst", dict(m=132, n=68, k=64, l=3), ("kml", "nkl", "mnl"), compute, vec=4, alpha=-2.0, beta=0.0)
    # padded pitches: lanes kept at a 16-byte-aligned offset, lost at an odd one
    _exact(env, "f32x_pitch4", dict(m=264, n=136, k=128), ("mk", "kn", "mn"), compute, vec=4, pad=(4, 8, 4), off=4, align=16, alpha=1.0, beta=-0.5)
    _exact(env, "f32x_pitch_odd", dict(m=262, n=134, k=134), ("km", "kn", "mn"), compute, vec=1, pad=(5, 3, 1), off=3, align=4, alpha=0.5, beta=1.0)
    # split-K: fp32 partials folded by the common fold kernel; in place (C = D)
    _exact(env, "f32x_splitk", dict(m=128, n=128, k=65536), ("km", "kn", "mn"), compute, vec=4, split=True, alpha=-2.0, beta=1.0)
    _exact(env, "f32x_splitk_odd", dict(m=100, n=60, k=4099), ("mk", "kn", "mn"), compute, vec=1, split=True, alpha=0.5, beta=-0.5, inplace=True)
    for i, (al, be) in enumerate(s):
        _exact(env, "f32x_scalars_%d" % i, dict(m=200, n=136, k=104), ("km", "nk", "mn"), compute, vec=4, alpha=al, beta=be, inplace=bool(i & 1))


@pytest.mark.parametrize("compute", MODES)
def test_exact_lone_and_peeled_plans_recurse_into_the_path(env, force, compute):
    """a mode that one input alone carries (reduced first) and an oversized mode group (peeled): the inner plans are made with the
    descriptor's compute type and take the reduced-precision kernels by themselves"""
    def lone(d, compute, vec, split):
        assert d.get("lone_reduce_A") == 1 and d["family"] == 2 and d["elem"] == ELEM[compute], d

    def peeled(d, compute, vec, split):
        assert d.get("peel_launches", 0) >= 2 and d["family"] == 2 and d["elem"] == ELEM[compute], d
    _exact(env, "f32x_lone_A", xc.LONE, ("kji", "lk", "li"), compute, alpha=-2.0, beta=1.0, check=lone)
    _exact(env, "f32x_peeled", xc.PEEL, ("paqbrcsdte", "xpyqzrst", "abxcydze"), compute, alpha=0.5, beta=1.0, check=peeled)


@pytest.mark.parametrize("compute", MODES)
def test_exact_row_and_column_groups_that_do_not_fuse(env, force, compute):
    """M and N of two modes each, interleaved in D: the mixed-radix row clamp and epilogue offsets, in ONE launch (xc.UNFUSED).  The family
    has no switch that forces split-K: a second case with k = 517 splits by itself."""
    def unfused(d, compute, vec, split):
        on_f32x(d, compute, vec, split)
        xc.one_launch(d)
    _exact(env, "f32x_unfused", xc.UNFUSED, xc.UNFUSED_MODES, compute, vec=1, tile=64, alpha=-2.0, beta=0.5, pad=xc.UNFUSED_PAD, check=unfused)
    # the same groups with a K long enough to split by itself: the partial walk and the fold on groups that do not fuse
    _exact(env, "f32x_unfused_splitk", xc.UNFUSED_LONG, xc.UNFUSED_MODES, compute, vec=1, split=True, tile=64, alpha=-2.0, beta=0.5, pad=xc.UNFUSED_PAD)


@pytest.mark.parametrize("roles", ("A_wide", "B_wide"))
@pytest.mark.parametrize("lay", (0, 3))
def test_exact_lo_planes_of_the_tf32_split(env, force, roles, lay):
    """One operand integer in [-4095, 4095]: hi + lo is exact (12 bits = 8 + a remainder of at most 4 significant bits) and lo != 0 for
    most of the draw; the other in {+-1, +-2, +-3}; K = 1000: sum |a||b| <= 1.23e7 < 2^24.  Exact under TF32 only if the lo planes are
    staged and multiplied: a one-term kernel gets (nearly) every output wrong."""
    ct, ops, h, torch = env
    mA, mB = LAYOUTS[lay]
    ext, modes = dict(m=200, n=136, k=1000), (mA, mB, "mn")
    rng = np.random.default_rng([4095, lay, roles == "A_wide"])
    shape = lambda m: [ext[c] for c in m]   # noqa: E731
    wide = lambda sh: rng.integers(-4095, 4096, size=sh).astype(np.float32)   # noqa: E731
    small = lambda sh: np.array([-3, -2, -1, 1, 2, 3], dtype=np.float32)[rng.integers(0, 6, size=sh)]   # noqa: E731
    A = torch.from_numpy(wide(shape(mA)) if roles == "A_wide" else small(shape(mA)))
    B = torch.from_numpy(small(shape(mB)) if roles == "A_wide" else wide(shape(mB)))
    w = A if roles == "A_wide" else B
    hi = w.to(torch.bfloat16).to(torch.float32)
    lo = (w - hi)
    assert bool((lo.to(torch.bfloat16).to(torch.float32) == lo).all()), "hi + lo is not exact on this draw"
    assert float((lo != 0).float().mean()) > 0.5
    # the bound from the draw: the largest |a| over m times the largest |b| over n, summed over k
    am = A.abs().amax(dim=mA.index("m")).double()
    bm = B.abs().amax(dim=mB.index("n")).double()
    assert float((am * bm).sum()) < 2.0 ** 24
    want = torch.from_numpy(np.einsum("%s,%s->mn" % (mA, mB), A.numpy().astype(np.int64), B.numpy().astype(np.int64)).astype(np.float64))
    plan = make_plan(env, ext, modes, "TF32")
    try:
        on_f32x(plan.describe(), "TF32", vec=4)
        got, d = contract(env, plan, ext, modes, A, B, None)
        xd.assert_exact(got, want, "lo planes %s %s" % (roles, d))
    finally:
        plan.destroy()


# ---- 5. the meaning of the mode -------------------------------------------------------------------------------------------------------
def _away_from_zero(torch, gen, shape):
    """+-U(2^-4, 1): away from fp16's subnormal range"""
    mag = torch.rand(shape, generator=gen, dtype=torch.float64) * (1.0 - 2.0 ** -4) + 2.0 ** -4
    sign = torch.randint(0, 2, shape, generator=gen, dtype=torch.int64) * 2 - 1
    return (mag * sign).to(torch.float32)


ROUND = {"16BF": "bfloat16", "16F": "float16"}


@pytest.mark.parametrize("compute,K", [("16BF", 8), ("16BF", 64), ("16BF", 256), ("16F", 8), ("16F", 64)])
def test_products_are_those_of_the_rounded_operands(env, force, compute, K):
    """D equals the fp64 contraction of the operands rounded to the mode's 16-bit type within K 2^-23 sum |a^||b^|: products of two
    16-bit values are exact in fp32, each accumulation step loses at most one fp32 ulp whatever the order.  A kernel that multiplies
    the unrounded fp32 operands is off by about 2^-9 (bf16) / 2^-12 (fp16) per factor: orders of magnitude above the bound."""
    ct, ops, h, torch = env
    gen = torch.Generator().manual_seed(1000 + K)
    ext, modes = dict(m=192, n=160, k=K), ("km", "kn", "mn")
    A, B = _away_from_zero(torch, gen, [K, 192]), _away_from_zero(torch, gen, [K, 160])
    rt = getattr(torch, ROUND[compute])
    ar, br = A.to(rt).double(), B.to(rt).double()
    ref = torch.einsum("km,kn->mn", ar, br)
    tol = K * 2.0 ** -23 * torch.einsum("km,kn->mn", ar.abs(), br.abs())
    plan = make_plan(env, ext, modes, compute)
    try:
        on_f32x(plan.describe(), compute, vec=4)
        got, d = contract(env, plan, ext, modes, A, B, None)
    finally:
        plan.destroy()
    err = (got.double() - ref).abs()
    unrounded = (torch.einsum("km,kn->mn", A.double(), B.double()) - ref).abs()
    print("f32x meaning %s K=%d: worst err / bound %.3g (the unrounded fp32 product would be at %.3g)" % (
        compute, K, float((err / tol).max()), float((unrounded / tol).max())))
    assert bool((err <= tol).all()), (compute, K, float((err / tol).max()))


# ---- 6. accuracy against the true result ----------------------------------------------------------------------------------------------
def _draw(torch, gen, compute, shape):
    if compute == "16F":
        return _away_from_zero(torch, gen, shape)
    return (torch.rand(shape, generator=gen, dtype=torch.float64) * 2 - 1).to(torch.float32)


ACC_SHAPES = [
    ("k8", dict(m=192, n=160, k=8), ("km", "kn", "mn"), 1.0, 0.0),
    ("k64", dict(m=192, n=160, k=64), ("mk", "kn", "mn"), 1.0, 0.0),
    ("k1000", dict(m=200, n=136, k=1000), ("km", "nk", "mn"), -2.0, 0.5),
    ("k4096", dict(m=256, n=192, k=4096), ("mk", "nk", "mn"), 1.0, 0.0),
    ("k4096_big_tile", dict(m=1664, n=1600, k=4096), ("km", "kn", "mn"), 0.5, 0.0),
    ("ref_50", dict(m=50, n=50, k=50), ("km", "kn", "mn"), 1.0, 0.0),                                      # extents of 50: 4-byte gathers (50 % 4 != 0)
    ("ref_mlik", dict(m=20, l=50, i=50, k=50, j=50), ("kilm", "mjkl", "jil"), 1.0, 1.0),                     # 'mlik,lkjm->lij': K = 1000
    ("ref_k8_odd", dict(m=51, n=49, k=8), ("mk", "kn", "mn"), 1.0, 0.0),
]


@pytest.mark.parametrize("compute", MODES)
@pytest.mark.parametrize("name,ext,modes,alpha,beta", ACC_SHAPES, ids=[s[0] for s in ACC_SHAPES])
def test_accuracy_against_the_true_result(env, force, compute, name, ext, modes, alpha, beta):
    ct, ops, h, torch = env
    gen = torch.Generator().manual_seed(77)
    sh = lambda m: [ext[c] for c in m]   # noqa: E731
    A, B, C = _draw(torch, gen, compute, sh(modes[0])), _draw(torch, gen, compute, sh(modes[1])), _draw(torch, gen, compute, sh(modes[2]))
    eq = "%s,%s->%s" % modes
    K = int(np.prod([ext[c] for c in modes[0] if c in modes[1] and c not in modes[2]]))
    a64, b64, c64 = A.cuda().double(), B.cuda().double(), C.double()
    ref = alpha * torch.einsum(eq, a64, b64).cpu() + beta * c64
    mag = abs(alpha) * torch.einsum(eq, a64.abs(), b64.abs()).cpu() + abs(beta) * c64.abs()
    plan = make_plan(env, ext, modes, compute)
    try:
        on_f32x(plan.describe(), compute)
        got, d = contract(env, plan, ext, modes, A, B, C, alpha, beta)
    finally:
        plan.destroy()
    tol = bound_factor(compute, K) * mag
    err = (got.double() - ref).abs()
    print("f32x accuracy %s %s K=%d: worst err / mag %.3g, bound %.3g (ratio %.3g)" % (
        compute, name, K, float((err / mag).max()), bound_factor(compute, K), float((err / tol).max())))
    assert bool((err <= tol).all()), (compute, name, float((err / tol).max()), d)


# ---- 7. non-finite values -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compute", ("TF32", "16BF"))
def test_an_infinity_in_a_gives_infinity_in_its_row_only(env, force, compute):
    ct, ops, h, torch = env
    gen = torch.Generator().manual_seed(5)
    ext, modes = dict(m=136, n=72, k=100), ("km", "kn", "mn")
    A = (torch.rand([100, 136], generator=gen, dtype=torch.float64) * 2 - 1).to(torch.float32)
    B = (torch.rand([100, 72], generator=gen, dtype=torch.float64) * 0.9 + 0.1).to(torch.float32)       # positive
    A[17, 33] = float("inf")
    plan = make_plan(env, ext, modes, compute)
    try:
        on_f32x(plan.describe(), compute, vec=4)
        got, d = contract(env, plan, ext, modes, A, B, None)
    finally:
        plan.destroy()
    assert bool((got[33] == float("inf")).all()), got[33]
    rows = [i for i in range(136) if i != 33]
    Af = A.clone()
    Af[17, 33] = 0.0
    ref = torch.einsum("km,kn->mn", Af.double(), B.double())[rows]
    mag = torch.einsum("km,kn->mn", Af.double().abs(), B.double().abs())[rows]
    assert bool(torch.isfinite(got[rows]).all())
    assert bool(((got[rows].double() - ref).abs() <= bound_factor(compute, 100) * mag).all())


# ---- 8. the default planner -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compute", MODES)
def test_default_planner_meets_the_bound_of_the_mode_asked_for(env, compute):
    """no switch: whichever path the planner takes for 4096^3, the result is within the bound of the mode that was asked for (the fp32 path
    is at least as accurate)"""
    ct, ops, h, torch = env
    gen = torch.Generator().manual_seed(11)
    E = 4096
    ext, modes = dict(m=E, n=E, k=E), ("km", "kn", "mn")
    A, B = _draw(torch, gen, compute, [E, E]), _draw(torch, gen, compute, [E, E])
    a, b = A.cuda(), B.cuda()
    plan = make_plan(env, ext, modes, compute, ws_limit=None)
    try:
        d = plan.describe()
        assert (d["family"] == 0) or (d["family"] == 2 and d["elem"] == ELEM[compute]), d
        out = torch.full((E, E), float("nan"), dtype=torch.float32, device="cuda")          # D[m, n] with m fastest: out[n, m]
        ws = torch.empty(max(plan.required_workspace, 256), dtype=torch.uint8, device="cuda")
        plan.contract(1.0, a.data_ptr(), b.data_ptr(), 0.0, 0, out.data_ptr(), ws.data_ptr(), plan.required_workspace)
        torch.cuda.synchronize()
    finally:
        plan.destroy()
    rows = torch.arange(0, E, 8, device="cuda")                                                # 512 rows of n, every m
    # A[k, m] in mode order (k, m) means k FASTEST: the buffer is row-major [m][k]; likewise B is [n][k]
    am, bn = a.reshape(E, E).double(), b.reshape(E, E)[rows].double()
    ref = bn @ am.t()
    mag = bn.abs() @ am.abs().t()
    err = (out[rows].double() - ref).abs()
    print("f32x default planner %s 4096^3: family %d, worst err / mag %.3g, bound %.3g" % (compute, d["family"], float((err / mag).max()), bound_factor(compute, E)))
    assert bool((err <= bound_factor(compute, E) * mag).all()), d


def test_the_headline_einsum_under_tf32_keeps_its_fp32_split_k_plan(env):
    """'abcd,dcbe->ae' is split-K-dominated (one 96 x 96 output, K = 262144): the committed sweep (profiles/f32x_f32_compute.jsonl) does not
    show the reduced-precision kernels faster there, so a TF32 plan is the fp32 plan"""
    plan = make_plan(env, xc.HEADLINE, xc.HEAD_MODES, "TF32", ws_limit=1 << 30)
    ref = make_plan(env, xc.HEADLINE, xc.HEAD_MODES, "32F", ws_limit=1 << 30)
    try:
        d, r = plan.describe(), ref.describe()
        assert d["family"] == 0 and d["splitK"] == 256 and d == r, (d, r)
    finally:
        plan.destroy()
        ref.destroy()
