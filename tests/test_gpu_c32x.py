"""complex64 contractions under a reduced-precision compute descriptor (csrc/kernels/gett_gen_c32x.inc) on the GPU.

A complex product is four real products; COMPUTE_DESC_16BF / _16F form each from parts rounded once to bf16 / fp16, COMPUTE_DESC_TF32 from
three bf16 products of a hi / lo split; fp32 accumulators, fp32 complex epilogue.  Every case but the default-planner ones runs with
CUTENSOR_AMD_F32X=force, asserts the plan's description and that the general family's launch counter went up; results live in NaN-filled
guarded buffers.  Expected values come from int64 / complex128 arithmetic on the host data, never from the library.

* exact: integer data (tests/exact_data.py, parts in {+-1, +-2, +-3}) comes back bit for bit in all three modes; the lo planes of the
  TF32 split on parts in [-4095, 4095];
* meaning: 16BF / 16F equal the complex128 contraction of the operands with both parts ROUNDED within 2K 2^-23 sum (|a^r|+|a^i|)(|b^r|+|b^i|)
  per component (a full-fp32 kernel misses that by orders of magnitude);
* accuracy against the true result, per component: (2.01 u + 2K 2^-23) mag with u = 2^-8 (16BF), 2^-11 (16F); (3.1 2^-16 + 2K 2^-23) mag
  for TF32, mag = (|al_r|+|al_i|) sum (|a_r|+|a_i|)(|b_r|+|b_i|) + (|be_r|+|be_i|)(|c_r|+|c_i|): the real-data heads (two roundings of
  relative u per real product; three dropped terms of u^2 for the split), one fp32 ulp for each of the 2K accumulation steps of a
  component.
Figures are printed before they are asserted (pytest -s)."""
import numpy as np
import pytest

import exact_cases as xc
import exact_data as xd

pytestmark = pytest.mark.gpu

ELEM = {"16BF": 10, "16F": 11, "TF32": 12}
MODES = ("16BF", "16F", "TF32")
U = {"16BF": 2.0 ** -8, "16F": 2.0 ** -11}
KNAME = "gett_gen_c32x_kernel"
LAYOUTS = xc.LAYOUTS
# alpha, beta with non-zero imaginary parts, every part an integer or a half
SCALARS = [(1 + 1j, 0.0), (-2 + 0.5j, 1 - 0.5j), (0.5 - 1j, -0.5 + 2j), (-1j, 0.0), (1 - 2j, 1j), (2 + 0.5j, 0.0)]


def bound_factor(compute, K):
    head = 3.1 * 2.0 ** -16 if compute == "TF32" else 2.01 * U[compute]
    return head + 2 * K * 2.0 ** -23


def l1(z):
    """|re| + |im| of a python scalar or a tensor, in fp64"""
    if isinstance(z, (int, float, complex)):
        z = complex(z)
        return abs(z.real) + abs(z.imag)
    return z.real.double().abs() + z.imag.double().abs()


def comp_err(got, ref):
    """the larger of the two components' errors, per element"""
    import torch
    g = got.to(torch.complex128)
    return torch.maximum((g.real - ref.real).abs(), (g.imag - ref.imag).abs())


@pytest.fixture(scope="module")
def env(built):
    import torch
    assert torch.cuda.is_available()
    from cudalibrarysamples_amd import cutensor as ct, ops
    return ct, ops, ops.Handle(), torch


@pytest.fixture
def force(monkeypatch):
    monkeypatch.setenv("CUTENSOR_AMD_F32X", "force")


def make_plan(env, ext, modes, compute, pad=(0, 0, 0), align=128, ws_limit=1 << 28, conj=(False, False, False)):
    import guarded as gd
    ct, ops, h, torch = env
    e = lambda m: [ext[c] for c in m]   # noqa: E731
    # pad: pitch padding of A, B, D — and of C, when a fourth entry gives C a pitch of its own
    st = [gd.packed_strides(e(modes[min(i, 2)]), pad[i]) for i in range(len(pad))]
    op = [ct.OP_CONJ if c else ct.OP_IDENTITY for c in conj]
    return ops.contraction_plan(h, e(modes[0]), modes[0], e(modes[1]), modes[1], e(modes[2]), modes[2], dtype=ct.C_32F, strideA=st[0], strideB=st[1],
                                strideC=st[-1], strideD=st[2] if len(pad) > 3 else None, alignment=align, compute=compute, workspace_limit=ws_limit, opA=op[0], opB=op[1], opC=op[2])


def contract(env, plan, ext, modes, A, B, C, alpha=1.0, beta=0.0, pad=(0, 0, 0), off=0, inplace=False, on_path=True):
    """A, B, C: logical host tensors (dimensions in the order of the mode strings).  D lives in a NaN-filled buffer; returns (D, description)"""
    ct, ops, h, torch = env
    d = plan.describe()
    e = lambda m: [ext[c] for c in m]   # noqa: E731
    pa, pb = xc.Placed(e(modes[0]), "complex64", pad[0], off), xc.Placed(e(modes[1]), "complex64", pad[1], off)
    pa.set(A)
    pb.set(B)
    pd = xc.Placed(e(modes[2]), "complex64", pad[2], off)
    pc = None
    if beta:
        pc = pd if inplace else xc.Placed(e(modes[2]), "complex64", pad[-1], off)
        pc.set(C)
    ws = torch.full((max(plan.required_workspace, 256),), 0xFF, dtype=torch.uint8, device="cuda")
    before = ct.launch_counts()["gen"]
    plan.contract(alpha, pa.ptr, pb.ptr, beta, pc.ptr if pc else 0, pd.ptr, ws.data_ptr(), plan.required_workspace)      # beta == 0: C absent
    torch.cuda.synchronize()
    if on_path:
        assert ct.launch_counts()["gen"] > before, d
    pd.check_outside(str(d))
    return pd.get(), d


def on_c32x(d, compute, vec=None, split=None):
    assert d["family"] == 2 and d["kname"] == KNAME and d["elem"] == ELEM[compute], d
    if vec is not None:
        assert d["vec"] == vec, d
    if split is not None:
        assert (d["splitK"] > 1) == split, d


# ---- 1. exact, zero tolerance ---------------------------------------------------------------------------------------------------------
_REF = {}      # (case id, draw) -> (A, B, C, expected): made once, shared by the three modes, never written to


def _exact_data(case, swap):
    key = (case.id, swap)
    if key not in _REF:
        if len(_REF) >= 4:
            _REF.clear()
        A, B, C = xd.make_exact(case, swap)
        xd.check_draw(case, A, B, C, swap)
        # the bound of a component, from the draw: |a_r b_r - a_i b_i| and |a_r b_i + a_i b_r| are at most max(|a_r|, |a_i|)(|b_r| + |b_i|), so
        # every partial sum is an integer below 2^24, and alpha * sum + beta * c a multiple of 1/2 below 2^23 (parts of alpha, beta: halves)
        import torch
        m = xd.Modes(*case.modes[:3])
        K = int(np.prod([case.ext[c] for c in m.K + m.loneA + m.loneB]))
        comp = K * float(torch.maximum(A.real.abs(), A.imag.abs()).max()) * float(l1(B).max())
        total = max(1.0, l1(case.alpha)) * comp + l1(case.beta) * float(l1(C).max())
        assert total < 2.0 ** 23, (case.id, total)
        want, _ = xd.expected(case, xd.exact_reference(case, A, B, C, device="cuda"))
        _REF[key] = (A, B, C, want)
    return _REF[key]


def _exact(env, cid, ext, modes, compute, vec=None, split=None, tile=None, alpha=1.0, beta=0.0, pad=(0, 0, 0), off=0, align=128, inplace=False,
           conj=(False, False, False), check=on_c32x):
    case = xc.Case(cid, "complex64", ext, modes, alpha=alpha, beta=beta, pad=pad, off=off, align=align, conj=conj)
    plan = make_plan(env, ext, modes, compute, pad, align, conj=conj)
    try:
        d = plan.describe()
        check(d, compute, vec, split)
        if tile is not None:
            assert (d["bm"], d["bn"]) == (tile, tile), d
        for swap in (False, True):
            A, B, C, want = _exact_data(case, swap)
            got, _ = contract(env, plan, ext, modes, A, B, C, alpha, beta, pad, off, inplace)
            xd.assert_exact(got, want, "%s %s draw %d %s" % (cid, compute, int(swap), d))
    finally:
        plan.destroy()


@pytest.mark.parametrize("compute", MODES)
@pytest.mark.parametrize("lay", range(4))
def test_exact_layouts_tiles_and_widths(env, force, compute, lay):
    mA, mB = LAYOUTS[lay]
    L = xc.LNAME[(mA, mB)]
    s = SCALARS
    # the 128 x 128 tile (169 output tiles) and the 64 x 64 one, 16-byte loads
    _exact(env, "c32x_big_%s" % L, dict(m=1664, n=1600, k=72), (mA, mB, "mn"), compute, vec=2, tile=128, alpha=s[lay][0], beta=s[lay][1])
    _exact(env, "c32x_small_%s" % L, dict(m=200, n=136, k=200), (mA, mB, "mn"), compute, vec=2, tile=64, alpha=s[lay + 1][0], beta=s[lay + 1][1])
    # 8-byte gathers: odd extents and an odd element offset at 8-byte alignment (both tiles)
    _exact(env, "c32x_odd_%s" % L, dict(m=67, n=45, k=333), (mA, mB, "mn"), compute, vec=1, tile=64, off=1, align=8, alpha=s[lay + 2][0], beta=s[lay + 2][1])
    _exact(env, "c32x_big_off_%s" % L, dict(m=1664, n=1600, k=40), (mA, mB, "mn"), compute, vec=1, tile=128, off=3, align=8)


@pytest.mark.parametrize("compute", MODES)
def test_exact_groups_pitches_split_k_and_in_place(env, force, compute):
    s = SCALARS
    # two contracted modes, the fastest one ragged against the K-tile: with 16-byte loads (36) and without (37)
    _exact(env, "c32x_two_k_36", dict(m=136, n=136, k=36, j=25), ("kmj", "kjn", "mn"), compute, vec=2, alpha=s[1][0], beta=s[1][1])
    _exact(env, "c32x_two_k_37", dict(m=136, n=72, k=37, j=25), ("kmj", "kjn", "mn"), compute, vec=1, alpha=s[2][0], beta=s[2][1])
    # a batch mode
    _exact(env, "c32x_batch", dict(m=132, n=68, k=64, l=3), ("mkl", "knl", "mnl"), compute, vec=2, alpha=0.5 + 1j, beta=1.0)
    _exact(env, "c32x_batch_kfirst", dict(m=132, n=68, k=64, l=3), ("kml", "nkl", "mnl"), compute, vec=2, alpha=-2.0, beta=0.0)
    # padded pitches: lanes kept at a 16-byte-aligned offset, lost at an odd one
    _exact(env, "c32x_pitch2", dict(m=264, n=136, k=128), ("mk", "kn", "mn"), compute, vec=2, pad=(2, 4, 2), off=2, align=16, alpha=1.0, beta=-0.5j)
    _exact(env, "c32x_pitch_odd", dict(m=262, n=134, k=134), ("km", "kn", "mn"), compute, vec=1, pad=(5, 3, 1), off=3, align=8, alpha=0.5j, beta=1.0)
    # split-K: float2 partials folded by the complex64 fold; in place (C = D)
    _exact(env, "c32x_splitk", dict(m=128, n=128, k=65536), ("km", "kn", "mn"), compute, vec=2, split=True, alpha=-2 + 0.5j, beta=1 - 0.5j)
    _exact(env, "c32x_splitk_odd", dict(m=100, n=60, k=4099), ("mk", "kn", "mn"), compute, vec=1, split=True, alpha=0.5 - 1j, beta=-0.5 + 2j, inplace=True)
    for i, (al, be) in enumerate(s):
        _exact(env, "c32x_scalars_%d" % i, dict(m=200, n=136, k=104), ("km", "nk", "mn"), compute, vec=2, alpha=al, beta=be, inplace=bool(i & 1))


@pytest.mark.parametrize("compute", MODES)
def test_exact_row_and_column_groups_that_do_not_fuse(env, force, compute):
    """M and N of two modes each, interleaved in D: the mixed-radix row clamp and epilogue offsets, in ONE launch (xc.UNFUSED).  The family
    has no switch that forces split-K: a second case with k = 517 splits by itself."""
    def unfused(d, compute, vec, split):
        on_c32x(d, compute, vec, split)
        xc.one_launch(d)
    _exact(env, "c32x_unfused", xc.UNFUSED, xc.UNFUSED_MODES, compute, vec=1, tile=64, alpha=0.5 - 1j, beta=-0.5 + 2j, pad=xc.UNFUSED_PAD,
           conj=(False, True, True), check=unfused)
    # the same groups with a K long enough to split by itself: the partial walk and the fold on groups that do not fuse
    _exact(env, "c32x_unfused_splitk", xc.UNFUSED_LONG, xc.UNFUSED_MODES, compute, vec=1, split=True, tile=64, alpha=0.5 - 1j, beta=-0.5 + 2j,
           pad=xc.UNFUSED_PAD, conj=(False, True, True))


@pytest.mark.parametrize("compute", MODES)
def test_exact_every_conjugation(env, force, compute):
    for i in range(1, 8):
        conj = (bool(i & 1), bool(i & 2), bool(i & 4))
        _exact(env, "c32x_conj_%d" % i, dict(m=72, n=136, k=104), (("km", "nk") if i & 1 else ("mk", "kn")) + ("mn",), compute, vec=2, conj=conj,
               alpha=-2 + 0.5j, beta=1 - 0.5j)


@pytest.mark.parametrize("compute", MODES)
def test_exact_lone_and_peeled_plans_recurse_into_the_path(env, force, compute):
    """a mode that one input alone carries (reduced first) and an oversized mode group (peeled): the inner plans are made with the
    descriptor's compute type and take the reduced-precision kernels by themselves"""
    def lone(d, compute, vec, split):
        assert d.get("lone_reduce_A") == 1 and d["family"] == 2 and d["kname"] == KNAME and d["elem"] == ELEM[compute], d

    def peeled(d, compute, vec, split):
        assert d.get("peel_launches", 0) >= 2 and d["family"] == 2 and d["kname"] == KNAME and d["elem"] == ELEM[compute], d
    _exact(env, "c32x_lone_A", xc.LONE, ("kji", "lk", "li"), compute, alpha=-2 + 1j, beta=1.0, check=lone)
    _exact(env, "c32x_peeled", xc.PEEL, ("paqbrcsdte", "xpyqzrst", "abxcydze"), compute, alpha=0.5 - 1j, beta=1j, check=peeled)


# ---- 2. the lo planes of the TF32 split -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("roles", ("A_wide", "B_wide"))
@pytest.mark.parametrize("lay", (0, 3))
def test_exact_lo_planes_of_the_tf32_split(env, force, roles, lay):
    """One operand's parts are integers in [-4095, 4095]: hi + lo is exact (12 bits = 8 + a remainder of at most 4 significant bits) and
    lo != 0 for most of the draw; the other's are in {+-1, +-2, +-3}; K = 600: a component's sum of |products| is at most
    2 * 600 * 4095 * 3 = 1.47e7 < 2^24.  Exact under TF32 only if all four lo images are staged and multiplied."""
    ct, ops, h, torch = env
    mA, mB = LAYOUTS[lay]
    ext, modes = dict(m=200, n=136, k=600), (mA, mB, "mn")
    rng = np.random.default_rng([4095, lay, roles == "A_wide"])
    shape = lambda m: [ext[c] for c in m]   # noqa: E731
    wide = lambda sh: rng.integers(-4095, 4096, size=sh)   # noqa: E731
    small = lambda sh: np.array([-3, -2, -1, 1, 2, 3])[rng.integers(0, 6, size=sh)]   # noqa: E731
    draw = lambda f, sh: (f(sh), f(sh))   # noqa: E731  (real, imaginary) int64 planes
    pa = draw(wide if roles == "A_wide" else small, shape(mA))
    pb = draw(small if roles == "A_wide" else wide, shape(mB))
    A = torch.complex(torch.from_numpy(pa[0]).float(), torch.from_numpy(pa[1]).float())
    B = torch.complex(torch.from_numpy(pb[0]).float(), torch.from_numpy(pb[1]).float())
    for w in ((A.real, A.imag) if roles == "A_wide" else (B.real, B.imag)):
        hi = w.to(torch.bfloat16).to(torch.float32)
        lo = w - hi
        assert bool((lo.to(torch.bfloat16).to(torch.float32) == lo).all()), "hi + lo is not exact on this draw"
        assert float((lo != 0).float().mean()) > 0.5
    # the bound from the draw: |a_r b_r - a_i b_i| and |a_r b_i + a_i b_r| are at most (|a_r| + |a_i|)(|b_r| + |b_i|) ... and at most
    # max(|a_r|, |a_i|)(|b_r| + |b_i|): the largest of that over m times the largest over n, summed over k
    am = torch.maximum(A.real.abs(), A.imag.abs()).amax(dim=mA.index("m")).double()
    bm = l1(B).amax(dim=mB.index("n"))
    if roles == "B_wide":
        am = l1(A).amax(dim=mA.index("m"))
        bm = torch.maximum(B.real.abs(), B.imag.abs()).amax(dim=mB.index("n")).double()
    assert float((am * bm).sum()) < 2.0 ** 24
    e = lambda x, y: np.einsum("%s,%s->mn" % (mA, mB), x, y)   # noqa: E731  int64
    want = torch.complex(torch.from_numpy((e(pa[0], pb[0]) - e(pa[1], pb[1])).astype(np.float64)),
                         torch.from_numpy((e(pa[0], pb[1]) + e(pa[1], pb[0])).astype(np.float64)))
    plan = make_plan(env, ext, modes, "TF32")
    try:
        on_c32x(plan.describe(), "TF32", vec=2)
        got, d = contract(env, plan, ext, modes, A, B, None)
        xd.assert_exact(got, want, "lo planes %s %s" % (roles, d))
    finally:
        plan.destroy()


# ---- 3. the meaning of 16BF / 16F -----------------------------------------------------------------------------------------------------
def _away_from_zero(torch, gen, shape):
    """+-U(2^-4, 1): away from fp16's subnormal range"""
    mag = torch.rand(shape, generator=gen, dtype=torch.float64) * (1.0 - 2.0 ** -4) + 2.0 ** -4
    sign = torch.randint(0, 2, shape, generator=gen, dtype=torch.int64) * 2 - 1
    return (mag * sign).to(torch.float32)


def _cplx(torch, f, gen, shape):
    return torch.complex(f(torch, gen, shape), f(torch, gen, shape))


ROUND = {"16BF": "bfloat16", "16F": "float16"}


@pytest.mark.parametrize("compute", ("16BF", "16F"))
@pytest.mark.parametrize("K", (8, 64, 256))
def test_products_are_those_of_the_rounded_parts(env, force, compute, K):
    """Each component of D equals the complex128 contraction of the operands with both parts rounded to the mode's 16-bit type within
    2K 2^-23 sum (|a^r|+|a^i|)(|b^r|+|b^i|): products of two 16-bit values are exact in fp32, each of the 2K accumulation steps of a
    component loses at most one fp32 ulp whatever the order.  A kernel that multiplies the unrounded parts is off by about 2^-9 (bf16) /
    2^-12 (fp16) per factor: orders of magnitude above the bound."""
    ct, ops, h, torch = env
    gen = torch.Generator().manual_seed(2000 + K)
    ext, modes = dict(m=192, n=160, k=K), ("km", "kn", "mn")
    A, B = _cplx(torch, _away_from_zero, gen, [K, 192]), _cplx(torch, _away_from_zero, gen, [K, 160])
    rt = getattr(torch, ROUND[compute])
    rounded = lambda z: torch.complex(z.real.to(rt).double(), z.imag.to(rt).double())   # noqa: E731
    ar, br = rounded(A), rounded(B)
    ref = torch.einsum("km,kn->mn", ar, br)
    tol = 2 * K * 2.0 ** -23 * torch.einsum("km,kn->mn", l1(ar), l1(br))
    plan = make_plan(env, ext, modes, compute)
    try:
        on_c32x(plan.describe(), compute, vec=2)
        got, d = contract(env, plan, ext, modes, A, B, None)
    finally:
        plan.destroy()
    err = comp_err(got, ref)
    unrounded = comp_err(torch.einsum("km,kn->mn", A.to(torch.complex128), B.to(torch.complex128)), ref)
    print("c32x meaning %s K=%d: worst err / bound %.3g (the unrounded complex64 product would be at %.3g)" % (
        compute, K, float((err / tol).max()), float((unrounded / tol).max())))
    assert bool((err <= tol).all()), (compute, K, float((err / tol).max()))


# ---- 4. accuracy against the true result ----------------------------------------------------------------------------------------------
def _uniform(torch, gen, shape):
    return (torch.rand(shape, generator=gen, dtype=torch.float64) * 2 - 1).to(torch.float32)


def _draw(torch, gen, compute, shape):
    return _cplx(torch, _away_from_zero if compute == "16F" else _uniform, gen, shape)


ACC_SHAPES = [
    ("k8", dict(m=192, n=160, k=8), ("km", "kn", "mn"), 1.0, 0.0),
    ("k64", dict(m=192, n=160, k=64), ("mk", "kn", "mn"), 1.0, 0.0),
    ("k1000", dict(m=200, n=136, k=1000), ("km", "nk", "mn"), -2 + 0.5j, 0.5 - 1j),
    ("k4096", dict(m=256, n=192, k=4096), ("mk", "nk", "mn"), 1.0, 0.0),
    ("k4096_big_tile", dict(m=1664, n=1600, k=4096), ("km", "kn", "mn"), 0.5j, 0.0),
    ("ref_50", dict(m=50, n=50, k=50), ("km", "kn", "mn"), 1.0, 0.0),                                      # the reference's extents of 50
    ("ref_mlik", dict(m=20, l=50, i=50, k=50, j=50), ("kilm", "mjkl", "jil"), 1.0, 1.0),                     # 'mlik,lkjm->lij': K = 1000
]


def _true_result(torch, eq, A, B, C, alpha, beta):
    """(reference, mag) in complex128 / fp64 on the device, from the host data"""
    a, b, c = A.cuda().to(torch.complex128), B.cuda().to(torch.complex128), C.to(torch.complex128)
    ref = alpha * torch.einsum(eq, a, b).cpu() + beta * c
    mag = l1(alpha) * torch.einsum(eq, l1(a), l1(b)).cpu() + l1(beta) * l1(c)
    return ref, mag


@pytest.mark.parametrize("compute", MODES)
@pytest.mark.parametrize("name,ext,modes,alpha,beta", ACC_SHAPES, ids=[s[0] for s in ACC_SHAPES])
def test_accuracy_against_the_true_result(env, force, compute, name, ext, modes, alpha, beta):
    ct, ops, h, torch = env
    gen = torch.Generator().manual_seed(77)
    sh = lambda m: [ext[c] for c in m]   # noqa: E731
    A, B, C = _draw(torch, gen, compute, sh(modes[0])), _draw(torch, gen, compute, sh(modes[1])), _draw(torch, gen, compute, sh(modes[2]))
    eq = "%s,%s->%s" % modes
    K = int(np.prod([ext[c] for c in modes[0] if c in modes[1] and c not in modes[2]]))
    ref, mag = _true_result(torch, eq, A, B, C, alpha, beta)
    plan = make_plan(env, ext, modes, compute)
    try:
        d = plan.describe()
        on_c32x(d, compute)
        if name == "k4096_big_tile":
            assert d["bm"] == 128, d
        got, d = contract(env, plan, ext, modes, A, B, C, alpha, beta)
    finally:
        plan.destroy()
    tol = bound_factor(compute, K) * mag
    err = comp_err(got, ref)
    print("c32x accuracy %s %s K=%d: worst err / mag %.3g, bound %.3g (ratio %.3g)" % (
        compute, name, K, float((err / mag).max()), bound_factor(compute, K), float((err / tol).max())))
    assert bool((err <= tol).all()), (compute, name, float((err / tol).max()), d)


# ---- 5. non-finite values -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compute", ("TF32", "16BF"))
def test_an_infinity_in_a_gives_infinity_in_its_row_only(env, force, compute):
    """+inf in the real part of one A element, B's parts in [0.1, 1]: re = inf * b_r - a_i b_i = +inf and im = inf * b_i + a_i b_r = +inf in
    that row of D; every other output is finite and within the bound"""
    ct, ops, h, torch = env
    gen = torch.Generator().manual_seed(5)
    ext, modes = dict(m=136, n=72, k=100), ("km", "kn", "mn")
    A = _cplx(torch, _uniform, gen, [100, 136])
    pos = lambda sh: (torch.rand(sh, generator=gen, dtype=torch.float64) * 0.9 + 0.1).to(torch.float32)   # noqa: E731
    B = torch.complex(pos([100, 72]), pos([100, 72]))
    A[17, 33] = complex(float("inf"), float(A[17, 33].imag))
    plan = make_plan(env, ext, modes, compute)
    try:
        on_c32x(plan.describe(), compute, vec=2)
        got, d = contract(env, plan, ext, modes, A, B, None)
    finally:
        plan.destroy()
    assert bool((got[33].real == float("inf")).all()) and bool((got[33].imag == float("inf")).all()), got[33]
    rows = [i for i in range(136) if i != 33]
    Af = A.clone()
    Af[17, 33] = 0.0
    a, b = Af.to(torch.complex128), B.to(torch.complex128)
    ref = torch.einsum("km,kn->mn", a, b)[rows]
    mag = torch.einsum("km,kn->mn", l1(a), l1(b))[rows]
    assert bool(torch.isfinite(got[rows].real).all()) and bool(torch.isfinite(got[rows].imag).all())
    assert bool((comp_err(got[rows], ref) <= bound_factor(compute, 100) * mag).all())


# ---- 6. the default planner -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compute", MODES)
def test_default_planner_meets_the_bound_of_the_mode_asked_for(env, compute):
    """no switch: whichever path the planner takes for 2048^3, 256 sampled rows are within the bound of the mode that was asked for (the
    complex64 path is at least as accurate)"""
    ct, ops, h, torch = env
    gen = torch.Generator().manual_seed(11)
    E = 2048
    ext, modes = dict(m=E, n=E, k=E), ("km", "kn", "mn")
    A, B = _draw(torch, gen, compute, [E, E]), _draw(torch, gen, compute, [E, E])
    a, b = A.cuda(), B.cuda()
    plan = make_plan(env, ext, modes, compute, ws_limit=None)
    try:
        d = plan.describe()
        assert d["family"] == 2 and ((d["kname"] == "gett_gen_kernel" and d["elem"] == 3) or (d["kname"] == KNAME and d["elem"] == ELEM[compute])), d
        out = torch.full((E, E), float("nan"), dtype=torch.complex64, device="cuda")        # D[m, n] with m fastest: out[n, m]
        ws = torch.empty(max(plan.required_workspace, 256), dtype=torch.uint8, device="cuda")
        before = ct.launch_counts()["gen"]
        plan.contract(1.0, a.data_ptr(), b.data_ptr(), 0.0, 0, out.data_ptr(), ws.data_ptr(), plan.required_workspace)
        torch.cuda.synchronize()
        assert ct.launch_counts()["gen"] > before, d
    finally:
        plan.destroy()
    rows = torch.arange(0, E, 8, device="cuda")                                                # 256 rows of n, every m
    # A[k, m] in mode order (k, m) means k FASTEST: the buffer is row-major [m][k]; likewise B is [n][k]
    am, bn = a.reshape(E, E).to(torch.complex128), b.reshape(E, E)[rows].to(torch.complex128)
    ref = bn @ am.t()
    mag = l1(bn) @ l1(am).t()
    err = comp_err(out[rows], ref)
    print("c32x default planner %s 2048^3: kernel %s elem %d, worst err / mag %.3g, bound %.3g" % (
        compute, d["kname"], d["elem"], float((err / mag).max()), bound_factor(compute, E)))
    assert bool((err <= bound_factor(compute, E) * mag).all()), d


def test_the_headline_einsum_retyped_to_complex64_keeps_its_plan_under_tf32(env):
    """'abcd,dcbe->ae' is split-K-dominated (one 96 x 96 output, K = 262144): a TF32 plan is the complex64 split-K plan"""
    plan = make_plan(env, xc.HEADLINE, xc.HEAD_MODES, "TF32", ws_limit=1 << 30)
    ref = make_plan(env, xc.HEADLINE, xc.HEAD_MODES, "32F", ws_limit=1 << 30)
    try:
        d, r = plan.describe(), ref.describe()
        assert d["family"] == 2 and d["kname"] == "gett_gen_kernel" and d["elem"] == 3 and d["splitK"] > 1 and d == r, (d, r)
    finally:
        plan.destroy()
        ref.destroy()


# ---- 7. front ends --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conj", ((False, False), (True, False), (False, True)), ids=("plain", "conj_a", "conj_b"))
def test_torch_einsum_with_tf32_on_complex64(env, force, conj):
    ct, ops, h, torch = env
    from cudalibrarysamples_amd import torch_einsum as te
    eq, sa, sb, K = "ik,kj->ij", (192, 256), (256, 160), 256
    gen = torch.Generator().manual_seed(3)
    a, b = _cplx(torch, _uniform, gen, sa), _cplx(torch, _uniform, gen, sb)
    key = (eq, tuple(sa), tuple(sb), torch.complex64, conj[0], conj[1], "TF32")
    te._plans.pop(key, None)                  # (a plan of an earlier test made without the switch)
    before = ct.launch_counts()["gen"]
    got = te.einsum(eq, a.cuda(), b.cuda(), conj_a=conj[0], conj_b=conj[1], compute="TF32")
    torch.cuda.synchronize()
    d = te._plans[key].describe()
    assert d["family"] == 2 and d["kname"] == KNAME and d["elem"] == 12 and ct.launch_counts()["gen"] > before, d
    a128, b128 = a.to(torch.complex128), b.to(torch.complex128)
    ref = torch.einsum(eq, a128.conj() if conj[0] else a128, b128.conj() if conj[1] else b128)
    mag = torch.einsum(eq, l1(a128), l1(b128))
    err = comp_err(got.cpu(), ref)
    print("c32x einsum TF32 %s: worst err / mag %.3g, bound %.3g" % (conj, float((err / mag).max()), bound_factor("TF32", K)))
    assert bool((err <= bound_factor("TF32", K) * mag).all())
    if conj[0] or conj[1]:      # the conjugation is not a no-op on this data
        plain = torch.einsum(eq, a128, b128)
        assert not bool((comp_err(got.cpu(), plain) <= bound_factor("TF32", K) * mag).all())
    te._plans.pop(key, None)


def test_compute_is_part_of_the_plan_key_and_other_types_still_refuse(env, monkeypatch):
    ct, ops, h, torch = env
    from cudalibrarysamples_amd import torch_einsum as te
    x = torch.ones(64, 64, dtype=torch.bfloat16, device="cuda")
    for bad in (x, x.to(torch.float16), x.to(torch.float64), x.to(torch.complex128)):
        with pytest.raises(ValueError):
            te.einsum("ik,kj->ij", bad, bad, compute="TF32")
    monkeypatch.setenv("CUTENSOR_AMD_F32X", "force")
    a = torch.full((128, 64), 1 + 1j, dtype=torch.complex64, device="cuda")
    b = torch.full((64, 96), 1 - 2j, dtype=torch.complex64, device="cuda")
    base = ("ik,kj->ij", (128, 64), (64, 96), torch.complex64, False, False)
    for k in (base, base + ("16BF",)):
        te._plans.pop(k, None)
    te.einsum("ik,kj->ij", a, b)
    out = te.einsum("ik,kj->ij", a, b, compute="16BF")
    d0 = te._plans[base].describe()
    assert d0["kname"] == "gett_gen_kernel" and d0["elem"] == 3, d0          # (the default plan keeps the key it always had)
    d = te._plans[base + ("16BF",)].describe()
    assert d["family"] == 2 and d["kname"] == KNAME and d["elem"] == 10, d
    assert te._plans[base] is not te._plans[base + ("16BF",)]
    assert bool((out == 64 * (1 + 1j) * (1 - 2j)).all())
    for k in (base, base + ("16BF",)):
        te._plans.pop(k, None)


def test_the_c_einsum_passes_the_descriptor_through_for_complex_float(env, force):
    """Einsum<std::complex<float>> (ctamdEinsumCreate with C_32F) + ctamdEinsumSetCompute: the plan is the forced element of each name"""
    ct, ops, h, torch = env
    from cudalibrarysamples_amd import torch_einsum as te
    for compute in MODES:
        p = te.EinsumPlan("ik,kj->ij", (256, 128), (128, 192), torch.complex64, compute=compute)
        d = p.describe()
        assert d["family"] == 2 and d["kname"] == KNAME and d["elem"] == ELEM[compute], (compute, d)
    d = te.EinsumPlan("ik,kj->ij", (256, 128), (128, 192), torch.complex64).describe()
    assert d["kname"] == "gett_gen_kernel" and d["elem"] == 3, d
