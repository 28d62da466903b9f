"""fp64 / complex128 contractions under COMPUTE_DESC_32F (csrc/kernels/gett_gen_f64x.inc) on the GPU.

The descriptor permits D = alpha * sum_k fp32(a_k) * fp32(b_k) + beta * op(C): every operand element (complex: both parts) rounded once
to fp32 on its way into LDS, products and sums on the fp32 MFMA, alpha / beta / C / D in fp64.  Every case but the default-planner one
runs with CUTENSOR_AMD_F64X=force, asserts the element of the plan's description (8: fp64 data, 9: complex128 data) and that the general
family's launch counter went up; D lives in a NaN-filled guarded buffer.

* rounding is visible: operands i + j 2^-30 with fp32(x) = i come back as the INTEGER contraction of the i, bit for bit — an fp64 kernel
  does not (checked on the CPU before the launch: its result differs on at least 99 % of the outputs);
* exact: integer data (tests/exact_data.py) comes back bit for bit.  The accumulators are fp32: the test asserts K * 9 (complex: K * 18)
  * max(1, |alpha|) + 3 |beta| < 2^24 itself (exact_data.acc_limit would allow 2^53 for these data types);
* accuracy against the fp64 result, worst case per output: (2.01 * 2^-24 + K * 2^-23) * mag for real data, mag = |alpha| sum |a||b| +
  |beta||c|; (2.01 * 2^-24 + 2 K * 2^-23) * mag per component for complex data, mag = |alpha| sum (|a_r| + |a_i|)(|b_r| + |b_i|) +
  |beta| (|c_r| + |c_i|): two roundings of relative 2^-24 per product, one fp32 ulp per accumulation step (a complex component sums 2 K
  products);
* an inf and an |x| = 1e39 operand element give +-inf, a NaN gives NaN, in exactly the outputs they feed.
Figures are printed before they are asserted (pytest -s)."""
import numpy as np
import pytest

import exact_cases as xc
import exact_data as xd

pytestmark = pytest.mark.gpu

KINDS = ("f64", "c128")
DTYPE = {"f64": "float64", "c128": "complex128"}
ELEM = {"f64": 8, "c128": 9}
ELEM64 = {"f64": 2, "c128": 4}
KNAME = "gett_gen_f64x_kernel"
LAYOUTS = xc.LAYOUTS
BIG = {"f64": (128, 128), "c128": (128, 64)}
SMALL = (64, 64)


def bound_factor(kind, K):
    return 2.01 * 2.0 ** -24 + (2 if kind == "c128" else 1) * K * 2.0 ** -23


@pytest.fixture(scope="module")
def env(built):
    import torch
    assert torch.cuda.is_available()
    from cudalibrarysamples_amd import cutensor as ct, ops
    return ct, ops, ops.Handle(), torch


@pytest.fixture
def force(monkeypatch):
    monkeypatch.setenv("CUTENSOR_AMD_F64X", "force")


def make_plan(env, kind, ext, modes, compute="32F", pad=(0, 0, 0), align=128, ws_limit=1 << 28, conj=(False, False, False)):
    import guarded as gd
    ct, ops, h, torch = env
    e = lambda m: [ext[c] for c in m]   # noqa: E731
    # pad: pitch padding of A, B, D — and of C, when a fourth entry gives C a pitch of its own
    st = [gd.packed_strides(e(modes[min(i, 2)]), pad[i]) for i in range(len(pad))]
    op = [ct.OP_CONJ if c else ct.OP_IDENTITY for c in conj]
    return ops.contraction_plan(h, e(modes[0]), modes[0], e(modes[1]), modes[1], e(modes[2]), modes[2], dtype=ct.R_64F if kind == "f64" else ct.C_64F,
                                strideA=st[0], strideB=st[1], strideC=st[-1], strideD=st[2] if len(pad) > 3 else None, alignment=align, compute=compute, workspace_limit=ws_limit,
                                opA=op[0], opB=op[1], opC=op[2])


def contract(env, kind, plan, ext, modes, A, B, C, alpha=1.0, beta=0.0, pad=(0, 0, 0), off=0, inplace=False):
    """A, B, C: logical host tensors (dimensions in the order of the mode strings).  D lives in a NaN-filled buffer; returns (D, description)"""
    ct, ops, h, torch = env
    d = plan.describe()
    dt = DTYPE[kind]
    e = lambda m: [ext[c] for c in m]   # noqa: E731
    pa, pb = xc.Placed(e(modes[0]), dt, pad[0], off), xc.Placed(e(modes[1]), dt, pad[1], off)
    pa.set(A)
    pb.set(B)
    pd = xc.Placed(e(modes[2]), dt, pad[2], off)
    pc = None
    if beta:
        pc = pd if inplace else xc.Placed(e(modes[2]), dt, pad[-1], off)
        pc.set(C)
    ws = torch.full((max(plan.required_workspace, 256),), 0xFF, dtype=torch.uint8, device="cuda")
    before = ct.launch_counts()["gen"]
    plan.contract(alpha, pa.ptr, pb.ptr, beta, pc.ptr if pc else 0, pd.ptr, ws.data_ptr(), plan.required_workspace)
    torch.cuda.synchronize()
    assert ct.launch_counts()["gen"] > before, d
    pd.check_outside(str(d))
    return pd.get(), d


def on_f64x(d, kind, vec=None, split=None, tile=None):
    assert d["family"] == 2 and d["kname"] == KNAME and d["elem"] == ELEM[kind], d
    if vec is not None:
        assert d["vec"] == (vec if kind == "f64" else 1), d      # complex128: one element is one 16-byte unit
    if split is not None:
        assert (d["splitK"] > 1) == split, d
    if tile is not None:
        assert (d["bm"], d["bn"]) == (BIG[kind] if tile == "big" else SMALL), d


def _K(ext, modes):
    return int(np.prod([ext[c] for c in modes[0] if c in modes[1] and c not in modes[2]]))


# ---- 1. the rounding is visible -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_operands_are_rounded_to_fp32(env, force, kind):
    """x = i + j 2^-30, i in {+-1, +-2, +-3}, j = +-1: fp32(x) = i exactly (|j 2^-30| is far below half an fp32 ulp of i).  The result is
    the integer contraction of the i, bit for bit; the fp64 contraction of the x themselves is not."""
    ct, ops, h, torch = env
    ext = dict(m=200, n=136, k=1000) if kind == "f64" else dict(m=136, n=72, k=520)
    modes = ("km", "kn", "mn")
    rng = np.random.default_rng([30, kind == "c128"])
    vals = np.array([-3, -2, -1, 1, 2, 3], dtype=np.int64)

    def draw(shape):
        i = vals[rng.integers(0, 6, size=shape)]
        j = rng.integers(0, 2, size=shape) * 2 - 1
        return i, i.astype(np.float64) + j.astype(np.float64) * 2.0 ** -30
    sA, sB = [ext[c] for c in modes[0]], [ext[c] for c in modes[1]]
    if kind == "f64":
        (ia, xa), (ib, xb) = draw(sA), draw(sB)
        want = np.einsum("km,kn->mn", ia, ib).astype(np.float64)
        A, B = torch.from_numpy(xa), torch.from_numpy(xb)
        assert bool((A.float().double() == torch.from_numpy(ia.astype(np.float64))).all())
    else:
        (iar, xar), (iai, xai), (ibr, xbr), (ibi, xbi) = draw(sA), draw(sA), draw(sB), draw(sB)
        e = lambda x, y: np.einsum("km,kn->mn", x, y)   # noqa: E731
        want = (e(iar, ibr) - e(iai, ibi)).astype(np.float64) + 1j * (e(iar, ibi) + e(iai, ibr)).astype(np.float64)
        A, B = torch.from_numpy(xar + 1j * xai), torch.from_numpy(xbr + 1j * xbi)
        assert bool((A.to(torch.complex64).to(torch.complex128) == torch.from_numpy(iar + 1j * iai)).all())
    want = torch.from_numpy(want)
    assert _K(ext, modes) * (18 if kind == "c128" else 9) < 2.0 ** 24
    # the draw proves something only if full fp64 products do NOT give the integer result
    full = torch.einsum("km,kn->mn", A, B)
    share = float((full != want).double().mean())
    print("f64x rounding %s: an fp64 contraction of the unrounded operands differs from the integer result on %.2f %% of the outputs" % (kind, 100 * share))
    assert share >= 0.99, share
    plan = make_plan(env, kind, ext, modes)
    try:
        on_f64x(plan.describe(), kind, vec=2)
        got, d = contract(env, kind, plan, ext, modes, A, B, None)
    finally:
        plan.destroy()
    xd.assert_exact(got, want, "rounding %s %s" % (kind, d))


# ---- 2. exact, zero tolerance ---------------------------------------------------------------------------------------------------------
def _exact(env, cid, kind, ext, modes, vec=None, split=None, tile=None, alpha=1.0, beta=0.0, pad=(0, 0, 0), off=0, align=128, inplace=False,
           conj=(False, False, False), check=on_f64x):
    ct, ops, h, torch = env
    if kind == "f64":
        conj = (False, False, False)
    case = xc.Case(cid + "_" + kind, DTYPE[kind], ext, modes, alpha=alpha, beta=beta, pad=pad, off=off, align=align, conj=conj)
    # fp32 accumulators: every product is at most 9 (complex: a component sums two products per k), C is at most 3 in each part
    K = _K(ext, modes)
    assert K * (18 if kind == "c128" else 9) * max(1.0, abs(alpha)) + 3 * abs(beta) < 2.0 ** 24, (cid, K)
    plan = make_plan(env, kind, ext, modes, "32F", pad, align, conj=conj)
    try:
        d = plan.describe()
        check(d, kind, vec, split, tile)
        for swap in (False, True):
            A, B, C = xd.make_exact(case, swap)
            xd.check_draw(case, A, B, C, swap)
            want, _ = xd.expected(case, xd.exact_reference(case, A, B, C, device="cuda"))
            got, _ = contract(env, kind, plan, ext, modes, A, B, C, alpha, beta, pad, off, inplace)
            xd.assert_exact(got, want, "%s %s draw %d %s" % (cid, kind, int(swap), d))
    finally:
        plan.destroy()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("lay", range(4))
def test_exact_layouts_tiles_and_widths(env, force, kind, lay):
    mA, mB = LAYOUTS[lay]
    L = xc.LNAME[(mA, mB)]
    s = xc.SCALARS32
    cj = ((lay & 1) == 1, (lay & 2) == 2, lay == 3)
    # the large tile (169 / 325 output tiles fill the chip) and the 64 x 64 one, 16-byte loads
    _exact(env, "f64x_big_%s" % L, kind, dict(m=1664, n=1600, k=200), (mA, mB, "mn"), vec=2, tile="big", alpha=s[lay][0], beta=s[lay][1], conj=cj)
    _exact(env, "f64x_small_%s" % L, kind, dict(m=200, n=136, k=1000), (mA, mB, "mn"), vec=2, tile="small", alpha=s[lay + 1][0], beta=s[lay + 1][1], conj=cj)
    # 8-byte gathers: odd extents; an odd element offset at element alignment (the large tile)
    _exact(env, "f64x_odd_%s" % L, kind, dict(m=67, n=45, k=333), (mA, mB, "mn"), vec=1, tile="small", alpha=s[lay + 2][0], beta=s[lay + 2][1], conj=cj)
    _exact(env, "f64x_big_off_%s" % L, kind, dict(m=1664, n=1600, k=72), (mA, mB, "mn"), vec=1, tile="big", off=3, align=8 if kind == "f64" else 16)


@pytest.mark.parametrize("kind", KINDS)
def test_exact_groups_pitches_split_k_and_in_place(env, force, kind):
    s = xc.SCALARS32
    al = 8 if kind == "f64" else 16
    # two contracted modes, the fastest one ragged against the K-tile: with 16-byte loads of fp64 pairs (36) and without (37)
    _exact(env, "f64x_two_k_36", kind, dict(m=136, n=136, k=36, j=25), ("kmj", "kjn", "mn"), vec=2, alpha=s[1][0], beta=s[1][1])
    _exact(env, "f64x_two_k_37", kind, dict(m=136, n=72, k=37, j=25), ("kmj", "kjn", "mn"), vec=1, alpha=s[2][0], beta=s[2][1], conj=(True, False, True))
    # a batch mode
    _exact(env, "f64x_batch", kind, dict(m=132, n=68, k=64, l=3), ("mkl", "knl", "mnl"), vec=2, alpha=0.5, beta=1.0)
    _exact(env, "f64x_batch_kfirst", kind, dict(m=132, n=68, k=64, l=3), ("kml", "nkl", "mnl"), vec=2, alpha=-2.0, beta=0.0, conj=(False, True, False))
    # padded pitches: 16-byte loads kept at a 16-byte-aligned offset, lost at an odd one
    _exact(env, "f64x_pitch4", kind, dict(m=264, n=136, k=128), ("mk", "kn", "mn"), vec=2, pad=(4, 8, 4), off=4, align=16, alpha=1.0, beta=-0.5)
    _exact(env, "f64x_pitch_odd", kind, dict(m=262, n=134, k=134), ("km", "kn", "mn"), vec=1, pad=(5, 3, 1), off=3, align=al, alpha=0.5, beta=1.0)
    # split-K: fp32 / float2 partials folded in fp64; in place (C = D)
    _exact(env, "f64x_splitk", kind, dict(m=128, n=128, k=65536), ("km", "kn", "mn"), vec=2, split=True, alpha=-2.0, beta=1.0, conj=(True, True, True))
    _exact(env, "f64x_splitk_odd", kind, dict(m=100, n=60, k=4099), ("mk", "kn", "mn"), vec=1, split=True, alpha=0.5, beta=-0.5, inplace=True)


@pytest.mark.parametrize("kind", KINDS)
def test_exact_row_and_column_groups_that_do_not_fuse(env, force, kind):
    """M and N of two modes each, interleaved in D: the mixed-radix row clamp and epilogue offsets, in ONE launch (xc.UNFUSED).  The family
    has no switch that forces split-K: a second case with k = 517 splits by itself."""
    def unfused(d, kind, vec, split, tile):
        on_f64x(d, kind, vec, split, tile)
        xc.one_launch(d)
    _exact(env, "f64x_unfused", kind, xc.UNFUSED, xc.UNFUSED_MODES, vec=1, tile="small", alpha=-2.0, beta=0.5, pad=xc.UNFUSED_PAD, conj=(False, True, True),
           check=unfused)
    # the same groups with a K long enough to split by itself: the partial walk and the fold on groups that do not fuse
    _exact(env, "f64x_unfused_splitk", kind, xc.UNFUSED_LONG, xc.UNFUSED_MODES, vec=1, split=True, tile="small", alpha=-2.0, beta=0.5, pad=xc.UNFUSED_PAD,
           conj=(False, True, True))


@pytest.mark.parametrize("kind", KINDS)
def test_exact_scalars_in_place_and_conjugation(env, force, kind):
    scalars = list(xc.SCALARS32)
    if kind == "c128":
        scalars += [(1.0 - 2.0j, 0.5j), (-2.0j, 1.0 + 1.0j)]
    for i, (al, be) in enumerate(scalars):
        cj = (bool(i & 1), bool(i & 2), bool(i & 4) or i == 1)
        _exact(env, "f64x_scalars_%d" % i, kind, dict(m=200, n=136, k=104), ("km", "nk", "mn"), vec=2, alpha=al, beta=be, inplace=bool(i & 1), conj=cj)


# ---- 3. accuracy against the fp64 result ----------------------------------------------------------------------------------------------
def _uniform(torch, gen, kind, shape):
    u = lambda: torch.rand(shape, generator=gen, dtype=torch.float64) * 2 - 1   # noqa: E731
    return u() if kind == "f64" else torch.complex(u(), u())


def _mag(x):
    return (x.real.abs() + x.imag.abs()) if x.is_complex() else x.abs()


def _err(got, ref):
    d = got - ref
    return torch_max(d.real.abs(), d.imag.abs()) if d.is_complex() else d.abs()


def torch_max(a, b):
    import torch
    return torch.maximum(a, b)


ACC_SHAPES = [
    ("k8", dict(m=192, n=160, k=8), ("km", "kn", "mn"), 1.0, 0.0),
    ("k64", dict(m=192, n=160, k=64), ("mk", "kn", "mn"), -2.0, 0.5),
    ("k4096", dict(m=256, n=192, k=4096), ("mk", "nk", "mn"), 1.0, 0.0),
]


def _check_accuracy(env, kind, name, ext, modes, alpha, beta, plan, expect):
    ct, ops, h, torch = env
    gen = torch.Generator().manual_seed(77)
    sh = lambda m: [ext[c] for c in m]   # noqa: E731
    A, B, C = (_uniform(torch, gen, kind, sh(modes[i])) for i in range(3))
    eq = "%s,%s->%s" % modes
    K = _K(ext, modes)
    ref = alpha * torch.einsum(eq, A.cuda(), B.cuda()).cpu() + beta * C
    mag = abs(alpha) * torch.einsum(eq, _mag(A).cuda(), _mag(B).cuda()).cpu() + abs(beta) * _mag(C)
    d = plan.describe()
    expect(d)
    got, d = contract(env, kind, plan, ext, modes, A, B, C, alpha, beta)
    if d["kname"] == KNAME:
        factor = bound_factor(kind, K)
    else:
        # the fp64 kernels against an fp64 reference: one fp64 ulp per accumulation step and one rounding per product, on either side
        factor = 2 * (2.0 ** -53 + (2 if kind == "c128" else 1) * K * 2.0 ** -52)
    err = _err(got, ref)
    print("f64x accuracy %s %s K=%d %s: worst err / mag %.3g, bound %.3g (ratio %.3g)" % (
        kind, name, K, d["kname"], float((err / mag).max()), factor, float((err / (factor * mag)).max())))
    assert bool((err <= factor * mag).all()), (kind, name, float((err / (factor * mag)).max()), d)
    return float((err / mag).max())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,ext,modes,alpha,beta", ACC_SHAPES, ids=[s[0] for s in ACC_SHAPES])
def test_accuracy_against_the_fp64_result(env, force, kind, name, ext, modes, alpha, beta):
    plan = make_plan(env, kind, ext, modes)
    try:
        worst = _check_accuracy(env, kind, name, ext, modes, alpha, beta, plan, lambda d: on_f64x(d, kind))
    finally:
        plan.destroy()
    # ... and the operands WERE rounded: an fp64 kernel would be below 2^-40 here
    assert worst > 2.0 ** -40, worst


# ---- 4. non-finite values -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_inf_overflow_and_nan_reach_exactly_the_outputs_they_feed(env, force, kind):
    """A[k = 17, m = 33] = inf, A[k = 5, m = 70] = -1e39 (beyond fp32: rounds to -inf), A[k = 9, m = 100] = NaN; B positive integers.  Rows
    33 / 70 / 100 of D are +inf / -inf / NaN in every column (complex data, the value in A's real / imaginary / real part: (+inf, +inf),
    (+inf, -inf) — Re = rr - ii with ii = -inf — and (NaN, NaN)); every other output is the exact integer result."""
    ct, ops, h, torch = env
    ext, modes = dict(m=136, n=72, k=100), ("km", "kn", "mn")
    rng = np.random.default_rng([7, kind == "c128"])
    vals = np.array([-3, -2, -1, 1, 2, 3], dtype=np.int64)
    ia = [vals[rng.integers(0, 6, size=(136, 100))] for _ in range(2)]          # [m][k] logical order (k, m): transposed below
    ib = [rng.integers(1, 4, size=(72, 100)) for _ in range(2)]
    e = lambda x, y: np.einsum("mk,nk->mn", x, y).astype(np.float64)   # noqa: E731
    if kind == "f64":
        want = torch.from_numpy(e(ia[0], ib[0]))
        A = torch.from_numpy(ia[0].astype(np.float64).T.copy())                 # dimensions (k, m)
        B = torch.from_numpy(ib[0].astype(np.float64).T.copy())
        A[17, 33], A[5, 70], A[9, 100] = float("inf"), -1e39, float("nan")
        special = {33: float("inf"), 70: float("-inf")}
    else:
        want = torch.from_numpy(e(ia[0], ib[0]) - e(ia[1], ib[1]) + 1j * (e(ia[0], ib[1]) + e(ia[1], ib[0])))
        A = torch.from_numpy((ia[0] + 1j * ia[1]).T.copy())
        B = torch.from_numpy((ib[0] + 1j * ib[1]).T.copy())
        A[17, 33] = complex(float("inf"), float(ia[1][33, 17]))
        A[5, 70] = complex(float(ia[0][70, 5]), -1e39)
        A[9, 100] = complex(float("nan"), float(ia[1][100, 9]))
        special = {33: complex(float("inf"), float("inf")), 70: complex(float("inf"), float("-inf"))}
    plan = make_plan(env, kind, ext, modes)
    try:
        on_f64x(plan.describe(), kind, vec=2)
        got, d = contract(env, kind, plan, ext, modes, A, B, None)
    finally:
        plan.destroy()
    for row, v in special.items():
        assert bool((got[row] == v).all()), (row, got[row][:4])
    nan_row = torch.view_as_real(got[100]) if kind == "c128" else got[100]
    assert bool(torch.isnan(nan_row).all()), got[100][:4]
    rows = [i for i in range(136) if i not in (33, 70, 100)]
    xd.assert_exact(got[rows], want[rows], "non-finite %s: the other rows %s" % (kind, d))


# ---- 5. the default planner -----------------------------------------------------------------------------------------------------------
def test_default_planner_meets_the_bound_of_the_path_it_takes(env):
    """no switch, a bench-class shape (2048 x 2048 x 512, fp64): the plan is either the single-precision one or today's fp64 plan, and the
    result is within the bound of the path the description names"""
    kind, ext, modes = "f64", dict(m=2048, n=2048, k=512), ("mk", "kn", "mn")

    def expect(d):
        assert d["family"] == 2 and ((d["kname"] == KNAME and d["elem"] == 8) or (d["kname"] == "gett_gen_kernel" and d["elem"] == 2)), d
    plan = make_plan(env, kind, ext, modes, ws_limit=None)
    try:
        _check_accuracy(env, kind, "default_2048x2048x512", ext, modes, 1.0, 0.0, plan, expect)
    finally:
        plan.destroy()


# ---- 6. torch_einsum ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_torch_einsum_selects_the_descriptor(env, force, kind):
    ct, ops, h, torch = env
    from cudalibrarysamples_amd import torch_einsum as te
    gen = torch.Generator().manual_seed(3)
    a, b = _uniform(torch, gen, kind, [136, 104]).cuda(), _uniform(torch, gen, kind, [104, 72]).cuda()
    ref = torch.einsum("ik,kj->ij", a, b)
    mag = torch.einsum("ik,kj->ij", _mag(a), _mag(b))
    before = ct.launch_counts()["gen"]
    got = te.einsum("ik,kj->ij", a, b, compute="32F")
    full = te.einsum("ik,kj->ij", a, b)
    torch.cuda.synchronize()
    assert ct.launch_counts()["gen"] >= before + 2
    base = ("ik,kj->ij", (136, 104), (104, 72), a.dtype, False, False)
    d32, d64 = te._plans[base + ("32F",)].describe(), te._plans[base].describe()
    assert d32["kname"] == KNAME and d32["elem"] == ELEM[kind], d32
    assert d64["kname"] == "gett_gen_kernel" and d64["elem"] == ELEM64[kind], d64
    e32, e64 = _err(got, ref), _err(full, ref)
    print("f64x torch_einsum %s: worst err / mag 32F %.3g, default %.3g" % (kind, float((e32 / mag).max()), float((e64 / mag).max())))
    assert bool((e32 <= bound_factor(kind, 104) * mag).all()) and float((e32 / mag).max()) > 2.0 ** -40
    assert float((e64 / mag).max()) < 2.0 ** -40


def test_torch_einsum_other_names_still_need_float32(env):
    ct, ops, h, torch = env
    from cudalibrarysamples_amd import torch_einsum as te
    a = torch.zeros(8, 8, dtype=torch.float64, device="cuda")
    for name in ("TF32", "16BF", "16F"):
        with pytest.raises(ValueError):
            te.einsum("ik,kj->ij", a, a, compute=name)
    # "32F" on the other data types is the default it always was: the plan key does not grow
    x = torch.ones(8, 8, dtype=torch.float32, device="cuda")
    te.einsum("ik,kj->ij", x, x, compute="32F")
    assert ("ik,kj->ij", (8, 8), (8, 8), torch.float32, False, False) in te._plans
