"""Which complex64 contractions the planner hands to the reduced-precision kernels (csrc/kernels/gett_gen_c32x.inc), host-only.

COMPUTE_DESC_16F / _16BF / _TF32 on complex64 data with complex-float scalars permit the four real products of a complex product to be
formed from rounded parts at the 16-bit matrix rate; under CUTENSOR_AMD_F32X=force the planner takes that path whenever the descriptor
permits it, under =0 never, and without the switch by its model (tests/test_gpu_c32x.py has the default-planner cases).
COMPUTE_DESC_32F / _3XTF32 / _64F on complex64, complex128 and real fp32 data are untouched."""
import pytest

ELEM = {"16BF": 10, "16F": 11, "TF32": 12}
ELEM_REAL = {"16BF": 5, "16F": 6, "TF32": 7}
KNAME = "gett_gen_c32x_kernel"


@pytest.fixture(scope="module")
def env(built):
    from cudalibrarysamples_amd import cutensor as ct, ops
    return ct, ops, ops.Handle()


def gemm(env, M, N, K, mA, mB, compute, dtype=None, **kw):
    ct, ops, h = env
    extA = [M, K] if mA == "mk" else [K, M]
    extB = [K, N] if mB == "kn" else [N, K]
    kw.setdefault("workspace_limit", 1 << 28)
    return ops.contraction_plan(h, extA, mA, extB, mB, [M, N], "mn", dtype=ct.C_32F if dtype is None else dtype, compute=compute, **kw)


def described(plan):
    d = plan.describe()
    plan.destroy()
    return d


def on_c32(d):
    return d["family"] == 2 and d["kname"] == "gett_gen_kernel" and d["elem"] == 3


@pytest.mark.parametrize("compute", sorted(ELEM))
def test_forced_path_elements_widths_and_orientations(env, monkeypatch, compute):
    monkeypatch.setenv("CUTENSOR_AMD_F32X", "force")
    for (mA, mB, oa, ob) in (("mk", "kn", 0, 1), ("km", "nk", 1, 0), ("km", "kn", 1, 1), ("mk", "nk", 0, 0)):
        d = described(gemm(env, 2048, 2048, 2048, mA, mB, compute))
        # the planner may have swapped the operands (D's stride-1 mode becomes kernel-N): compare as a set when it did
        got = (d["orientA"], d["orientB"]) if not d["swapped"] else (d["orientB"], d["orientA"])
        assert d["family"] == 2 and d["kname"] == KNAME and d["elem"] == ELEM[compute] and d["vec"] == 2 and got == (oa, ob), (mA, mB, d)
        assert (d["bm"], d["bn"], d["bk"]) == (128, 128, 32) and d["splitK"] == 1 and d["workspace"] == 0, d
    # odd extents / element alignment only: 8-byte gathers on the small tile
    for args, kw in (((37, 29, 51, "mk", "kn"), {}), ((64, 64, 64, "km", "kn"), dict(alignment=8)), ((51, 51, 51, "km", "kn"), {})):
        d = described(gemm(env, *args, compute, **kw))
        assert d["family"] == 2 and d["kname"] == KNAME and d["elem"] == ELEM[compute] and d["vec"] == 1 and (d["bm"], d["bn"], d["bk"]) == (64, 64, 32), d
    # the reference's extents of 50: the small tile; 50 is even, so two complex64 are one 16-byte unit here as they are for the complex64
    # kernel (on real fp32 data 50 % 4 != 0 makes the same shape a gather)
    d = described(gemm(env, 50, 50, 50, "km", "kn", compute))
    assert d["family"] == 2 and d["kname"] == KNAME and d["elem"] == ELEM[compute] and (d["bm"], d["bn"], d["bk"]) == (64, 64, 32), d
    assert d["vec"] == 2 == described(gemm(env, 50, 50, 50, "km", "kn", "32F"))["vec"], d


def test_full_precision_descriptors_and_other_data_types_are_untouched(env, monkeypatch):
    ct, ops, h = env
    shape = (2048, 2048, 2048, "km", "kn")
    base = {c: described(gemm(env, *shape, c)) for c in ("32F", "3XTF32", "64F")}
    base128 = {c: described(gemm(env, 1024, 1024, 1024, "km", "kn", c, dtype=ct.C_64F)) for c in ("32F", "64F")}
    base32 = {c: described(gemm(env, *shape, c, dtype=ct.R_32F)) for c in ("32F", "TF32", "16BF", "16F")}
    assert on_c32(base["32F"]) and on_c32(base["3XTF32"]), base
    monkeypatch.setenv("CUTENSOR_AMD_F32X", "force")
    for c in ("32F", "3XTF32", "64F"):
        assert described(gemm(env, *shape, c)) == base[c], c
    # complex128 under its two descriptors, described as before; real fp32 data takes ITS reduced-precision kernels under the switch
    for c in ("32F", "64F"):
        assert described(gemm(env, 1024, 1024, 1024, "km", "kn", c, dtype=ct.C_64F)) == base128[c], c
    assert described(gemm(env, *shape, "32F", dtype=ct.R_32F)) == base32["32F"]
    for c in ("TF32", "16BF", "16F"):
        d = described(gemm(env, *shape, c, dtype=ct.R_32F))
        assert d["family"] == 2 and d["kname"] == "gett_gen_f32x_kernel" and d["elem"] == ELEM_REAL[c] and d["vec"] == 4, d
    # a caller who names a candidate gets the complex64 plan, as ever
    for kw in (dict(kernel_rank=1), dict(algo=0)):
        d = described(gemm(env, *shape, "TF32", **kw))
        assert on_c32(d), (kw, d)


@pytest.mark.parametrize("compute", sorted(ELEM))
def test_switched_off_every_mode_is_the_complex64_plan(env, monkeypatch, compute):
    monkeypatch.setenv("CUTENSOR_AMD_F32X", "0")
    for args in ((2048, 2048, 2048, "km", "kn"), (37, 29, 51, "mk", "kn"), (128, 128, 65536, "km", "kn")):
        want = described(gemm(env, *args, "32F"))
        d = described(gemm(env, *args, compute))
        assert on_c32(d) and d == want, (args, d, want)


@pytest.mark.parametrize("compute", sorted(ELEM))
def test_workspace_contract(env, monkeypatch, compute):
    ct, ops, h = env
    monkeypatch.setenv("CUTENSOR_AMD_F32X", "force")
    shapes = [(2048, 2048, 2048, "km", "kn"), (128, 128, 65536, "km", "kn"), (100, 60, 4099, "mk", "kn")]
    for (M, N, K, mA, mB) in shapes:
        for pref in (ct.WORKSPACE_DEFAULT, ct.WORKSPACE_MAX):
            p = gemm(env, M, N, K, mA, mB, compute, workspace_limit=None, workspace_pref=pref)
            d = p.describe()
            assert d["family"] == 2 and d["elem"] == ELEM[compute] and p.required_workspace <= p.workspace_estimate, (d, p.workspace_estimate)
            p.destroy()
        p = gemm(env, M, N, K, mA, mB, compute, workspace_limit=0)
        d = p.describe()
        assert d["family"] == 2 and d["elem"] == ELEM[compute] and d["splitK"] == 1 and p.required_workspace == 0, d
        p.destroy()
        p = gemm(env, M, N, K, mA, mB, compute, workspace_limit=None, workspace_pref=ct.WORKSPACE_MIN)
        d = p.describe()
        assert d["family"] == 2 and d["elem"] == ELEM[compute] and d["splitK"] == 1 and p.required_workspace == 0, d
        p.destroy()
    # one output tile row, deep K: split over the chip, float2 partials [slice][L][M][N]
    p = gemm(env, 128, 128, 65536, "km", "kn", compute)
    d = p.describe()
    assert d["splitK"] > 1 and d["workspace"] == d["splitK"] * 128 * 128 * 8 == p.required_workspace, d
    p.destroy()


def test_plans_of_different_compute_modes_do_not_answer_each_other(env, monkeypatch):
    """the plan memo holds the compute descriptor in its key (and stands aside while the switch is set): 32F, TF32, 16BF, then 32F again"""
    ct, ops, h = env
    h2 = ops.Handle()

    def mk(compute):
        return ops.contraction_plan(h2, [1024, 512], "km", [1024, 768], "kn", [512, 768], "mn", dtype=ct.C_32F, compute=compute, workspace_limit=1 << 28)
    a = described(mk("32F"))
    monkeypatch.setenv("CUTENSOR_AMD_F32X", "force")
    b = described(mk("TF32"))
    c = described(mk("16BF"))
    monkeypatch.delenv("CUTENSOR_AMD_F32X")
    a2 = described(mk("32F"))
    assert on_c32(a) and a2 == a and b["kname"] == KNAME and b["elem"] == 12 and c["kname"] == KNAME and c["elem"] == 10, (a, b, c)
    # without the switch the memo is live: the same sequence again answers each descriptor with its own plan
    first = [described(mk(x)) for x in ("32F", "TF32", "16BF", "16F", "32F")]
    again = [described(mk(x)) for x in ("32F", "TF32", "16BF", "16F", "32F")]
    assert first == again and first[0] == a and first[4] == a, (first, again)
    for x, d in zip(("TF32", "16BF", "16F"), first[1:4]):
        assert on_c32(d) or (d["kname"] == KNAME and d["elem"] == ELEM[x]), (x, d)


@pytest.mark.parametrize("compute", sorted(ELEM))
def test_lone_modes_and_peeled_plans_pick_the_path_up(env, monkeypatch, compute):
    ct, ops, h = env
    import workspace_cases as wc
    monkeypatch.setenv("CUTENSOR_AMD_F32X", "force")
    e = wc.LONE
    p = ops.contraction_plan(h, [e[c] for c in "kji"], "kji", [e[c] for c in "lk"], "lk", [e[c] for c in "li"], "li", dtype=ct.C_32F, compute=compute,
                             workspace_limit=1 << 28)
    d = described(p)
    assert d.get("lone_reduce_A") == 1 and d["family"] == 2 and d["kname"] == KNAME and d["elem"] == ELEM[compute], d
    e = wc.PEEL
    mA, mB, mC = "paqbrcsdte", "xpyqzrst", "abxcydze"
    p = ops.contraction_plan(h, [e[c] for c in mA], mA, [e[c] for c in mB], mB, [e[c] for c in mC], mC, dtype=ct.C_32F, compute=compute, workspace_limit=1 << 24)
    d = described(p)
    assert d.get("peel_launches", 0) >= 2 and d["family"] == 2 and d["kname"] == KNAME and d["elem"] == ELEM[compute], d


def test_default_planner_keeps_what_its_model_cannot_place(env):
    """no switch: element gathers, split-K problems (the headline einsum retyped to complex64) and problems smaller than the chip stay on the
    complex64 kernels, described exactly as under COMPUTE_DESC_32F"""
    ct, ops, h = env
    import exact_cases as xc
    e, (mA, mB, mC) = xc.HEADLINE, xc.HEAD_MODES

    def head(compute):
        return described(ops.contraction_plan(h, [e[c] for c in mA], mA, [e[c] for c in mB], mB, [e[c] for c in mC], mC, dtype=ct.C_32F, compute=compute,
                                              workspace_limit=1 << 30))
    want = head("32F")
    assert on_c32(want) and want["splitK"] > 1, want
    for compute in sorted(ELEM):
        assert head(compute) == want
        for args in ((37, 29, 51, "mk", "kn"), (128, 128, 65536, "km", "kn"), (256, 256, 256, "km", "kn")):
            assert described(gemm(env, *args, compute)) == described(gemm(env, *args, "32F")), (compute, args)
