"""Which fp32 contractions the planner hands to the reduced-precision kernels (csrc/kernels/gett_gen_f32x.inc), host-only.

COMPUTE_DESC_16F / _16BF / _TF32 on real fp32 data with fp32 scalars permit products of rounded operands at the 16-bit matrix rate; under
CUTENSOR_AMD_F32X=force the planner takes that path whenever the descriptor permits it, under =0 never, and without the switch by its
model (tests/test_gpu_f32x.py has the default-planner cases).  COMPUTE_DESC_32F / _3XTF32, complex and 16-bit data are untouched."""
import pytest

ELEM = {"16BF": 5, "16F": 6, "TF32": 7}
KNAME = "gett_gen_f32x_kernel"


@pytest.fixture(scope="module")
def env(built):
    from cudalibrarysamples_amd import cutensor as ct, ops
    return ct, ops, ops.Handle()


def gemm(env, M, N, K, mA, mB, compute, dtype=None, **kw):
    ct, ops, h = env
    extA = [M, K] if mA == "mk" else [K, M]
    extB = [K, N] if mB == "kn" else [N, K]
    kw.setdefault("workspace_limit", 1 << 28)
    return ops.contraction_plan(h, extA, mA, extB, mB, [M, N], "mn", dtype=ct.R_32F if dtype is None else dtype, compute=compute, **kw)


def described(plan):
    d = plan.describe()
    plan.destroy()
    return d


@pytest.mark.parametrize("compute", sorted(ELEM))
def test_forced_path_elements_widths_and_orientations(env, monkeypatch, compute):
    monkeypatch.setenv("CUTENSOR_AMD_F32X", "force")
    for (mA, mB, oa, ob) in (("mk", "kn", 0, 1), ("km", "nk", 1, 0), ("km", "kn", 1, 1), ("mk", "nk", 0, 0)):
        d = described(gemm(env, 2048, 2048, 2048, mA, mB, compute))
        # the planner may have swapped the operands (D's stride-1 mode becomes kernel-N): compare as a set when it did
        got = (d["orientA"], d["orientB"]) if not d["swapped"] else (d["orientB"], d["orientA"])
        assert d["family"] == 2 and d["kname"] == KNAME and d["elem"] == ELEM[compute] and d["vec"] == 4 and got == (oa, ob), (mA, mB, d)
        assert (d["bm"], d["bn"], d["bk"]) == (128, 128, 32 if compute == "TF32" else 64) and d["splitK"] == 1 and d["workspace"] == 0, d
    # odd extents / element alignment only: 4-byte gathers
    for args, kw in (((37, 29, 51, "mk", "kn"), {}), ((64, 64, 64, "km", "kn"), dict(alignment=4)), ((50, 50, 50, "km", "kn"), {})):
        d = described(gemm(env, *args, compute, **kw))
        assert d["family"] == 2 and d["kname"] == KNAME and d["elem"] == ELEM[compute] and d["vec"] == 1 and (d["bm"], d["bk"]) == (64, 32), d


def test_full_precision_descriptors_and_other_data_types_are_untouched(env, monkeypatch):
    ct, ops, h = env
    monkeypatch.setenv("CUTENSOR_AMD_F32X", "force")
    for compute in ("32F", "3XTF32"):
        d = described(gemm(env, 2048, 2048, 2048, "km", "kn", compute))
        assert d["family"] == 0 and d["kname"] in ("gett_f32_stream_kernel", "gett_f32_kernel"), d
    base = described(gemm(env, 2048, 2048, 2048, "km", "kn", "32F"))
    monkeypatch.delenv("CUTENSOR_AMD_F32X")
    assert described(gemm(env, 2048, 2048, 2048, "km", "kn", "32F")) == base
    monkeypatch.setenv("CUTENSOR_AMD_F32X", "force")
    # fp64 accumulation of fp32 data, complex64 under 3XTF32, 16-bit data under its own descriptor
    assert described(gemm(env, 512, 512, 512, "km", "kn", "64F"))["family"] == 0
    d = described(gemm(env, 512, 512, 512, "km", "kn", "3XTF32", dtype=ct.C_32F))
    assert d["family"] == 2 and d["kname"] == "gett_gen_kernel" and d["elem"] == 3, d
    d = described(gemm(env, 2048, 2048, 1024, "mk", "kn", "16BF", dtype=ct.R_16BF))
    assert d["family"] == 1, d
    # a caller who names a candidate addresses the fp32 list, as ever
    d = described(gemm(env, 2048, 2048, 2048, "km", "kn", "TF32", kernel_rank=1))
    assert d["family"] == 0, d
    d = described(gemm(env, 2048, 2048, 2048, "km", "kn", "TF32", algo=0))
    assert d["family"] == 0, d


@pytest.mark.parametrize("compute", sorted(ELEM))
def test_switched_off_every_mode_is_the_fp32_plan(env, monkeypatch, compute):
    monkeypatch.setenv("CUTENSOR_AMD_F32X", "0")
    want = described(gemm(env, 2048, 2048, 2048, "km", "kn", "32F"))
    d = described(gemm(env, 2048, 2048, 2048, "km", "kn", compute))
    assert d["family"] == 0 and d == want, d
    assert described(gemm(env, 37, 29, 51, "mk", "kn", compute))["family"] == 0


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
        assert p.describe()["family"] == 2 and p.required_workspace == 0, p.describe()
        p.destroy()
    # one output tile row, deep K: split over the chip, fp32 partials [slice][L][M][N]
    p = gemm(env, 128, 128, 65536, "km", "kn", compute)
    d = p.describe()
    assert d["splitK"] > 1 and d["workspace"] == d["splitK"] * 128 * 128 * 4 == p.required_workspace, d
    p.destroy()


def test_plans_of_different_compute_modes_do_not_answer_each_other(env, monkeypatch):
    """the plan memo holds the compute descriptor in its key (and stands aside while the switch is set): 32F then TF32 then 32F"""
    ct, ops, h = env
    h2 = ops.Handle()
    def mk(compute):
        return ops.contraction_plan(h2, [1024, 512], "km", [1024, 768], "kn", [512, 768], "mn", dtype=ct.R_32F, compute=compute, workspace_limit=1 << 28)
    a = described(mk("32F"))
    monkeypatch.setenv("CUTENSOR_AMD_F32X", "force")
    b = described(mk("TF32"))
    c = described(mk("16BF"))
    monkeypatch.delenv("CUTENSOR_AMD_F32X")
    a2 = described(mk("32F"))
    assert a["family"] == 0 and a2 == a and b["family"] == 2 and b["elem"] == 7 and c["elem"] == 5 and b != a, (a, b, c)
    # without the switch the memo is live: the same sequence again answers each descriptor with its own plan
    first = [described(mk(x)) for x in ("32F", "TF32", "16BF", "16F")]
    again = [described(mk(x)) for x in ("32F", "TF32", "16BF", "16F")]
    assert first == again and first[0] == a, (first, again)
    for x, d in zip(("TF32", "16BF", "16F"), first[1:]):
        assert d["family"] == 0 or d["elem"] == ELEM[x], (x, d)


@pytest.mark.parametrize("compute", sorted(ELEM))
def test_lone_modes_and_peeled_plans_pick_the_path_up(env, monkeypatch, compute):
    ct, ops, h = env
    import workspace_cases as wc
    monkeypatch.setenv("CUTENSOR_AMD_F32X", "force")
    e = wc.LONE
    p = ops.contraction_plan(h, [e[c] for c in "kji"], "kji", [e[c] for c in "lk"], "lk", [e[c] for c in "li"], "li", dtype=ct.R_32F, compute=compute,
                             workspace_limit=1 << 28)
    d = described(p)
    assert d.get("lone_reduce_A") == 1 and d["family"] == 2 and d["elem"] == ELEM[compute], d
    e = wc.PEEL
    mA, mB, mC = "paqbrcsdte", "xpyqzrst", "abxcydze"
    p = ops.contraction_plan(h, [e[c] for c in mA], mA, [e[c] for c in mB], mB, [e[c] for c in mC], mC, dtype=ct.R_32F, compute=compute, workspace_limit=1 << 24)
    d = described(p)
    assert d.get("peel_launches", 0) >= 2 and d["family"] == 2 and d["elem"] == ELEM[compute], d


def test_default_planner_keeps_what_its_model_cannot_place(env):
    """no switch: element gathers, split-K problems (the headline einsum) and problems smaller than the chip stay on the fp32 kernels,
    described exactly as under COMPUTE_DESC_32F"""
    ct, ops, h = env
    import exact_cases as xc
    e, (mA, mB, mC) = xc.HEADLINE, xc.HEAD_MODES
    def head(compute):
        return described(ops.contraction_plan(h, [e[c] for c in mA], mA, [e[c] for c in mB], mB, [e[c] for c in mC], mC, dtype=ct.R_32F, compute=compute,
                                              workspace_limit=1 << 30))
    want = head("32F")
    assert want["family"] == 0 and want["splitK"] == 256
    for compute in sorted(ELEM):
        assert head(compute) == want
        for args in ((37, 29, 51, "mk", "kn"), (128, 128, 65536, "km", "kn"), (256, 256, 256, "km", "kn")):
            assert described(gemm(env, *args, compute)) == described(gemm(env, *args, "32F")), (compute, args)
