"""Which fp64 / complex128 contractions the planner hands to the single-precision-compute kernels (csrc/kernels/gett_gen_f64x.inc),
host-only.

COMPUTE_DESC_32F on a contraction whose tensors are all real fp64 (all complex128) with double (complex double) scalars permits products
of operands rounded once to fp32, on the fp32 MFMA.  Under CUTENSOR_AMD_F64X=force the planner takes that path whenever the descriptor
permits it, under =0 never, and without the switch by its model (f64x_decide, contraction_route.cpp).  COMPUTE_DESC_64F, the 16-bit / TF32 descriptors
on fp64 data, fp32 and complex64 data, and a caller who names a candidate are untouched."""
import pytest

ELEM = {"f64": 8, "c128": 9}
KNAME = "gett_gen_f64x_kernel"
LAYOUTS = (("mk", "kn", 0, 1), ("km", "nk", 1, 0), ("km", "kn", 1, 1), ("mk", "nk", 0, 0))


@pytest.fixture(scope="module")
def env(built):
    from cudalibrarysamples_amd import cutensor as ct, ops
    return ct, ops, ops.Handle()


def gemm(env, M, N, K, mA, mB, compute, kind="f64", handle=None, **kw):
    ct, ops, h = env
    extA = [M, K] if mA == "mk" else [K, M]
    extB = [K, N] if mB == "kn" else [N, K]
    kw.setdefault("workspace_limit", 1 << 28)
    dtype = kw.pop("dtype") if "dtype" in kw else (ct.R_64F if kind == "f64" else ct.C_64F)
    return ops.contraction_plan(handle or h, extA, mA, extB, mB, [M, N], "mn", dtype=dtype, compute=compute, **kw)


def described(plan):
    d = plan.describe()
    plan.destroy()
    return d


@pytest.mark.parametrize("kind", sorted(ELEM))
def test_forced_path_elements_widths_and_orientations(env, monkeypatch, kind):
    monkeypatch.setenv("CUTENSOR_AMD_F64X", "force")
    for (mA, mB, oa, ob) in LAYOUTS:
        d = described(gemm(env, 2048, 2048, 2048, mA, mB, "32F", kind))
        # the planner may have swapped the operands (D's stride-1 mode becomes kernel-N): compare as a set when it did
        got = (d["orientA"], d["orientB"]) if not d["swapped"] else (d["orientB"], d["orientA"])
        assert d["family"] == 2 and d["kname"] == KNAME and d["elem"] == ELEM[kind] and got == (oa, ob), (mA, mB, d)
        assert d["splitK"] == 1 and d["workspace"] == 0, d
        if kind == "f64":
            assert d["vec"] == 2 and (d["bm"], d["bn"], d["bk"]) == (128, 128, 32), d
        else:
            assert d["vec"] == 1 and (d["bm"], d["bn"], d["bk"]) == (128, 64, 16), d
    # odd extents / element alignment only: 8-byte gathers, the small tile
    for args, kw in (((37, 29, 51, "mk", "kn"), {}), ((64, 64, 64, "km", "kn"), dict(alignment=8)), ((51, 51, 51, "km", "kn"), {})):
        d = described(gemm(env, *args, "32F", "f64", **kw))
        assert d["family"] == 2 and d["kname"] == KNAME and d["elem"] == 8 and d["vec"] == 1 and (d["bm"], d["bn"], d["bk"]) == (64, 64, 32), d
    d = described(gemm(env, 37, 29, 51, "mk", "kn", "32F", "c128", alignment=16))
    assert d["kname"] == KNAME and d["elem"] == 9 and d["vec"] == 1 and (d["bm"], d["bn"], d["bk"]) == (64, 64, 16), d


@pytest.mark.parametrize("kind", sorted(ELEM))
def test_switched_off_and_under_64f_the_description_is_todays(env, monkeypatch, kind):
    """=0: a 32F plan is the 64F plan, byte for byte; 64F is the same plan whatever the switch says"""
    shapes = ((2048, 2048, 2048, "km", "kn"), (4096, 4096, 4096, "mk", "kn"), (37, 29, 51, "mk", "kn"), (128, 128, 65536, "km", "kn"))
    want = [described(gemm(env, *s, "64F", kind)) for s in shapes]
    for d in want:
        assert d["family"] == 2 and d["kname"] == "gett_gen_kernel" and d["elem"] == (2 if kind == "f64" else 4), d
    monkeypatch.setenv("CUTENSOR_AMD_F64X", "0")
    assert [described(gemm(env, *s, "32F", kind)) for s in shapes] == want
    assert [described(gemm(env, *s, "64F", kind)) for s in shapes] == want
    monkeypatch.setenv("CUTENSOR_AMD_F64X", "force")
    assert [described(gemm(env, *s, "64F", kind)) for s in shapes] == want


def test_other_descriptors_data_types_and_named_candidates_are_untouched(env, monkeypatch):
    ct, ops, h = env
    args = (2048, 2048, 2048, "km", "kn")
    base = {c: described(gemm(env, *args, c)) for c in ("64F", "16BF", "TF32", "16F", "3XTF32")}
    f32 = described(gemm(env, *args, "32F", dtype=ct.R_32F))
    c64 = described(gemm(env, *args, "32F", dtype=ct.C_32F))
    named = [described(gemm(env, *args, "32F", kernel_rank=1)), described(gemm(env, *args, "32F", algo=0))]
    monkeypatch.setenv("CUTENSOR_AMD_F64X", "force")
    # the 16-bit / TF32 descriptors on fp64 data stay at full fp64
    for c, want in base.items():
        d = described(gemm(env, *args, c))
        assert d == want and d["family"] == 2 and d["kname"] == "gett_gen_kernel" and d["elem"] == 2, (c, d)
    # fp32 data and complex64 data under their own 32F
    assert described(gemm(env, *args, "32F", dtype=ct.R_32F)) == f32 and f32["family"] == 0
    assert described(gemm(env, *args, "32F", dtype=ct.C_32F)) == c64 and c64["elem"] == 3 and c64["kname"] == "gett_gen_kernel"
    # a caller who names a candidate gets the fp64 plan, as ever
    d1, d2 = described(gemm(env, *args, "32F", kernel_rank=1)), described(gemm(env, *args, "32F", algo=0))
    assert [d1, d2] == named and d1["elem"] == 2 and d2["elem"] == 2 and d1["kname"] == "gett_gen_kernel", (d1, d2)
    assert described(gemm(env, *args, "32F"))["elem"] == 8


@pytest.mark.parametrize("kind", sorted(ELEM))
def test_workspace_contract_and_fp32_partials(env, monkeypatch, kind):
    ct, ops, h = env
    monkeypatch.setenv("CUTENSOR_AMD_F64X", "force")
    shapes = [(2048, 2048, 2048, "km", "kn"), (128, 128, 65536, "km", "kn"), (100, 60, 4099, "mk", "kn")]
    for (M, N, K, mA, mB) in shapes:
        for pref in (ct.WORKSPACE_DEFAULT, ct.WORKSPACE_MAX):
            p = gemm(env, M, N, K, mA, mB, "32F", kind, workspace_limit=None, workspace_pref=pref)
            d = p.describe()
            assert d["family"] == 2 and d["elem"] == ELEM[kind] and p.required_workspace <= p.workspace_estimate, (d, p.workspace_estimate)
            p.destroy()
        p = gemm(env, M, N, K, mA, mB, "32F", kind, workspace_limit=0)
        d = p.describe()
        assert d["family"] == 2 and d["elem"] == ELEM[kind] and d["splitK"] == 1 and p.required_workspace == 0, d
        p.destroy()
    # one output tile row, deep K: split over the chip — fp32 (complex: float2) partials [slice][L][M][N], half of what the fp64 plan takes
    p = gemm(env, 128, 128, 65536, "km", "kn", "32F", kind)
    d = p.describe()
    assert d["splitK"] > 1 and d["workspace"] == d["splitK"] * 128 * 128 * (4 if kind == "f64" else 8) == p.required_workspace, d
    p.destroy()
    d64 = described(gemm(env, 128, 128, 65536, "km", "kn", "64F", kind))
    assert d64["splitK"] > 1 and d64["workspace"] == d64["splitK"] * 128 * 128 * (8 if kind == "f64" else 16), d64


@pytest.mark.parametrize("kind", sorted(ELEM))
def test_64f_and_32f_plans_do_not_meet_in_the_plan_memo(env, monkeypatch, kind):
    """the plan memo holds the compute descriptor in its key (and stands aside while the switch is set)"""
    ct, ops, h = env
    h2 = ops.Handle(plan_cache=64)

    def mk(compute):
        return described(gemm(env, 512, 768, 1024, "km", "kn", compute, kind, handle=h2))
    a = mk("64F")
    monkeypatch.setenv("CUTENSOR_AMD_F64X", "force")
    b = mk("32F")
    monkeypatch.delenv("CUTENSOR_AMD_F64X")
    a2 = mk("64F")
    assert a["kname"] == "gett_gen_kernel" and a2 == a and b["kname"] == KNAME and b["elem"] == ELEM[kind], (a, b)
    # without the switch the memo is live: 64F, then 32F, then both again — each descriptor is answered with its own plan.  (4096^3 /
    # 2048^3: a shape the default planner decides by its model, see the decisions below.)
    E = 4096 if kind == "f64" else 2048

    def big(compute):
        return described(gemm(env, E, E, E, "mk", "kn", compute, kind, handle=h2))
    first = [big("64F"), big("32F")]
    hits = ct.plan_memo_stats(h2.h)[0]
    again = [big("64F"), big("32F")]
    assert ct.plan_memo_stats(h2.h)[0] == hits + 2, "the second pair was not answered from the memo"
    assert first == again and first[0]["kname"] == "gett_gen_kernel" and first[0]["elem"] == (2 if kind == "f64" else 4), first
    monkeypatch.setenv("CUTENSOR_AMD_F64X", "0")
    assert big("32F") == first[0]
    monkeypatch.setenv("CUTENSOR_AMD_F64X", "force")
    forced = big("32F")
    assert forced["kname"] == KNAME and forced != first[0]
    monkeypatch.delenv("CUTENSOR_AMD_F64X")
    assert [big("64F"), big("32F")] == first
    assert first[1] in (first[0], forced)


def test_trinary_and_lone_mode_plans(env, monkeypatch):
    """a trinary contraction keeps fp64 in both of its pairwise plans; the inner contraction of a lone-mode plan picks the path up, its
    reduction stays what it is under 64F"""
    ct, ops, h = env
    import workspace_cases as wc
    e = wc.LONE

    def lone(compute):
        return described(ops.contraction_plan(h, [e[c] for c in "kji"], "kji", [e[c] for c in "lk"], "lk", [e[c] for c in "li"], "li", dtype=ct.R_64F,
                                              compute=compute, workspace_limit=1 << 28))

    def tri(compute):
        return described(ops.contraction_trinary_plan(h, [24, 20, 12], "acd", [20, 16], "cb", [12, 28], "de", [24, 16, 28], "abe", dtype=ct.R_64F,
                                                      compute=compute, workspace_limit=1 << 28))
    l64, t64 = lone("64F"), tri("64F")
    monkeypatch.setenv("CUTENSOR_AMD_F64X", "force")
    d = lone("32F")
    assert d.get("lone_reduce_A") == 1 and d["family"] == 2 and d["elem"] == 8 and d["kname"] == KNAME, d
    assert {k: v for k, v in d.items() if k.startswith("lone")} == {k: v for k, v in l64.items() if k.startswith("lone")}, (d, l64)
    assert tri("32F") == t64


# ---- the default planner at the shapes of tools/bench_f64_compute.py ---------------------------------------------------------------------
# (kind, M, N, K, mA, mB) -> the kernel a default-planner 32F plan names.  As measured — profiles/f64x_compute.jsonl, the
# {"record": "decision"} line of each shape (forced_over_64F = forced-32F time / 64F time in one process; below 0.8 everywhere):
#   f64 4096^3 mk,kn 0.57   km,kn 0.60   mk,nk 0.55   2048^3 0.56   4096^2 x 512 0.62   1024^3 0.56   8192^2 x 256 0.65
#   c128 2048^3 0.59   1024^3 0.59
# and the {"record": "summary"} line: forced 103.7 / 105.1 TFLOP/s at f64 4096^3 / c128 2048^3 = 0.66 / 0.67 of 157.3.
NEW, OLD = KNAME, "gett_gen_kernel"
BENCH_DECISIONS = [
    (("f64", 4096, 4096, 4096, "mk", "kn"), NEW), (("f64", 4096, 4096, 4096, "km", "kn"), NEW), (("f64", 4096, 4096, 4096, "mk", "nk"), NEW),
    (("f64", 2048, 2048, 2048, "mk", "kn"), NEW), (("f64", 4096, 4096, 512, "mk", "kn"), NEW), (("f64", 1024, 1024, 1024, "mk", "kn"), NEW),
    (("f64", 8192, 8192, 256, "mk", "kn"), NEW), (("c128", 2048, 2048, 2048, "mk", "kn"), NEW), (("c128", 1024, 1024, 1024, "mk", "kn"), NEW),
]


def _recorded_decisions():
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "f64x_compute.jsonl")
    out = {}
    for line in open(path):
        r = json.loads(line)
        if r.get("record") == "decision":
            out[(r["kind"], r["M"], r["N"], r["K"], r["mA"], r["mB"])] = r
    return out


@pytest.mark.parametrize("shape,want", BENCH_DECISIONS, ids=["%s_%dx%dx%d_%s_%s" % s for s, _ in BENCH_DECISIONS])
def test_default_planner_decisions_at_the_bench_shapes(env, shape, want):
    """no switch: the 32F plan of every bench shape names the kernel pinned above; where that is the new kernel it is the forced plan,
    unsplit; where it is the fp64 kernel the description is the 64F plan's byte for byte.  The committed sweep agrees: it ran that kernel
    by default, and where the planner takes the new kernels the forced kernel measured below 0.8 x the 64F time there."""
    kind, M, N, K, mA, mB = shape
    d32, d64 = described(gemm(env, M, N, K, mA, mB, "32F", kind)), described(gemm(env, M, N, K, mA, mB, "64F", kind))
    assert d64["kname"] == OLD
    assert d32["kname"] == want, d32
    if want == NEW:
        assert d32["elem"] == ELEM[kind] and d32["splitK"] == 1, d32
    else:
        assert d32 == d64, (d32, d64)
    r = _recorded_decisions().get(shape)
    assert r is not None, "profiles/f64x_compute.jsonl has no decision record for %r" % (shape,)
    assert r["default_32F_kernel"] == want and (want == OLD or r["forced_32F_us"] < 0.8 * r["64F_us"]), r
