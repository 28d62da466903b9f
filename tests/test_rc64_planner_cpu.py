"""How the planner takes the two mixed rows of the contraction type table — one input R_64F, the other one, C and D C_64F, complex double
scalars, COMPUTE_DESC_64F (csrc/kernels/gett_gen_rc64.inc) — host-only: every case of tests/rc64_cases.py plans on its path, the real
operand's width, split-K, the lone-mode reduction, peeling and the mode table, the workspace contract, every refusal, and — against
descriptions recorded on the commit before the feature (tests/golden/rc64_unchanged_descriptions.json, tools/
gen_rc64_unchanged_descriptions.py) — that all-fp64 and all-complex128 descriptors plan exactly as they did."""
import ctypes
import json
import os
import sys

import pytest

import rc64_cases as rc
import workspace_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def env(built):
    from cudalibrarysamples_amd import cutensor as ct, ops
    return ct, ops, ops.Handle()


@pytest.mark.parametrize("cid", rc.IN_PROCESS)
def test_every_case_plans_on_its_path(env, cid):
    """new kname / elem / "real" (both type orders, four layouts, both kernel sides), vec, split-K, lone reduction, peel; scalar type C_64F;
    estimate >= required workspace"""
    ct, ops, h = env
    rc.plan_path(ct, ops, h, rc.BY_ID[cid])


def test_both_kernel_sides_and_every_table_row_group_are_planned(env):
    """over the ragged and the vector-width cases the real tensor runs as kernel-A and as kernel-B on every orientation pair, at both widths;
    the kernel index is that row of the table behind every earlier kernel"""
    ct, ops, h = env
    seen, base = set(), set()
    for c in rc.CASES:
        if not c.id.startswith(("ragged_", "vec")):
            continue
        d = rc.plan_path(ct, ops, h, c)
        side = d.get("real") ^ d.get("swapped")
        row = side * 8 + (0 if d.get("vec") == 2 else 4) + 2 * d.get("orientA") + d.get("orientB")
        base.add(d.get("kernel") - row)
        seen.add((side, d.get("orientA"), d.get("orientB")))
        assert (d.get("bm"), d.get("bn"), d.get("bk")) == (64, 64, 8), d.raw
    assert len(base) == 1, base
    assert seen == {(s, a, b) for s in (0, 1) for a in (0, 1) for b in (0, 1)}, sorted(seen)
    # appended at the END of the family's table: the complex128 rows keep their indices (the recorded descriptions name kernel 56 .. 59)
    assert base.pop() > 59


def test_vec_follows_the_real_operands_alignment_and_extents(env):
    ct, ops, h = env

    def vec(ext, real, align_real=128, off=0):
        c = rc.Case("probe", ext, ("km", "kn", "nm"), real, rc.tiled(real), align_real=align_real, off=off)
        return rc.plan_path(ct, ops, h, c).get("vec")
    for real in (0, 1):
        assert vec(dict(m=64, n=48, k=40), real) == 2
        assert vec(dict(m=64, n=48, k=40), real, align_real=8, off=1) == 1          # an odd element offset
        assert vec(dict(m=64, n=48, k=37), real) == 1                                 # an odd extent of the real operand's stride-1 mode
    # the COMPLEX operand's extents and alignment do not narrow the real one: 'mk,kn' with m odd, the real B contiguous in k
    c = rc.Case("probe", dict(m=63, n=48, k=40), ("mk", "kn", "nm"), 1, rc.tiled(1))
    assert rc.plan_path(ct, ops, h, c).get("vec") == 2


def test_long_k_splits_into_complex128_partials(env):
    ct, ops, h = env
    for real in (0, 1):
        c = rc.Case("probe", dict(m=128, n=128, k=65536), ("km", "kn", "mn"), real, rc.tiled(real, split=True))
        d = rc.plan_path(ct, ops, h, c)
        assert d.get("workspace") == d.get("splitK") * 128 * 128 * 16, d.raw
        c0 = rc.Case("probe", dict(m=128, n=128, k=65536), ("km", "kn", "mn"), real, rc.tiled(real, split=False), ws_limit=0)
        assert rc.plan_path(ct, ops, h, c0).get("workspace") == 0
    # ... decided as for complex128: the same slices
    p = ops.contraction_plan(h, [65536, 128], "km", [65536, 128], "kn", [128, 128], "mn", dtype=ct.C_64F, workspace_limit=1 << 28)
    d128 = p.describe()
    p.destroy()
    assert (d128["splitK"], d128["kPerSlice"]) == (d.get("splitK"), d.get("kPerSlice")), (d128, d.raw)


def test_lone_mode_of_the_real_operand_is_a_real_reduction(env, capfd):
    """'ijk,kl->il' with the real operand carrying j: its first step is an fp64 reduction with double scalars into a real temporary"""
    ct, ops, h = env
    d = rc.plan_path(ct, ops, h, rc.BY_ID["lone_on_real"])
    e = wc.LONE
    assert d.get("lone_reduce_A") == 1 and d.get("lone_bytes") == 8 * e["k"] * e["i"], d.raw            # 8 bytes per element of the temporary
    d = rc.plan_path(ct, ops, h, rc.BY_ID["lone_on_complex"])
    assert d.get("lone_reduce_A") == 1 and d.get("lone_bytes") == 16 * e["k"] * e["i"], d.raw


def test_wide_views_peel_or_reach_the_mode_table(env):
    ct, ops, h = env
    for cid in ("peeled_realA", "peeled_realB"):
        d = rc.plan_path(ct, ops, h, rc.BY_ID[cid])
        assert d.get("peel_launches") >= 2 and d.get("elem") == rc.ELEM, d.raw
    import exact_cases as xc
    out = xc.in_child([c.id for c in rc.CASES if c.group == "peel0"], {"CUTENSOR_AMD_PEEL": "0"}, 120, mode="plan", script="rc64_cases.py")
    assert "ok mode_table_realA" in out and "ok mode_table_realB" in out


def test_attributes_scalar_type_and_moved_bytes(env):
    ct, ops, h = env
    M, N, K = 64, 48, 40
    for real in (0, 1):
        c = rc.Case("probe", dict(m=M, n=N, k=K), ("km", "kn", "mn"), real, rc.tiled(real))
        plan = rc.make_plan(ct, ops, h, c)
        try:
            assert plan.scalar_type == ct.C_64F
            moved = ctypes.c_float(0)
            ct.check(ct.cutensorOperationDescriptorGetAttribute(h.h, plan.op, ct.OPERATION_DESCRIPTOR_MOVED_BYTES, ctypes.byref(moved), 4))
            ea, eb = (8, 16) if real == 0 else (16, 8)
            assert moved.value == float(ea * M * K + eb * K * N + 16 * M * N), moved.value
        finally:
            plan.destroy()


def test_named_candidates_and_autotuning_get_the_one_mixed_plan(env):
    ct, ops, h = env
    c = rc.Case("probe", dict(m=63, n=45, k=37), ("km", "kn", "mn"), 0, rc.tiled(0))
    want = rc.plan_path(ct, ops, h, c).raw
    e, m = c.extents, c.modes
    for kw in (dict(algo=0), dict(algo=3), dict(kernel_rank=2), dict(algo=ct.ALGO_DEFAULT_PATIENT), dict(autotune=ct.AUTOTUNE_MODE_INCREMENTAL, incremental_count=3)):
        p = ops.contraction_plan(h, e(m[0]), m[0], e(m[1]), m[1], e(m[2]), m[2], dtype=ct.C_64F, dtypeA=ct.R_64F, workspace_limit=1 << 28, **kw)
        try:
            assert wc.describe(ct, p).raw == want, kw
        finally:
            p.destroy()


def test_mixed_and_complex128_plans_do_not_meet_in_the_plan_memo(env):
    """C_64F x R_64F differs from C_64F x C_64F only in B's type: the memo and the plan cache key hold it"""
    ct, ops, _ = env
    h2 = ops.Handle(plan_cache=64)
    ext, modes = dict(m=63, n=45, k=37), ("km", "kn", "mn")

    def mk(**kw):
        p = ops.contraction_plan(h2, [ext[c] for c in modes[0]], modes[0], [ext[c] for c in modes[1]], modes[1], [ext[c] for c in modes[2]], modes[2],
                                 dtype=ct.C_64F, workspace_limit=1 << 28, **kw)
        d = p.describe()
        p.destroy()
        return d
    a, b, c, a2, b2 = mk(), mk(dtypeB=ct.R_64F), mk(dtypeA=ct.R_64F), mk(), mk(dtypeB=ct.R_64F)
    assert a == a2 and b == b2 and a["kname"] == "gett_gen_kernel" and "real" not in a
    assert b["kname"] == rc.KNAME and b["real"] == 1 and c["kname"] == rc.KNAME and c["real"] == 0


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def _create(ct, ops, h, tA, tB, tC, tD, compute="64F", ext=None, modes=("km", "kn", "mn")):
    ext = ext or dict(m=16, n=16, k=16)
    d = [ops.tensor_descriptor(h, [ext[c] for c in m], None, t, 16) for m, t in zip((modes[0], modes[1], modes[2], modes[2]), (tA, tB, tC, tD))]
    op = ctypes.c_void_p()
    st = ct.cutensorCreateContraction(h.h, ctypes.byref(op), d[0], ct.i32(modes[0]), ct.OP_IDENTITY, d[1], ct.i32(modes[1]), ct.OP_IDENTITY, d[2],
                                      ct.i32(modes[2]), ct.OP_IDENTITY, d[3], ct.i32(modes[2]), ct.compute_desc(compute))
    for x in d:
        ct.cutensorDestroyTensorDescriptor(x)
    if st == ct.STATUS_SUCCESS:
        ct.cutensorDestroyOperationDescriptor(op)
    return st


def test_the_two_rows_are_accepted_and_every_other_combination_is_refused(env):
    ct, ops, h = env
    R64, C64, R32, C32 = ct.R_64F, ct.C_64F, ct.R_32F, ct.C_32F
    assert _create(ct, ops, h, R64, C64, C64, C64) == ct.STATUS_SUCCESS
    assert _create(ct, ops, h, C64, R64, C64, C64) == ct.STATUS_SUCCESS
    refused = [(R64, C64, R64, R64), (R64, C64, C64, R64), (R64, C64, R64, C64), (C64, R64, R64, R64),      # real C or D
               (R32, C32, C32, C32), (C32, R32, C32, C32),                                                  # R_32F with C_32F
               (R64, C32, C32, C32), (R32, C64, C64, C64), (R64, R64, C64, C64), (C64, C64, R64, R64)]      # any other mixture
    for types in refused:
        assert _create(ct, ops, h, *types) == ct.STATUS_NOT_SUPPORTED, types
    # the compute descriptor: 64F only
    for compute in ("32F", "3XTF32", "TF32", "16F", "16BF"):
        assert _create(ct, ops, h, R64, C64, C64, C64, compute) == ct.STATUS_NOT_SUPPORTED, compute
        assert _create(ct, ops, h, C64, R64, C64, C64, compute) == ct.STATUS_NOT_SUPPORTED, compute


def test_refusals_name_their_reason_in_the_log():
    """CUTENSOR_LOG_LEVEL is read once per process: a child creates a refused descriptor of each kind"""
    import subprocess
    code = ("import ctypes, sys; sys.path[:0] = [%r, %r]\n"
            "from cudalibrarysamples_amd import cutensor as ct, ops\n"
            "import test_rc64_planner_cpu as t\n"
            "h = ops.Handle()\n"
            "print(t._create(ct, ops, h, ct.R_64F, ct.C_64F, ct.C_64F, ct.C_64F, '32F'))\n"
            "print(t._create(ct, ops, h, ct.R_64F, ct.C_64F, ct.R_64F, ct.R_64F))\n"
            "print(t._create(ct, ops, h, ct.R_32F, ct.C_32F, ct.C_32F, ct.C_32F))\n") % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, CUTENSOR_LOG_LEVEL="1", CTAMD_LIB_FLAVOUR="hooks"))
    assert r.returncode == 0 and r.stdout.split() == ["15", "15", "15"], r.stdout + r.stderr
    assert "COMPUTE_DESC_64F only" in r.stderr and r.stderr.count("mixed data types") >= 3, r.stderr


def test_trinary_and_block_sparse_contractions_refuse_mixed_types(env):
    ct, ops, h = env
    dts = {"acd": ct.R_64F, "cb": ct.C_64F, "de": ct.C_64F, "abe": ct.C_64F}
    ext = dict(a=6, b=5, c=8, d=4, e=7)
    d = {m: ops.tensor_descriptor(h, [ext[c] for c in m], None, t, 16) for m, t in dts.items()}
    op = ctypes.c_void_p()
    st = ct.cutensorCreateContractionTrinary(h.h, ctypes.byref(op), d["acd"], ct.i32("acd"), ct.OP_IDENTITY, d["cb"], ct.i32("cb"), ct.OP_IDENTITY,
                                             d["de"], ct.i32("de"), ct.OP_IDENTITY, d["abe"], ct.i32("abe"), ct.OP_IDENTITY, d["abe"], ct.i32("abe"),
                                             ct.compute_desc("64F"))
    for x in d.values():
        ct.cutensorDestroyTensorDescriptor(x)
    assert st == ct.STATUS_NOT_SUPPORTED
    # block-sparse: A of another type than B, C, D
    descs = []
    for m, dt in (("ki", ct.R_64F), ("k", ct.C_64F), ("i", ct.C_64F)):
        bd = ctypes.c_void_p()
        ct.check(ct.cutensorCreateBlockSparseTensorDescriptor(h.h, ctypes.byref(bd), len(m), 1, (ctypes.c_uint32 * len(m))(*[1] * len(m)),
                                                              ct.i64([8] * len(m)), ct.i32([0] * len(m)), None, dt))
        descs.append(bd)
    st = ct.cutensorCreateBlockSparseContraction(h.h, ctypes.byref(op), descs[0], ct.i32("ki"), ct.OP_IDENTITY, descs[1], ct.i32("k"), ct.OP_IDENTITY,
                                                 descs[2], ct.i32("i"), ct.OP_IDENTITY, descs[2], ct.i32("i"), ct.compute_desc("64F"))
    for bd in descs:
        ct.cutensorDestroyBlockSparseTensorDescriptor(bd)
    assert st == ct.STATUS_NOT_SUPPORTED


# ---- nothing else moved --------------------------------------------------------------------------------------------------------------------
def test_fp64_and_complex128_descriptions_are_the_recorded_ones(env):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_rc64_unchanged_descriptions as gen
    finally:
        sys.path.pop(0)
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "rc64_unchanged_descriptions.json")))
    got = gen.describe_all()
    assert sorted(got) == sorted(want) and len(want) >= 40
    diff = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not diff, diff
