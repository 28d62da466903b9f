"""Type conversion in cutensorPermute and the binary form, on the CPU planner (no GPU; the table is tests/convert_cases.py): every case
plans onto the path it names with the table's scalar type, every draw is exact in A's, C's and D's types, every refusal the interface
documents is CUTENSOR_STATUS_NOT_SUPPORTED, a converting plan and the same-type plan of the same shapes do not meet in the plan memo,
and the moved bytes count |D| (sizeof A + sizeof D) (+ |D| sizeof D with C)."""
import ctypes

import pytest

import convert_cases as cc
import exact_cases as xc
import workspace_cases as wc


@pytest.fixture(scope="module")
def env(built):
    from cudalibrarysamples_amd import cutensor as ct, ops
    return ct, ops, ops.Handle()


def test_the_table_names_the_library_s_data_types(env):
    ct = env[0]
    assert cc.HIP == {"float32": ct.R_32F, "float64": ct.R_64F, "float16": ct.R_16F, "bfloat16": ct.R_16BF}


@pytest.mark.parametrize("case", cc.CASES + [cc.PAD_CASE], ids=[c.id for c in cc.CASES + [cc.PAD_CASE]])
def test_case_is_on_its_path_and_its_draws_hold(env, case):
    ct, ops, h = env
    kw = dict(padding=(cc.PAD_LEFT, cc.PAD_RIGHT, cc.PAD_VALUE)) if case is cc.PAD_CASE else {}
    d = cc.plan_path(ct, ops, h, case, **kw)
    assert d["convert"] == [cc.HIP[case.dtypeA], cc.HIP[case.dtype]]
    cc.check_case(case)


def test_the_table_reaches_every_form_of_every_pair():
    for pair in cc.PAIRS:
        mine = [c for c in cc.CASES if c.pair == pair]
        for kind in ("permutation", "binary"):
            ids = " ".join(c.id for c in mine if c.kind == kind)
            assert all(w in ids for w in ("rowcopy", "transpose", "generic")), (pair, kind, ids)
        # the transposing tiles of the pair: every width its rule can give
        park_perm = min(cc.SIZE[pair[0]], cc.SIZE[pair[1]])
        assert {cc.tile0(pair, False, e) for e in (33 * cc.lane(pair), 256, 384)} == {t for t in (64, 128, 256) if t * 64 * park_perm <= 32768}


def _status(ct, fn):
    try:
        fn().destroy()
    except Exception as e:                                                     # ct.check raises with the status name
        return str(e)
    return "SUCCESS"


def _refused(ct, fn, what):
    st = _status(ct, fn)
    assert "NOT_SUPPORTED" in st, "%s: %s" % (what, st)


E, MA, MD = [16, 8, 24], "abc", "cba"


def test_every_other_mixture_is_refused(env):
    ct, ops, h = env
    T = {"bf16": ct.R_16BF, "f16": ct.R_16F, "f32": ct.R_32F, "f64": ct.R_64F, "c64": ct.C_32F, "c128": ct.C_64F}
    ED = [24, 8, 16]
    perm = lambda a, d, **kw: ops.permutation_plan(h, E, MA, ED, MD, dtype=T[a], dtypeB=T[d], **kw)   # noqa: E731
    bina = lambda a, d, **kw: ops.binary_plan(h, E, MA, ED, MD, dtype=T[a], dtypeC=T[d], **kw)         # noqa: E731
    # (positive control: the table's pairs plan, under the table's compute descriptor, which is also the helpers' default)
    for a, d, comp in (("bf16", "f32", "32F"), ("f16", "f32", "32F"), ("f32", "bf16", "32F"), ("f32", "f16", "32F"), ("f32", "f64", "64F"),
                       ("f64", "f32", "64F")):
        assert _status(ct, lambda: perm(a, d, compute=comp)) == "SUCCESS"
        assert _status(ct, lambda: bina(a, d, compute=comp)) == "SUCCESS"
        # a pair under a compute descriptor other than its row's
        for other in ("16F", "16BF", "TF32", "32F", "64F"):
            if other != comp:
                _refused(ct, lambda: perm(a, d, compute=other), "%s -> %s under %s" % (a, d, other))
                _refused(ct, lambda: bina(a, d, compute=other), "%s -> %s under %s (binary)" % (a, d, other))
    # any other pair
    for a, d in (("bf16", "f16"), ("f16", "bf16"), ("bf16", "f64"), ("f64", "bf16"), ("f16", "f64"), ("f64", "f16"), ("f32", "c64"), ("c64", "f32"),
                 ("c64", "c128"), ("c128", "c64"), ("f64", "c128"), ("c128", "f64"), ("f32", "c128")):
        for comp in ("32F", "64F"):
            _refused(ct, lambda: perm(a, d, compute=comp), "%s -> %s" % (a, d))
            _refused(ct, lambda: bina(a, d, compute=comp), "%s -> %s (binary)" % (a, d))

    # C's type differs from D's
    def binary_acd(ta, tc, td, comp):
        dA, dC, dD = ops.tensor_descriptor(h, E, None, T[ta]), ops.tensor_descriptor(h, ED, None, T[tc]), ops.tensor_descriptor(h, ED, None, T[td])
        opd = ctypes.c_void_p()
        st = ct.cutensorCreateElementwiseBinary(h.h, ctypes.byref(opd), dA, ct.i32(MA), ct.OP_IDENTITY, dC, ct.i32(MD), ct.OP_IDENTITY, dD, ct.i32(MD),
                                                ct.OP_ADD, ct.compute_desc(comp))
        for d in (dA, dC, dD):
            ct.cutensorDestroyTensorDescriptor(d)
        ct.check(st)
        return ops.Plan(h, opd, "binary", T[ta], workspace_limit=0)
    assert _status(ct, lambda: binary_acd("bf16", "f32", "f32", "32F")) == "SUCCESS"
    _refused(ct, lambda: binary_acd("bf16", "bf16", "f32", "32F"), "C of A's type")
    _refused(ct, lambda: binary_acd("f32", "f32", "bf16", "32F"), "C of A's type")
    _refused(ct, lambda: binary_acd("f32", "f64", "f32", "64F"), "C wider than D")

    # the other entry points stay same-type
    def tri(ta, tb, tc, td):
        d = [ops.tensor_descriptor(h, E, None, T[ta]), ops.tensor_descriptor(h, E, None, T[tb]), ops.tensor_descriptor(h, ED, None, T[tc]),
             ops.tensor_descriptor(h, ED, None, T[td])]
        opd = ctypes.c_void_p()
        st = ct.cutensorCreateElementwiseTrinary(h.h, ctypes.byref(opd), d[0], ct.i32(MA), ct.OP_IDENTITY, d[1], ct.i32(MA), ct.OP_IDENTITY, d[2], ct.i32(MD),
                                                 ct.OP_IDENTITY, d[3], ct.i32(MD), ct.OP_ADD, ct.OP_ADD, ct.compute_desc("32F"))
        for x in d:
            ct.cutensorDestroyTensorDescriptor(x)
        ct.check(st)
        return ops.Plan(h, opd, "trinary", T[ta], workspace_limit=0)
    assert _status(ct, lambda: tri("f32", "f32", "f32", "f32")) == "SUCCESS"
    for mix in (("bf16", "bf16", "f32", "f32"), ("bf16", "f32", "f32", "f32"), ("f32", "bf16", "f32", "f32"), ("f32", "f32", "bf16", "bf16"),
                ("f32", "f32", "f32", "bf16"), ("f32", "f32", "bf16", "f32")):
        _refused(ct, lambda: tri(*mix), "trinary %s" % (mix,))

    def red(ta, td):
        dA, dD = ops.tensor_descriptor(h, E, None, T[ta]), ops.tensor_descriptor(h, [16, 24], None, T[td])
        opd = ctypes.c_void_p()
        st = ct.cutensorCreateReduction(h.h, ctypes.byref(opd), dA, ct.i32(MA), ct.OP_IDENTITY, dD, ct.i32("ac"), ct.OP_IDENTITY, dD, ct.i32("ac"), ct.OP_ADD,
                                        ct.compute_desc("32F"))
        ct.cutensorDestroyTensorDescriptor(dA)
        ct.cutensorDestroyTensorDescriptor(dD)
        ct.check(st)
        return ops.Plan(h, opd, "reduction", T[ta])
    assert _status(ct, lambda: red("f32", "f32")) == "SUCCESS"
    _refused(ct, lambda: red("bf16", "f32"), "reduction bf16 -> f32")
    _refused(ct, lambda: red("f32", "bf16"), "reduction f32 -> bf16")

    def contraction(ta, tb, tc):
        d = [ops.tensor_descriptor(h, [32, 16], None, T[ta]), ops.tensor_descriptor(h, [16, 24], None, T[tb]), ops.tensor_descriptor(h, [32, 24], None, T[tc])]
        opd = ctypes.c_void_p()
        st = ct.cutensorCreateContraction(h.h, ctypes.byref(opd), d[0], ct.i32("mk"), ct.OP_IDENTITY, d[1], ct.i32("kn"), ct.OP_IDENTITY, d[2], ct.i32("mn"),
                                          ct.OP_IDENTITY, d[2], ct.i32("mn"), ct.compute_desc("32F"))
        for x in d:
            ct.cutensorDestroyTensorDescriptor(x)
        ct.check(st)
        return ops.Plan(h, opd, "contraction", T[ta])
    assert _status(ct, lambda: contraction("f32", "f32", "f32")) == "SUCCESS"
    _refused(ct, lambda: contraction("bf16", "bf16", "f32"), "contraction bf16 x bf16 -> f32")
    _refused(ct, lambda: contraction("f32", "bf16", "f32"), "contraction f32 x bf16")

    def blocksparse(ta, tb, tc):
        sec = dict(m=[8, 8], k=[8], n=[8])
        descs = []
        for modes, coords, t in (("mk", [(0, 0), (1, 0)], ta), ("kn", [(0, 0)], tb), ("mn", [(0, 0), (1, 0)], tc)):
            d = ctypes.c_void_p()
            ct.check(ct.cutensorCreateBlockSparseTensorDescriptor(h.h, ctypes.byref(d), len(modes), len(coords), (ctypes.c_uint32 * len(modes))(*[len(sec[c]) for c in modes]),
                                                                  ct.i64([e for c in modes for e in sec[c]]), ct.i32([x for c in coords for x in c]), None, T[t]))
            descs.append(d)
        opd = ctypes.c_void_p()
        st = ct.cutensorCreateBlockSparseContraction(h.h, ctypes.byref(opd), descs[0], ct.i32("mk"), ct.OP_IDENTITY, descs[1], ct.i32("kn"), ct.OP_IDENTITY,
                                                     descs[2], ct.i32("mn"), ct.OP_IDENTITY, descs[2], ct.i32("mn"), ct.compute_desc("32F"))
        for d in descs:
            ct.cutensorDestroyBlockSparseTensorDescriptor(d)
        ct.check(st)
        return ops.Plan(h, opd, "blocksparse", T[ta])
    assert _status(ct, lambda: blocksparse("f32", "f32", "f32")) == "SUCCESS"
    _refused(ct, lambda: blocksparse("f32", "f32", "f64"), "block-sparse f32 x f32 -> f64")
    _refused(ct, lambda: blocksparse("f64", "f32", "f32"), "block-sparse f64 x f32")


def test_unary_operators_are_judged_on_both_sides(env):
    ct, ops, h = env
    p = ops.permutation_plan(h, E, MA, [24, 8, 16], MD, dtype=ct.R_32F, dtypeB=ct.R_16BF, opA="SQRT")
    d = wc.describe(ct, p)
    p.destroy()
    assert d.get("unary") == [ct.OP_SQRT, ct.OP_IDENTITY, ct.OP_IDENTITY] and d.get("convert") == [ct.R_32F, ct.R_16BF], d.raw
    _refused(ct, lambda: ops.permutation_plan(h, E, MA, [24, 8, 16], MD, dtype=ct.C_32F, dtypeB=ct.R_32F, opA="SQRT"), "SQRT on complex A")


@pytest.mark.parametrize("kind", ("permutation", "binary"))
@pytest.mark.parametrize("pair", cc.PAIRS, ids=[cc._name(p) for p in cc.PAIRS])
def test_a_converting_plan_does_not_meet_the_same_type_plan_in_the_memo(env, pair, kind):
    """the same shapes planned same-type (in A's type and in D's) before and after a converting plan on ONE handle with the plan cache on:
    the descriptions a fresh handle gives, and each new problem is a memo miss"""
    ct, ops, _ = env
    lv = cc.lane(pair)
    ext = dict(a=17 * lv, b=3, c=33 * lv)
    dA, dD = xc._dt(ct, pair[0]), xc._dt(ct, pair[1])

    def plan(h, ta, td):
        if kind == "permutation":
            p = ops.permutation_plan(h, [ext[c] for c in "abc"], "abc", [ext[c] for c in "cba"], "cba", dtype=ta, dtypeB=td)
        else:
            p = ops.binary_plan(h, [ext[c] for c in "abc"], "abc", [ext[c] for c in "cba"], "cba", dtype=ta, dtypeC=td)
        raw = wc.describe(ct, p).raw
        p.destroy()
        return raw
    alone = {}
    for ta, td in ((dA, dA), (dD, dD), (dA, dD)):
        h0 = ops.Handle(plan_cache=64)
        alone[(ta, td)] = plan(h0, ta, td)
        h0.close()
    assert '"convert"' in alone[(dA, dD)] and '"convert"' not in alone[(dA, dA)] and '"convert"' not in alone[(dD, dD)]
    h = ops.Handle(plan_cache=64)
    order = [(dA, dA), (dA, dD), (dD, dD), (dA, dA), (dA, dD), (dD, dD)]
    for i, key in enumerate(order):
        assert plan(h, *key) == alone[key], (i, key)
        hits, misses, entries = ct.plan_memo_stats(h.h)
        assert (hits, misses, entries) == (max(0, i - 2), min(i + 1, 3), min(i + 1, 3)), (i, hits, misses, entries)
    h.close()


@pytest.mark.parametrize("pair", cc.PAIRS, ids=[cc._name(p) for p in cc.PAIRS])
def test_moved_bytes_and_scalar_type(env, pair):
    ct, ops, h = env
    dA, dD = xc._dt(ct, pair[0]), xc._dt(ct, pair[1])
    n = 16 * 8 * 24
    for kind, want in (("permutation", n * (cc.SIZE[pair[0]] + cc.SIZE[pair[1]])), ("binary", n * (cc.SIZE[pair[0]] + 2 * cc.SIZE[pair[1]]))):
        p = (ops.permutation_plan(h, E, MA, [24, 8, 16], MD, dtype=dA, dtypeB=dD) if kind == "permutation" else
             ops.binary_plan(h, E, MA, [24, 8, 16], MD, dtype=dA, dtypeC=dD))
        moved, st = ctypes.c_float(0), ctypes.c_int(-1)
        ct.check(ct.cutensorOperationDescriptorGetAttribute(h.h, p.op, ct.OPERATION_DESCRIPTOR_MOVED_BYTES, ctypes.byref(moved), 4))
        ct.check(ct.cutensorOperationDescriptorGetAttribute(h.h, p.op, ct.OPERATION_DESCRIPTOR_SCALAR_TYPE, ctypes.byref(st), 4))
        assert moved.value == float(want), (kind, moved.value, want)
        assert st.value == xc._dt(ct, cc.scalar_type(pair)) == p.scalar_type
        assert isinstance(p.scalar(1.0), ctypes.c_double if "float64" in pair else ctypes.c_float)
        p.destroy()
