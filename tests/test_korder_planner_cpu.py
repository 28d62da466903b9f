"""The order of the contracted digits in a plan's GETT view (describe()["Kdigits"], fastest first: [extent, strideA, strideB]), host-only.

A split-K plan of the streaming fp32 kernel (gett_f32_stream_kernel, 96 x 96 on the 3-deep ring) in which exactly ONE operand is
K-contiguous keeps that operand's stride-1 digit first — its LDS image stays rows of 128 bytes — and orders the remaining contracted
modes by the OTHER operand's strides, smallest first: a workgroup's consecutive K-tiles then read neighbouring rows of that operand
(plan_contraction.cpp, stream_k_order).  The kernel, the split and the slice length are chosen before the order and do not move.
Every other plan keeps the K-contiguous operand's order (A's when neither or both are), digit for digit, and so does every plan under
CUTENSOR_AMD_KORDER=A."""
import pytest

HEAD = dict(a=96, e=96, b=64, c=64, d=64)


@pytest.fixture(scope="module")
def env(built):
    from cudalibrarysamples_amd import cutensor as ct, ops
    return ct, ops, ops.Handle()


def describe(env, ext, mA, mB, mC, **kw):
    ct, ops, h = env
    kw.setdefault("workspace_limit", 1 << 30)
    kw.setdefault("cache_mode", ct.CACHE_MODE_NONE)
    p = ops.contraction_plan(h, [ext[c] for c in mA], mA, [ext[c] for c in mB], mB, [ext[c] for c in mC], mC, **kw)
    d = p.describe()
    p.destroy()
    return d


def packed_strides(ext, modes):
    s, acc = {}, 1
    for c in modes:
        s[c] = acc
        acc *= ext[c]
    return s


def digits_in_order_of(ext, mA, mB, order, swapped=False):
    """Unfused digits of the modes `order` (fastest first) of packed operands"""
    sA, sB = packed_strides(ext, mA), packed_strides(ext, mB)
    if swapped:
        sA, sB = sB, sA
    return [[ext[c], sA[c], sB[c]] for c in order]


def both_orders(env, monkeypatch, *args, **kw):
    d = describe(env, *args, **kw)
    monkeypatch.setenv("CUTENSOR_AMD_KORDER", "A")
    old = describe(env, *args, **kw)
    monkeypatch.delenv("CUTENSOR_AMD_KORDER")
    return d, old


def test_headline_orders_the_upper_digits_by_the_other_operand(env, monkeypatch):
    d, old = both_orders(env, monkeypatch, HEAD, "dcba", "ebcd", "ea")
    assert d["Kdigits"] == [[64, 1, 393216], [64, 4096, 96], [64, 64, 6144]], d
    assert old["Kdigits"] == [[64, 1, 393216], [64, 64, 6144], [64, 4096, 96]], old
    assert d["kname"] == "gett_f32_stream_kernel" and (d["bm"], d["bn"], d["pf"], d["splitK"], d["kPerSlice"]) == (96, 96, 3, 256, 1024), d
    for key in ("kernel", "kname", "splitK", "kPerSlice", "blocks", "workspace", "layA", "layB", "swapped", "nt", "model_us"):
        assert d[key] == old[key], (key, d, old)


def test_headline_under_the_streamed_preference_and_with_the_roles_swapped(env, monkeypatch):
    d, old = both_orders(env, monkeypatch, HEAD, "dcba", "ebcd", "ea", operands_streamed=True)
    assert d["nt"] == 1 and d["Kdigits"] == [[64, 1, 393216], [64, 4096, 96], [64, 64, 6144]] and d["kernel"] == old["kernel"], d
    # D's fastest mode in A: the user's A plays kernel-B, the K-contiguous operand is kernel-B and the order follows kernel-A's strides
    d, old = both_orders(env, monkeypatch, HEAD, "abcd", "dcbe", "ae")
    assert d["swapped"] == 1 and (d["layA"], d["layB"]) == (1, 0) and d["splitK"] == 256, d
    assert d["Kdigits"] == digits_in_order_of(HEAD, "abcd", "dcbe", "dbc", swapped=True), d
    assert old["Kdigits"] == digits_in_order_of(HEAD, "abcd", "dcbe", "dcb", swapped=True), old


def test_unequal_extents_keep_each_digit_with_its_strides(env, monkeypatch):
    ext = dict(a=96, e=96, d=64, c=5, b=8)

    def ring3(split):
        """the 96 x 96 ring-3 streaming candidate at a forced split (CUTENSOR_AMD_F32_SPLITK, hooks flavour)"""
        monkeypatch.setenv("CUTENSOR_AMD_F32_SPLITK", str(split))
        for algo in range(64):
            d = describe(env, ext, "dcba", "ebcd", "ea", algo=algo)
            if d["kname"] == "gett_f32_stream_kernel" and (d["bm"], d["pf"], d["nt"]) == (96, 3, 0):
                return d
        raise AssertionError("no ring-3 streaming candidate")

    d = ring3(8)
    assert d["splitK"] == 8 and d["kPerSlice"] == 320, d
    assert d["Kdigits"] == digits_in_order_of(ext, "dcba", "ebcd", "dbc") == [[64, 1, 96 * 8 * 5], [8, 320, 96], [5, 64, 768]], d
    # a shorter last slice (80 K-tiles in slices of 7, 7, ... 3) is still a launch of the flat entry: the same order
    d = ring3(12)
    assert (d["splitK"], d["kPerSlice"]) == (12, 7 * 32), d
    assert d["Kdigits"] == digits_in_order_of(ext, "dcba", "ebcd", "dbc"), d


def kept(env, monkeypatch, want, *args, **kw):
    d, old = both_orders(env, monkeypatch, *args, **kw)
    assert d == old, (d, old)
    if want is not None:
        assert d["Kdigits"] == want, d
    return d


def test_plans_that_keep_their_digits(env, monkeypatch):
    ct, ops, h = env
    # contraction.cu default C[m,u,n,v] = A[m,h,k,n] B[u,k,v,h]: neither operand K-contiguous; D's fastest mode is in A, so B plays
    # kernel-A and the order is that of its strides (k, h)
    e = dict(m=96, n=96, u=96, v=64, h=64, k=64)
    d = kept(env, monkeypatch, [[64, 96, 6144], [64, 393216, 96]], e, "mhkn", "ukvh", "munv")
    assert d["family"] == 0 and d["swapped"] == 1 and d["Kdigits"] == digits_in_order_of(e, "mhkn", "ukvh", "kh", swapped=True), d
    # 'km,kn': one contracted mode, neither operand K-contiguous
    g = dict(m=4096, n=4096, k=4096)
    kept(env, monkeypatch, [[4096, 4096, 4096]], g, "mk", "nk", "nm")
    # one contracted mode, K-contiguous in A only, split-K on the streaming kernel: nothing to order
    g1 = dict(m=96, n=96, k=262144)
    d = kept(env, monkeypatch, [[262144, 1, 96]], g1, "km", "nk", "nm")
    assert d["kname"] == "gett_f32_stream_kernel" and d["splitK"] > 1, d
    # both operands K-contiguous (the headline with B stored d-fastest): A's order, which is also B's here
    d = kept(env, monkeypatch, None, HEAD, "dcba", "dcbe", "ea")
    assert d["kname"] == "gett_f32_stream_kernel" and d["splitK"] > 1 and (d["layA"], d["layB"]) == (1, 1), d
    # ... and with B's upper modes the other way round: still A's order
    kept(env, monkeypatch, digits_in_order_of(HEAD, "dcba", "dbce", "dcb"), HEAD, "dcba", "dbce", "ea")
    # ... and K-contiguous in DIFFERENT modes (A in d, B in c): both are K-contiguous, A's order (on the operands as they lie:
    # without the switch the planner copies B first, and the copy's plan has fused digits)
    monkeypatch.setenv("CUTENSOR_AMD_REPACK", "0")
    kept(env, monkeypatch, digits_in_order_of(HEAD, "dcba", "cebd", "dcb"), HEAD, "dcba", "cebd", "ea")
    monkeypatch.delenv("CUTENSOR_AMD_REPACK")
    # 16-bit and fp64 data of the headline equation
    for dtype in (ct.R_16BF, ct.R_64F):
        d = kept(env, monkeypatch, [[64, 1, 393216], [64, 64, 6144], [64, 4096, 96]], HEAD, "dcba", "ebcd", "ea", dtype=dtype)
        assert d["family"] != 0, d
    # an fp32 streaming plan without split: many output tiles, A K-contiguous over three contracted modes
    big = dict(a=3072, e=3072, d=64, c=4, b=4)
    d = kept(env, monkeypatch, digits_in_order_of(big, "dcba", "ebcd", "dcb"), big, "dcba", "ebcd", "ea")
    assert d["kname"] == "gett_f32_stream_kernel" and d["splitK"] == 1, d
    # more than one output tile, split: the flat entry does not cover it, the order stays
    two = dict(HEAD, a=192)
    d = kept(env, monkeypatch, [[64, 1, 393216], [64, 64, 6144], [64, 4096, 96]], two, "dcba", "ebcd", "ea")
    assert d["kname"] == "gett_f32_stream_kernel" and d["splitK"] > 1 and d["blocks"] == 2 * d["splitK"], d


def test_explicit_orders_of_the_hook_still_apply(env, monkeypatch):
    monkeypatch.setenv("CUTENSOR_AMD_KORDER", "d,c:16,b,c")
    d = describe(env, HEAD, "dcba", "ebcd", "ea")
    assert d["Kdigits"] == [[64, 1, 393216], [16, 64, 6144], [64, 4096, 96], [4, 1024, 98304]], d
    monkeypatch.setenv("CUTENSOR_AMD_KORDER", "B")
    d = describe(env, HEAD, "dcba", "ebcd", "ea")
    assert [x[2] for x in d["Kdigits"]] == [96, 6144, 393216], d
