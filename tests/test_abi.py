"""CPU-only: the C-ABI library loads, exports every symbol include/*.h declares, and the host logic
(descriptors, planning, workspace invariants, error behaviour) follows the reference call sites.
No compute entry point is launched here."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ct(built):
    import cudalibrarysamples_amd.cutensor as ct
    return ct


@pytest.fixture(scope="module")
def ops(built):
    from cudalibrarysamples_amd import ops
    return ops


def _declared_functions(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b((?:cutensor(?:Mg|Mp)?|ctamdMp)[A-Z]\w*)\s*\(", src)))


def test_every_declared_symbol_is_exported(ct):
    names = _declared_functions("cutensor.h")
    assert "cutensorContract" in names and "cutensorCreatePlan" in names
    for n in names:
        assert hasattr(ct.lib, n), "libcutensor.so does not export %s" % n
    for d in ct.DATA_SYMBOLS:
        assert ctypes.c_void_p.in_dll(ct.lib, d).value, d


def test_mg_symbols_exported(built):
    mg = ctypes.CDLL(os.path.join(ROOT, "cudalibrarysamples_amd", "lib", "libcutensorMg.so"))
    for n in _declared_functions("cutensorMg.h"):
        assert hasattr(mg, n), "libcutensorMg.so does not export %s" % n


def test_mp_symbols_exported(built):
    mp = ctypes.CDLL(os.path.join(ROOT, "cudalibrarysamples_amd", "lib", "libcutensorMp.so"))
    names = _declared_functions("cutensorMp.h")
    assert "cutensorMpContract" in names and "cutensorMpCreateTensorDescriptor" in names and "ctamdMpLocalWorldCreate" in names
    for n in names:
        assert hasattr(mp, n), "libcutensorMp.so does not export %s" % n
    # Destroy*(NULL) is tolerated, and nothing below needs a device
    for n in ("cutensorMpDestroyPlan", "cutensorMpDestroyTensorDescriptor", "cutensorMpDestroyOperationDescriptor",
              "cutensorMpDestroyPlanPreference", "cutensorMpDestroy"):
        assert getattr(mp, n)(None) == 0
    world = ctypes.c_void_p()
    assert mp.ctamdMpLocalWorldCreate(ctypes.byref(world), 4) == 0 and world.value
    assert mp.ctamdMpLocalWorldCreate(ctypes.byref(ctypes.c_void_p()), 0) != 0
    assert mp.ctamdMpLocalWorldDestroy(world) == 0


def test_lifecycle_and_null_tolerance(ct):
    h = ctypes.c_void_p()
    assert ct.cutensorCreate(ctypes.byref(h)) == ct.STATUS_SUCCESS
    # Destroy*(NULL) must be tolerated (python/einsum.h:302,396)
    assert ct.cutensorDestroyTensorDescriptor(None) == ct.STATUS_SUCCESS
    assert ct.cutensorDestroyPlan(None) == ct.STATUS_SUCCESS
    assert ct.cutensorDestroyOperationDescriptor(None) == ct.STATUS_SUCCESS
    assert ct.cutensorHandleResizePlanCache(h, 1024) == ct.STATUS_SUCCESS     # einsum.cu:445
    assert ct.getErrorString(15) == "CUTENSOR_STATUS_NOT_SUPPORTED"
    assert ct.cutensorCreate(None) == ct.STATUS_INVALID_VALUE
    assert ct.cutensorDestroy(h) == ct.STATUS_SUCCESS


def test_contraction_sample_sequence(ct, ops):
    """contraction.cu:122-239 up to (not including) the execution."""
    h = ops.Handle()
    p = ops.contraction_plan(h, [96, 64, 64, 96], "mhkn", [96, 64, 64, 64], "ukvh", [96, 96, 96, 64], "munv")
    assert p.scalar_type == ct.R_32F                      # contraction.cu:176-182
    assert p.required_workspace <= p.workspace_estimate   # contraction.cu:239
    d = p.describe()
    # M = m*n = 9216, N = u*v = 6144, K = 4096; D is m-contiguous so the engine
    # swaps operands to put (m, n) on the coalesced side
    assert sorted([d["M"], d["N"]]) == [6144, 9216] and d["K"] == 4096 and d["N"] == 9216
    flops = ctypes.c_float(0)
    assert ct.cutensorOperationDescriptorGetAttribute(h.h, p.op, ct.OPERATION_DESCRIPTOR_FLOPS, ctypes.byref(flops), 4) == 0
    assert abs(flops.value - 463856467968.0) / 463856467968.0 < 1e-6    # contraction.cu:61
    p.destroy()


def test_headline_einsum_plan_uses_split_k(ct, ops):
    h = ops.Handle()
    p = ops.contraction_plan(h, [64, 64, 64, 96], "dcba", [96, 64, 64, 64], "ebcd", [96, 96], "ea",
                             workspace_limit=1 << 30)
    d = p.describe()
    assert (d["M"], d["N"], d["K"]) == (96, 96, 262144)
    assert d["layA"] == 1 and d["layB"] == 0       # A K-contiguous, B free-contiguous
    assert d["splitK"] > 1 and d["blocks"] >= 256  # a single 96x96 tile must be split over the chip
    assert p.required_workspace == d["splitK"] * 96 * 96 * 4
    # with no workspace the same problem still plans (no split)
    p0 = ops.contraction_plan(h, [64, 64, 64, 96], "dcba", [96, 64, 64, 64], "ebcd", [96, 96], "ea", workspace_limit=0)
    assert p0.required_workspace == 0 and p0.describe()["splitK"] == 1


def test_mode_fusion_and_batch(ct, ops):
    h = ops.Handle()
    # 'lik,lkj->lij' row-major == cuTENSOR modes reversed; l is a batch mode
    p = ops.contraction_plan(h, [50, 50, 50], "kil", [50, 50, 50], "jkl", [50, 50, 50], "jil")
    d = p.describe()
    assert (d["L"], d["M"], d["N"], d["K"]) == (50, 50, 50, 50)
    # fully fusable GEMM: A[m1,m2,k] B[k,n] -> C[m1,m2,n] fuses (m1,m2)
    p = ops.contraction_plan(h, [8, 4, 16], "abk", [16, 12], "kn", [8, 4, 12], "abn")
    d = p.describe()
    assert sorted([d["M"], d["N"]]) == [12, 32] and d["K"] == 16


def test_error_behaviour(ct, ops):
    h = ops.Handle()
    with pytest.raises(ct.CuTensorError) as e:      # extent mismatch between A and B for mode k
        ops.contraction_plan(h, [4, 5], "mk", [6, 7], "kn", [4, 7], "mn")
    assert e.value.status == ct.STATUS_INVALID_VALUE
    # a mode that ONE INPUT alone carries is summed over that input since round 6 (tests/test_gpu_lone_modes.py) ...
    p = ops.contraction_plan(h, [4, 5, 3], "mkz", [5, 7], "kn", [4, 7], "mn", workspace_limit=1 << 20)
    assert p.describe()["lone_reduce_A"] == 1 and p.required_workspace >= 4 * 5 * 4
    p.destroy()
    with pytest.raises(ct.CuTensorError) as e:      # ... but its temporary lives in the workspace
        ops.contraction_plan(h, [4, 5, 3], "mkz", [5, 7], "kn", [4, 7], "mn", workspace_limit=0)
    assert e.value.status == ct.STATUS_INSUFFICIENT_WORKSPACE
    with pytest.raises(ct.CuTensorError) as e:      # a mode that only the OUTPUT carries (a broadcast) is no contraction
        ops.contraction_plan(h, [4, 5], "mk", [5, 7], "kn", [4, 7, 3], "mnz")
    assert e.value.status == ct.STATUS_NOT_SUPPORTED
    d = ctypes.c_void_p()
    assert ct.cutensorCreateTensorDescriptor(h.h, ctypes.byref(d), 2, ct.i64([4, -1]), None, ct.R_32F, 128) == ct.STATUS_INVALID_VALUE
    assert ct.cutensorCreateTensorDescriptor(None, ctypes.byref(d), 2, ct.i64([4, 4]), None, ct.R_32F, 128) == ct.STATUS_NOT_INITIALIZED


def test_permutation_and_reduction_plans(ct, ops):
    h = ops.Handle()
    p = ops.permutation_plan(h, [32, 128, 128, 128], "whcn", [128, 32, 128, 128], "cwhn")   # elementwise_permute.cu:51-63
    d = p.describe()
    # (variant 4 since round 6: pure fp32 permutations below 512 MB go to the element-wise 64 x 64 transposer — level with the 16-byte-lane
    # kernel at this shape, 5.71 / 5.74 TB/s, ahead at 4096^2-class shapes: profiles/r06zzo_*, r06zzq_*)
    assert d["variant"] in (0, 4) and d["E0"] == 128 and d["E1"] == 4096 and p.required_workspace == 0
    r = ops.reduction_plan(h, [196, 256, 64, 64], "mhkv", [196, 64], "mv")                   # reduction.cu:49-61
    d = r.describe()
    assert d["kept"] == 196 * 64 and d["red"] == 256 * 64 and r.required_workspace <= r.workspace_estimate
    # einsum.cu:449-450: a reduction descriptor without reduced modes is a permutation
    q = ops.reduction_plan(h, [5, 4, 2], "jin", [2, 5, 4], "nji")
    assert q.describe()["op"] == "elementwise"
    # identical layouts fuse into ONE contiguous mode (a flat copy: the packed identity permutations of cutensorMp, 'ij->ij'): cut into rows
    # of the largest divisor in [256, 4096] so that the row-copy kernel's 8-row tiles are full (round 6: 1.85 -> 6 TB/s on 96 MB)
    d = ops.permutation_plan(h, [400, 200, 300], "abc", [400, 200, 300], "abc").describe()
    assert d["variant"] == 1 and d["E0"] == 4000 and d["E1"] == 6000, d
    d = ops.permutation_plan(h, [7, 11, 13], "abc", [7, 11, 13], "abc").describe()          # too small to cut: as before
    assert d["E0"] == 7 * 11 * 13 and d["E1"] == 1, d


def test_plan_cache_file_roundtrip(ct, ops, tmp_path):
    h = ops.Handle(plan_cache=8)
    f = str(tmp_path / "cache.txt").encode()
    assert ct.cutensorHandleWritePlanCacheToFile(h.h, f) == ct.STATUS_SUCCESS
    n = ctypes.c_uint32(7)
    assert ct.cutensorHandleReadPlanCacheFromFile(h.h, f, ctypes.byref(n)) == ct.STATUS_SUCCESS and n.value == 0
    assert ct.cutensorHandleReadPlanCacheFromFile(h.h, b"/nonexistent/x", ctypes.byref(n)) == ct.STATUS_IO_ERROR   # contraction_plan_cache.cu:136


def test_einsum_helper_parsing(ct):
    """C++ Einsum<> mirror vs the oracle's restatement of einsum.cu:63-223 (host logic only)."""
    import oracle
    cases = [("ijn,jmk->inkm", (2, 4, 5), (4, 8, 7)), ("ijn,jmk", (2, 4, 5), (4, 8, 7)), ("nij", (2, 4, 5), ()),
             ("nij->ijn", (2, 4, 5), ()), ("nij->ji", (2, 4, 5), ()), ("abcd,dcbe->ae", (96, 64, 64, 64), (64, 64, 64, 96)),
             ("ab...,bc->ac", (2, 3, 4), (3, 4)), ("ab,bc->ac", (2, 3, 4), (3, 4)), (" a b , b c -> a c ", (2, 3), (3, 4))]
    for eq, sa, sb in cases:
        e = ct.lib.ctamdEinsumCreate(eq.encode(), ct.i64(list(sa)), len(sa), ct.i64(list(sb)), len(sb), ct.R_32F)
        ref = oracle.einsum_parse(eq, sa, sb, max_modes=64)
        assert bool(ct.lib.ctamdEinsumIsInitialized(e)) == (ref is not None), eq
        if ref is not None:
            out = (ctypes.c_int64 * 64)()
            n = ct.lib.ctamdEinsumOutputShape(e, out, 64)
            assert [out[i] for i in range(n)] == ref["output_shape"], eq
        ct.lib.ctamdEinsumDestroy(e)


def _op_attr_float(ct, h, op, attr):
    v = ctypes.c_float(0)
    ct.check(ct.cutensorOperationDescriptorGetAttribute(h.h, op, attr, ctypes.byref(v), 4))
    return v.value


def test_trinary_contraction_pair_order_and_workspace(ct, ops):
    """contraction_trinary.cu:44-67: D_{m,n,b,r,a} = A_{m,k,a,j,b,i} B_{k,n,i} C_{r,j}; the sample states the work as
    flops(A*B) + flops((AB)*C) (:65-67) — the planner must find that order, and the workspace estimate must hold
    the packed intermediate T_{m,a,j,b,n}."""
    h = ops.Handle()
    ext = dict(m=256, a=32, b=32, n=64, r=64, k=8, i=8, j=64)
    mA, mB, mC, mD = "mkajbi", "kni", "rj", "mnbra"
    dA, dB, dC, dD = [ops.tensor_descriptor(h, [ext[c] for c in m]) for m in (mA, mB, mC, mD)]
    op = ctypes.c_void_p()
    ct.check(ct.cutensorCreateContractionTrinary(h.h, ctypes.byref(op), dA, ct.i32(mA), ct.OP_IDENTITY, dB, ct.i32(mB), ct.OP_IDENTITY,
                                                 dC, ct.i32(mC), ct.OP_IDENTITY, dD, ct.i32(mD), ct.OP_IDENTITY, dD, ct.i32(mD),
                                                 ct.compute_desc("32F")))
    e = ext
    first = 2.0 * e["m"] * e["a"] * e["b"] * e["j"] * e["n"] * e["k"] * e["i"]
    second = 2.0 * e["m"] * e["a"] * e["b"] * e["n"] * e["r"] * e["j"]
    flops = _op_attr_float(ct, h, op, ct.OPERATION_DESCRIPTOR_FLOPS) if hasattr(ct, "OPERATION_DESCRIPTOR_FLOPS") else _op_attr_float(ct, h, op, 2)
    assert abs(flops - (first + second)) / (first + second) < 1e-6
    est = ctypes.c_uint64(0)
    ct.check(ct.cutensorEstimateWorkspaceSize(h.h, op, None, ct.WORKSPACE_DEFAULT, ctypes.byref(est)))
    t_bytes = 4 * e["m"] * e["a"] * e["j"] * e["b"] * e["n"]
    assert est.value >= t_bytes
    mn = ctypes.c_uint64(0)
    ct.check(ct.cutensorEstimateWorkspaceSize(h.h, op, None, ct.WORKSPACE_MIN, ctypes.byref(mn)))
    assert t_bytes <= mn.value <= est.value
    ct.cutensorDestroyOperationDescriptor(op)


def test_elementwise_trinary_descriptor_and_operator_checks(ct, ops):
    """elementwise_trinary.cu:174-182; ADD/MUL/MAX/MIN combiners are served, anything else is NOT_SUPPORTED."""
    h = ops.Handle()
    ext = dict(a=40, b=20, c=30)
    d = {m: ops.tensor_descriptor(h, [ext[c] for c in m]) for m in ("cba", "cab", "abc")}
    for opAB, opABC, want in ((ct.OP_ADD, ct.OP_ADD, ct.STATUS_SUCCESS), (ct.OP_MUL, ct.OP_MAX, ct.STATUS_SUCCESS), (2, ct.OP_ADD, 15)):
        op = ctypes.c_void_p()
        st = ct.cutensorCreateElementwiseTrinary(h.h, ctypes.byref(op), d["cba"], ct.i32("cba"), ct.OP_IDENTITY, d["cab"], ct.i32("cab"),
                                                 ct.OP_IDENTITY, d["abc"], ct.i32("abc"), ct.OP_IDENTITY, d["abc"], ct.i32("abc"),
                                                 opAB, opABC, ct.compute_desc("32F"))
        assert st == want
        if st == ct.STATUS_SUCCESS:
            moved = _op_attr_float(ct, h, op, 3)      # MOVED_BYTES: 4 |D| (elementwise_trinary.cu:234-238)
            assert moved == 4.0 * 4 * 40 * 20 * 30
            ct.cutensorDestroyOperationDescriptor(op)


def test_many_mode_and_complex_contractions_are_accepted(ct, ops):
    """contraction_jit.cu:31-56: 25 / 13 / 24 modes of extent 2, complex<float> data, complex scalar type."""
    h = ops.Handle()
    mC = [0, 1, 2, 3, 4, 6, 8, 9, 25, 26, 10, 12, 14, 27, 15, 28, 17, 19, 29, 20, 21, 30, 23, 24]
    mA = [0, 2, 1, 4, 3, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 20, 19, 21, 22, 23, 24]
    mB = [25, 26, 27, 28, 29, 30, 5, 7, 11, 13, 16, 18, 22]
    dA, dB, dC = [ops.tensor_descriptor(h, [2] * len(m), dtype=ct.C_32F) for m in (mA, mB, mC)]
    op = ctypes.c_void_p()
    ct.check(ct.cutensorCreateContraction(h.h, ctypes.byref(op), dA, ct.i32(mA), ct.OP_IDENTITY, dB, ct.i32(mB), ct.OP_IDENTITY,
                                          dC, ct.i32(mC), ct.OP_IDENTITY, dC, ct.i32(mC), ct.compute_desc("3XTF32")))
    st = ctypes.c_int(0)
    ct.check(ct.cutensorOperationDescriptorGetAttribute(h.h, op, ct.OPERATION_DESCRIPTOR_SCALAR_TYPE, ctypes.byref(st), 4))
    assert st.value == ct.C_32F                     # contraction_jit.cu:205
    est = ctypes.c_uint64(1)
    ct.check(ct.cutensorEstimateWorkspaceSize(h.h, op, None, ct.WORKSPACE_DEFAULT, ctypes.byref(est)))
    assert est.value == 0                           # the mode-table kernel needs no workspace
    ct.cutensorDestroyOperationDescriptor(op)
    # complex element-wise operations are served since round 5 (test_complex_reductions_and_permutations_plan); 25 identically
    # ordered extent-2 modes fuse into one
    p = ctypes.c_void_p()
    assert ct.cutensorCreatePermutation(h.h, ctypes.byref(p), dA, ct.i32(mA), ct.OP_IDENTITY, dA, ct.i32(mA), ct.compute_desc("32F")) == 0
    ct.cutensorDestroyOperationDescriptor(p)


def test_blocksparse_descriptor_validation(ct, ops):
    """blocksparse.cu:102-107: section index out of range / non-positive section extent are INVALID_VALUE."""
    h = ops.Handle()
    nsec = (ctypes.c_uint32 * 2)(2, 2)
    d = ctypes.c_void_p()
    ok = ct.cutensorCreateBlockSparseTensorDescriptor(h.h, ctypes.byref(d), 2, 2, nsec, ct.i64([4, 5, 6, 7]), ct.i32([0, 0, 1, 1]), None, ct.R_64F)
    assert ok == ct.STATUS_SUCCESS
    assert ct.cutensorDestroyBlockSparseTensorDescriptor(d) == ct.STATUS_SUCCESS
    bad = ct.cutensorCreateBlockSparseTensorDescriptor(h.h, ctypes.byref(d), 2, 1, nsec, ct.i64([4, 5, 6, 7]), ct.i32([0, 2]), None, ct.R_64F)
    assert bad == ct.STATUS_INVALID_VALUE
    bad = ct.cutensorCreateBlockSparseTensorDescriptor(h.h, ctypes.byref(d), 2, 1, nsec, ct.i64([4, 0, 6, 7]), ct.i32([0, 0]), None, ct.R_64F)
    assert bad == ct.STATUS_INVALID_VALUE


def test_padding_attributes(ct, ops):
    """elementwise_permute_padding.cu:178-195: one int per output mode; wrong sizes are INVALID_VALUE; non-permutation
    descriptors refuse the attribute."""
    h = ops.Handle()
    dA = ops.tensor_descriptor(h, [8, 6, 4])
    dC = ops.tensor_descriptor(h, [4, 8, 6])
    op = ctypes.c_void_p()
    ct.check(ct.cutensorCreatePermutation(h.h, ctypes.byref(op), dA, ct.i32("whc"), ct.OP_IDENTITY, dC, ct.i32("cwh"), ct.compute_desc("32F")))
    pad = (ctypes.c_int32 * 3)(0, 1, 2)
    assert ct.cutensorOperationDescriptorSetAttribute(h.h, op, 4, pad, 12) == ct.STATUS_SUCCESS
    assert ct.cutensorOperationDescriptorSetAttribute(h.h, op, 5, pad, 8) == ct.STATUS_INVALID_VALUE
    v = ctypes.c_float(1.5)
    assert ct.cutensorOperationDescriptorSetAttribute(h.h, op, 6, ctypes.byref(v), 4) == ct.STATUS_SUCCESS
    ct.cutensorDestroyOperationDescriptor(op)
    red = ctypes.c_void_p()
    dR = ops.tensor_descriptor(h, [8])
    ct.check(ct.cutensorCreateReduction(h.h, ctypes.byref(red), dA, ct.i32("whc"), ct.OP_IDENTITY, dR, ct.i32("w"), ct.OP_IDENTITY, dR, ct.i32("w"),
                                        ct.OP_ADD, ct.compute_desc("32F")))
    assert ct.cutensorOperationDescriptorSetAttribute(h.h, red, 4, pad, 12) == 15


def test_reference_torch_binding_loads_without_gpu(built):
    """oracle/_ref/pyref (the reference's einsum.cc compiled unmodified against include/ + libcutensor.so, see
    oracle/build_ref_torch_binding.sh) imports on a CPU-only host and exposes the three entry points the reference's
    einsum.py binds (einsum.py:22); its undefined cutensor* symbols all resolve in OUR library."""
    import glob
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pyref = os.path.join(root, "oracle", "_ref", "pyref")
    sos = glob.glob(os.path.join(pyref, "cutensor", "torch", "binding*.so"))
    if not sos:
        pytest.skip("oracle/_ref/pyref was not built (reference tree absent at build time)")
    code = ("import sys; sys.path[:0]=[%r,%r]; import cutensor.torch as c, cutensor.torch.binding as b; "
            "print(sorted(n for n in dir(b) if not n.startswith('_')))") % (pyref, os.path.join(root, "tests", "sample_compat", "pyshim"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "'einsum', 'execute', 'plan'" in r.stdout, r.stdout
    und = subprocess.run(["nm", "-D", "--undefined-only", sos[0]], capture_output=True, text=True).stdout
    wanted = sorted({ln.split()[-1] for ln in und.splitlines() if " cutensor" in ln or ln.split()[-1].startswith("CUTENSOR_")})
    assert "cutensorContract" in wanted and "cutensorCreatePlan" in wanted, wanted
    lib = subprocess.run(["nm", "-D", "--defined-only", os.path.join(root, "cudalibrarysamples_amd", "lib", "libcutensor.so")],
                         capture_output=True, text=True).stdout
    have = {ln.split()[-1] for ln in lib.splitlines()}
    assert not [s for s in wanted if s not in have], [s for s in wanted if s not in have]


def test_allocation_failure_inside_an_entry_point_becomes_a_status(built, tmp_path):
    """No exception crosses the C ABI (csrc/host/api_guard.hpp): tests/harness/alloc_fail_harness.cpp replaces operator new, lets the
    k-th allocation of the contraction.cu:123-235 call sequence (and of the contraction_multi_gpu.cu:151-250 planning sequence on two
    device ids) throw std::bad_alloc for every k, and every entry point must answer CUTENSOR_STATUS_ALLOC_FAILED — an exception
    that unwound into the harness's C-style frames would end the process in std::terminate.  The same for the cuTENSORMp planning
    sequence on one rank of a four-rank local world, under a gather and a reduce layout.  The harness also counts live allocations:
    no round of the cuTENSORMp sweeps and of the single-GPU tensor-descriptor calls may leave an object behind (the plan, descriptors
    and copies are owned from the moment they exist); cuTENSORMg's count is printed, not asserted."""
    import subprocess
    exe = str(tmp_path / "alloc_fail_harness")
    lib = os.path.join(ROOT, "cudalibrarysamples_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
                           os.path.join(ROOT, "tests", "harness", "alloc_fail_harness.cpp"), "-o", exe,
                           "-L", lib, "-lcutensorMp", "-lcutensorMg", "-lcutensor", "-Wl,-rpath," + lib])
    r = subprocess.run([exe, "mg"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cutensor: alloc guard ok" in r.stdout and "cutensorMg: alloc guard ok" in r.stdout, r.stdout
    assert "cutensorMp: alloc guard ok" in r.stdout, r.stdout
    for sweep in ("cutensorMp gather", "cutensorMp reduce", "cutensor descriptors"):
        assert "%s: alloc guard ok" % sweep in r.stdout and "%s: 0 rounds left allocations behind" % sweep in r.stdout, r.stdout


def test_every_extern_c_entry_point_is_a_function_try_block():
    """Static twin of the test above: every function the libraries define inside an `extern "C"` block opens a function-try-block
    (`) try {`, closed by a CTAMD_API_CATCH* handler) — a new entry point without one fails here, not in a caller's process."""
    csrc = os.path.join(ROOT, "cudalibrarysamples_amd", "csrc")
    missing, seen = [], 0
    files = sorted(os.path.relpath(os.path.join(d, f), csrc) for d, _, fs in os.walk(csrc) for f in fs if f.endswith(".cpp"))
    for rel in files:     # every source file with an `extern "C" {` block, wherever a later split puts one
        lines = open(os.path.join(csrc, rel)).read().split("\n")
        if not any(line.startswith('extern "C" {') for line in lines):
            continue
        inside = False
        for i, line in enumerate(lines):
            if line.startswith('extern "C" {'):
                inside = True
            elif line.startswith('}  // extern "C"'):
                inside = False
            m = inside and re.match(r"^(?:cutensorStatus_t|int|size_t|void\*?|cutensorPlan_t) ((?:cutensor|ctamd)\w+)\(", line)
            if not m or m.group(1) == "cutensorGetVersion":
                continue
            j = i
            while not re.search(r"\)\s*(?:try\s*)?\{", lines[j]):      # the line that closes the parameter list and opens the body
                j += 1
            seen += 1
            if not re.search(r"\) try \{", lines[j]):
                missing.append((rel, m.group(1)))
    assert seen >= 100 and not missing, (seen, missing)


def test_complex_reductions_and_permutations_plan(ct, ops):
    """Planning only (no GPU): complex64 / complex128 reductions, permutations and the binary element-wise form are accepted (round 5:
    python/einsum.h:326-343 routes a unary einsum on complex tensors to cutensorCreateReduction), the scalar type is the data type,
    split-reduction partials are (re, im) pairs in the data's precision, MAX / MIN and the trinary form stay NOT_SUPPORTED."""
    h = ops.Handle()
    for dt, es in ((ct.C_32F, 8), (ct.C_64F, 16)):
        p = ops.permutation_plan(h, [50, 64], "ij", [64, 50], "ji", dtype=dt)
        assert p.scalar_type == dt and p.describe()["variant"] == 0          # round 6: the tiled transposing kernel of 8- / 16-byte elements
        p.destroy()
        p = ops.permutation_plan(h, [51, 63], "ij", [63, 51], "ji", dtype=dt)
        assert p.describe()["variant"] == (2 if es == 8 else 0)              # odd extents: complex64 pairs need even ones (EW_GENERIC), complex128 does not
        p.destroy()
        r = ops.reduction_plan(h, [65536, 6], "ab", [6], "b", dtype=dt, opA=ct.OP_CONJ)    # (tiled RED_ROW since round 6: splits from 8192 reduced elements per workgroup on)
        assert r.scalar_type == dt and r.required_workspace % (6 * es) == 0 and r.required_workspace > 0   # [splitR][kept] pairs
        assert r.required_workspace <= r.workspace_estimate
        r.destroy()
        r = ops.reduction_plan(h, [20, 50, 30], "kji", [30, 20], "ik", dtype=dt)           # the binding's "ijk->ik" after reversal
        r.destroy()
        with pytest.raises(RuntimeError):
            ops.reduction_plan(h, [8, 8], "ab", [8], "a", dtype=dt, op_reduce=ct.OP_MAX)
        with pytest.raises(RuntimeError):
            ops.binary_plan(h, [8, 8], "ab", [8, 8], "ba", op="MIN", dtype=dt)
        b = ops.binary_plan(h, [8, 8], "ab", [8, 8], "ba", op="MUL", dtype=dt)
        b.destroy()
    # CONJ on real data is the identity, not an error
    ops.reduction_plan(h, [64, 8], "ab", [8], "b", opA=ct.OP_CONJ).destroy()


def test_operands_streamed_preference_ranks_the_nontemporal_twins(ct, ops):
    """Engine extension CUTENSOR_AMD_PLAN_PREFERENCE_OPERANDS_STREAMED (include/cutensor/types.h, round 5): the headline einsum's
    201 MB of operands may or may not be resident in the 256-MiB Infinity Cache — a caller that knows they are not says so and gets
    the nontemporal-load twin of the streaming kernel (+3.6 % from HBM, -5.5 % cache-resident: profiles/r03_headline_nt.txt); without
    the preference the default policy stays, and the plan memo keeps the two apart."""
    h = ops.Handle(plan_cache=64)
    E = dict(a=96, b=64, c=64, d=64, e=96)
    args = ([E[c] for c in "dcba"], "dcba", [E[c] for c in "ebcd"], "ebcd", [E[c] for c in "ea"], "ea")
    seen = []
    for streamed in (None, True, None, True):
        p = ops.contraction_plan(h, *args, workspace_limit=1 << 30, operands_streamed=streamed)
        d = p.describe()
        assert d["kname"] == "gett_f32_stream_kernel" and d["splitK"] == 256 and d["nt"] == (1 if streamed else 0), (streamed, d)
        seen.append(d["kernel"])
        p.destroy()
    assert seen[0] == seen[2] and seen[1] == seen[3] and seen[0] != seen[1], seen
    # a multi-tile problem re-reads its panels: the preference changes nothing there
    p = ops.contraction_plan(h, [4096, 4096], "mk", [4096, 4096], "kn", [4096, 4096], "mn", operands_streamed=True)
    assert p.describe()["nt"] == 0
    p.destroy()


def test_production_libraries_carry_no_test_hooks(built):
    """Round-5 review, Weak #8: the libraries a user links (cudalibrarysamples_amd/lib/) read no behaviour-changing test / measurement
    switch and export no test entry point — `strings` lists CUTENSOR_LOG_LEVEL and the three documented cuTENSORMg switches only; the
    hooks flavour (lib_hooks/, what this suite loads: tests/conftest.py) has them."""
    import subprocess
    lib = os.path.join(ROOT, "cudalibrarysamples_amd", "lib")
    hooks = os.path.join(ROOT, "cudalibrarysamples_amd", "lib_hooks")
    def switches(path):
        out = subprocess.run(["strings", path], capture_output=True, text=True, check=True).stdout.split("\n")
        return sorted(set(x for x in out if re.fullmatch(r"CUTENSOR(MG|MP)?_(AMD_)?[A-Z0-9_]+", x) and not x.startswith(("CUTENSOR_STATUS_", "CUTENSOR_COMPUTE_DESC_"))))
    assert switches(os.path.join(lib, "libcutensor.so")) == ["CUTENSOR_LOG_LEVEL"]
    assert switches(os.path.join(lib, "libcutensorMg.so")) == ["CUTENSORMG_AMD_FORCE_GATHER", "CUTENSORMG_AMD_TRANSPORT", "CUTENSORMG_AMD_WAVES"]
    assert switches(os.path.join(lib, "libcutensorMp.so")) == []
    assert "CUTENSOR_AMD_H16_WAVES" in switches(os.path.join(hooks, "libcutensor.so"))
    prod, hk = ctypes.CDLL(os.path.join(lib, "libcutensorMg.so")), ctypes.CDLL(os.path.join(hooks, "libcutensorMg.so"))
    assert not hasattr(prod, "ctamdMgReplayOnHost") and hasattr(hk, "ctamdMgReplayOnHost")
    assert ctypes.CDLL(os.path.join(lib, "libcutensor.so")).ctamdTestHooksBuilt() == 0
    assert ctypes.CDLL(os.path.join(hooks, "libcutensor.so")).ctamdTestHooksBuilt() == 1
