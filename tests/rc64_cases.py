"""The case table of the mixed fp64 x complex128 contraction tests (tests/test_gpu_rc64_exact.py runs every case, tests/
test_rc64_planner_cpu.py plans every case without a GPU) — a helper module, not a conftest, in the style of tests/exact_cases.py.

One input is real fp64, the other one, C and D are complex128; the scalars are complex.  A case: id, extents, modes (the ABI's order,
fastest mode first), which of the caller's inputs is real, scalars, conjugations, pitch padding (A, B, D, C), the real operand's element
offset and descriptor alignment, the switches that reach its path and a predicate on the plan's description that proves the path ran.
Data: the draws of tests/exact_data.py — integers from {+-1, +-2, +-3} (complex: both parts), C from [-3, 3] — so that in fp64 every
product and every sum is exact in any order and the result is compared bit for bit with the CPU's complex128 einsum on the WIDENED real
operand (which is exact).  Every tensor lives in a NaN-filled buffer (exact_cases.Placed): D is NaN before the call, C is all NaN when
beta = 0 (it must not be read), guards and pitch padding are checked afterwards.  A case runs twice (two draws).  Cases whose switch the
library reads once per process run in a child: `python rc64_cases.py run ids...`."""
import os
import sys

import exact_cases as xc
import exact_data as xd
import workspace_cases as wc

KNAME = "gett_gen_rc64_kernel"
ELEM = 13                    # GEN_RC64 (csrc/kernels/params.h, kGenElemRC64)
ALPHA = complex(-2, 1)
BETAS = (0j, complex(0.5, -0.5), complex(1, 0))


class Case:
    def __init__(self, id, ext, modes, real, expect, alpha=ALPHA, beta=0j, conj=(False, False, False), pad=(0, 0, 0, 0), off=0, align_real=128,
                 env=None, group=None, ws_limit=1 << 28):
        self.id, self.ext, self.modes, self.real, self.expect = id, ext, modes, real, expect
        self.alpha, self.beta, self.conj, self.pad, self.off, self.align_real = alpha, beta, conj, pad, off, align_real
        self.env, self.group, self.ws_limit = dict(env or {}), group, ws_limit
        self.data_key = id

    def __repr__(self):
        return self.id

    def extents(self, m):
        return [self.ext[c] for c in m]

    def dtypes(self):
        """the data types of A, B (and of C / D: complex128)"""
        return ("float64", "complex128") if self.real == 0 else ("complex128", "float64")


def tiled(real, vec=None, split=None, side=None):
    """one launch of the mixed kernel (+ the fold): the new kname and element, the right "real"; optionally the real operand's width, whether K
    is split, and which KERNEL operand the real tensor became (real ^ swapped)"""
    def ok(d):
        if d.get("family") != 2 or d.get("kname") != KNAME or d.get("elem") != ELEM or d.get("real") != real:
            return False
        if any(d.get(k) for k in ("peel_launches", "lone_reduce_A", "lone_reduce_B", "repack_A", "repack_B")):
            return False
        if vec is not None and d.get("vec") != vec:
            return False
        if side is not None and (d.get("real") ^ d.get("swapped")) != side:
            return False
        return split is None or (d.get("splitK", 1) > 1) == split
    return ok


CASES = []


def add(*a, **kw):
    c = Case(*a, **kw)
    assert all(c.id != o.id for o in CASES), c.id
    CASES.append(c)
    return c


# ragged edges: 63 x 45 against the 64-wide tile, k = 37 against the K-tile of 8 — four layouts x the real tensor as A / as B x D contiguous in
# n / in m: the view swaps the operands for the latter, so the real tensor runs as kernel-A AND as kernel-B on every layout (side = real ^ swapped)
RAGGED = dict(m=63, n=45, k=37)
CONJS = ((False, False, False), (True, False, False), (False, True, False), (False, False, True), (True, True, True))
_n = 0
for mA, mB in xc.LAYOUTS:
    for real in (0, 1):
        for mC in ("nm", "mn"):
            swapped = mC == "mn"       # D's stride-1 mode lives in A: A plays kernel-B
            add("ragged_%s_real%s_%s" % (xc.LNAME[(mA, mB)], "AB"[real], mC), RAGGED, (mA, mB, mC), real, tiled(real, side=real ^ int(swapped)),
                beta=BETAS[_n % 3], conj=CONJS[_n % 5])
            _n += 1
# vector width: even extents and an aligned real operand -> 16-byte lanes; the same at element offset 1 -> 8-byte gathers
VEC = dict(m=64, n=48, k=40)
for mA, mB in xc.LAYOUTS:
    for real in (0, 1):
        L = "%s_real%s" % (xc.LNAME[(mA, mB)], "AB"[real])
        add("vec2_" + L, VEC, (mA, mB, "nm"), real, tiled(real, vec=2), beta=BETAS[(_n + real) % 3])
        add("vec1_" + L, VEC, (mA, mB, "nm"), real, tiled(real, vec=1), off=1, align_real=8, beta=BETAS[(_n + real + 1) % 3])
    _n += 1
# unfused modes (mixed-radix row clamp and epilogue offsets), padded pitches (C's differs from D's), two batches; k = 517: the planner splits
for real in (0, 1):
    for bi, beta in enumerate(BETAS):
        add("unfused_real%s_beta%d" % ("AB"[real], bi), xc.UNFUSED, xc.UNFUSED_MODES, real, tiled(real, split=False), beta=beta, pad=xc.UNFUSED_PAD,
            conj=CONJS[(bi + real) % 5])
    add("unfused_long_real%s" % "AB"[real], xc.UNFUSED_LONG, xc.UNFUSED_MODES, real, tiled(real, split=True), beta=BETAS[1 + real], pad=xc.UNFUSED_PAD,
        conj=(False, False, bool(real)))
# exactly one K-tile, and a single k
for k in (8, 1):
    for real in (0, 1):
        add("k%d_real%s" % (k, "AB"[real]), dict(m=63, n=45, k=k), ("mk", "nk", "nm"), real, tiled(real), beta=BETAS[real])
# CONJ on the real operand is the identity: the same problem with and without it (the results are compared with one reference either way)
for real in (0, 1):
    cj = (real == 0, real == 1, False)
    add("conj_on_real_%s" % "AB"[real], RAGGED, ("km", "kn", "nm"), real, tiled(real), beta=BETAS[1], conj=cj)
# lone mode 'ijk,kl->il' (reversed): j summed out of the real operand (a real fp64 reduction into a real temporary), and out of the complex one
add("lone_on_real", wc.LONE, ("kji", "lk", "li"), 0, wc._lone(1, 0, lambda d: d.get("kname") == KNAME and d.get("real") == 0), beta=BETAS[1])
add("lone_on_complex", wc.LONE, ("kji", "lk", "li"), 1, wc._lone(1, 0, lambda d: d.get("kname") == KNAME and d.get("real") == 1), beta=BETAS[2],
    conj=(True, False, False))
# wide views: peeled into launches of the mixed inner plan; with CUTENSOR_AMD_PEEL=0 the mode-table kernel reads the real operand as reals
PEEL_MODES = ("paqbrcsdte", "xpyqzrst", "abxcydze")
add("peeled_realA", wc.PEEL, PEEL_MODES, 0, lambda d: d.get("peel_launches", 0) >= 2 and d.get("kname") == KNAME and d.get("real") == 0, beta=BETAS[2],
    ws_limit=1 << 24)
add("peeled_realB", wc.PEEL, PEEL_MODES, 1, lambda d: d.get("peel_launches", 0) >= 2 and d.get("kname") == KNAME and d.get("real") == 1, beta=BETAS[1],
    ws_limit=1 << 24, conj=(True, False, True))
for real in (0, 1):
    add("mode_table_real%s" % "AB"[real], wc.PEEL, PEEL_MODES, real, lambda d, real=real: d.get("kname") == "gett_wide_kernel" and d.get("real") == real,
        env={"CUTENSOR_AMD_PEEL": "0"}, group="peel0", beta=BETAS[1 + real], conj=(bool(real), not real, False), ws_limit=1 << 24)

BY_ID = {c.id: c for c in CASES}
IN_PROCESS = [c.id for c in CASES if c.group is None]
GROUPS = sorted({c.group for c in CASES if c.group})


# ---- data, plan, run -------------------------------------------------------------------------------------------------------------------
def make_inputs(case, swap):
    """(A, B, C) logical CPU tensors (dimensions in the order of the mode strings): exact_data's dense draws; the real operand float64"""
    import torch
    vals = (-3, -2, -1, 1, 2, 3)
    out = []
    for i, dt in enumerate(case.dtypes()):
        rng = xd._rng(case, swap, i)
        shape = case.extents(case.modes[i])
        re = torch.from_numpy(xd._dense(rng, shape, vals)).to(torch.float64)
        out.append(re if dt == "float64" else torch.complex(re, torch.from_numpy(xd._dense(rng, shape, vals)).to(torch.float64)))
    rc = xd._rng(case, swap, 2)
    shape = case.extents(case.modes[2])
    c = torch.complex(torch.from_numpy(rc.integers(-3, 4, size=shape)).to(torch.float64), torch.from_numpy(rc.integers(-3, 4, size=shape)).to(torch.float64))
    return out[0], out[1], c


def reference(case, A, B, C):
    """the CPU's complex128 result with the real operand widened (exact); CONJ on the real operand is the identity by definition"""
    import torch
    a, b = A.to(torch.complex128), B.to(torch.complex128)
    a = a.conj() if case.conj[0] else a
    b = b.conj() if case.conj[1] else b
    ref = case.alpha * torch.einsum("%s,%s->%s" % case.modes, a, b)
    if case.beta != 0:
        ref = ref + case.beta * (C.conj() if case.conj[2] else C)
    return ref


def make_plan(ct, ops, h, case):
    import guarded as gd
    e, m = case.extents, case.modes
    stA, stB, stD, stC = (gd.packed_strides(e(m[i]), case.pad[j]) for i, j in ((0, 0), (1, 1), (2, 2), (2, 3)))
    conj = [ct.OP_CONJ if c else ct.OP_IDENTITY for c in case.conj]
    # one descriptor alignment for all four tensors: what the real operand's placement admits (complex128 elements need 16)
    align = 128 if case.align_real == 128 else 16
    if case.align_real == 128:
        return ops.contraction_plan(h, e(m[0]), m[0], e(m[1]), m[1], e(m[2]), m[2], dtype=ct.C_64F, strideA=stA, strideB=stB, strideC=stC, strideD=stD,
                                    alignment=align, opA=conj[0], opB=conj[1], opC=conj[2], workspace_limit=case.ws_limit,
                                    **{"dtypeA" if case.real == 0 else "dtypeB": ct.R_64F})
    # the real operand at an odd element offset: its own descriptor says 8 bytes
    import ctypes
    d = [ops.tensor_descriptor(h, e(m[0]), stA, ct.R_64F if case.real == 0 else ct.C_64F, case.align_real if case.real == 0 else 16),
         ops.tensor_descriptor(h, e(m[1]), stB, ct.R_64F if case.real == 1 else ct.C_64F, case.align_real if case.real == 1 else 16),
         ops.tensor_descriptor(h, e(m[2]), stC, ct.C_64F, 16), ops.tensor_descriptor(h, e(m[2]), stD, ct.C_64F, 16)]
    op = ctypes.c_void_p()
    st = ct.cutensorCreateContraction(h.h, ctypes.byref(op), d[0], ct.i32(m[0]), conj[0], d[1], ct.i32(m[1]), conj[1], d[2], ct.i32(m[2]), conj[2],
                                      d[3], ct.i32(m[2]), ct.compute_desc("64F"))
    for x in d:
        ct.cutensorDestroyTensorDescriptor(x)
    ct.check(st)
    return ops.Plan(h, op, "contraction", ct.C_64F, workspace_limit=case.ws_limit)


def plan_path(ct, ops, h, case):
    """the case's plan is on the path the case covers (the planner needs no GPU); estimate >= required workspace"""
    with wc.hook_env(case):
        plan = make_plan(ct, ops, h, case)
    try:
        d = wc.describe(ct, plan)
        assert case.expect(d), "%s is off its path: %s" % (case.id, d.raw)
        assert plan.workspace_estimate >= plan.required_workspace, (case.id, plan.workspace_estimate, plan.required_workspace)
        assert plan.scalar_type == ct.C_64F
    finally:
        plan.destroy()
    return d


def run_case(ct, ops, h, case):
    import torch
    with wc.hook_env(case):
        plan = make_plan(ct, ops, h, case)
    try:
        d = wc.describe(ct, plan)
        assert case.expect(d), "%s is off its path: %s" % (case.id, d.raw)
        ws = torch.empty(max(plan.required_workspace, 256), dtype=torch.uint8, device="cuda")
        dts = case.dtypes()
        for swap in (False, True):
            A, B, C = make_inputs(case, swap)
            want = reference(case, A, B, C)
            offs = [case.off if i == case.real else 0 for i in (0, 1)]
            pa = xc.Placed(case.extents(case.modes[0]), dts[0], case.pad[0], offs[0])
            pb = xc.Placed(case.extents(case.modes[1]), dts[1], case.pad[1], offs[1])
            pa.set(A)
            pb.set(B)
            pd = xc.Placed(case.extents(case.modes[2]), "complex128", case.pad[2])          # D: NaN everywhere
            pc = xc.Placed(case.extents(case.modes[2]), "complex128", case.pad[3])          # C: NaN everywhere — beta = 0 must not read it
            if case.beta != 0:
                pc.set(C)
            plan.contract(case.alpha, pa.ptr, pb.ptr, case.beta, pc.ptr, pd.ptr, ws.data_ptr(), plan.required_workspace)
            torch.cuda.synchronize()
            what = "%s (draw %d) %s" % (case.id, int(swap), d.raw)
            xd.assert_exact(pd.get(), want, what)
            for p, name in ((pd, "D"), (pa, "A"), (pb, "B"), (pc, "C")):
                p.check_outside(what + " " + name)
    finally:
        plan.destroy()
    return d


if __name__ == "__main__":
    from cudalibrarysamples_amd import cutensor as ct_, ops as ops_
    mode_ = sys.argv[1]
    h_ = ops_.Handle()
    for cid in sys.argv[2:]:
        if mode_ == "plan":
            plan_path(ct_, ops_, h_, BY_ID[cid])
        else:
            run_case(ct_, ops_, h_, BY_ID[cid])
        print("ok", cid, flush=True)
