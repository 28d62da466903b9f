"""The case table of the unary-operator tests (tests/test_unary_cpu.py plans every case and checks every draw on the CPU,
tests/test_gpu_unary_exact.py runs every case, tests/test_gpu_unary_transcendental.py the four transcendental operators) — a helper
module, not a conftest.  The per-operand operators of cutensorPermute, cutensorElementwiseBinaryExecute,
cutensorElementwiseTrinaryExecute and cutensorReduce on real data:

    permutation   D = alpha * uA(perm A)
    binary        D = opAC(alpha * uA(perm A), gamma * uC(C))
    trinary       D = opABC(opAB(alpha * uA(A), beta * uB(B)), gamma * uC(C))
    reduction     D = alpha * reduce_op(uA(A)) + beta * uC(C)

Geometry (extents, modes, padded pitches, element offset, alignment, switches), runs (scalars, where C lives), buffers and the predicate
that proves the kernel all come from tests/ew_exact_cases.py: one case here is one REAL-data case of that table with operators attached.
The plans are built here (ew_exact_cases.make_plan only knows conjugation).  A plan with an operator must meet its base case's predicate:
the operator changes the arithmetic, never the path.

Exact cases (zero tolerance): ABS, NEG, RELU on integers in [-3, 3]; SQRT on perfect squares up to 16; RCP on +-2^k, |k| <= 2; scalars and C
as in the base table.  Any correct evaluation is exact on them, the reference (numpy, float64: the operator on the inputs, then the base
table's reference) asserts that every output is a value of the data type before anything runs.
  * permutation / binary: the operators rotate through the five over the table, so every kernel meets several of them.
  * trinary: uA = ABS, uB = NEG, uC = RELU on signed data — a misattributed or doubly applied operator changes the result — on every form
    (E = A, E = B, two tiles, two passes, and the single gather launch when C is D).
  * reductions, by the base case's operator: ADD -> NEG on A and RELU on C (beta != 0 with C in place and apart; beta = 0 over a NaN D
    with uC set), plus ABS (an L1 norm) or SQRT on A in a second case; MAX -> ABS with one spike of -100 per kept element; MIN -> NEG with
    one spike of +100; MUL -> RCP on powers of two.  The spikes sit where ew_exact_cases.forced_positions says: the ends, both sides of
    every split boundary, the unrolled loops' tails.  ABS under MAX shows an operator that is missing or applied to the identity
    element (-inf); NEG under MIN and under ADD shows one applied twice (to a partial) as well.  16-bit ADD data is mostly zeros (at most
    24 non-zeros per reduced line) so that alpha * sum + beta * c stays an exact integer of the type."""
import os
import sys

import numpy as np

import ew_exact_cases as ec
import exact_cases as xc
import exact_data as xd
import workspace_cases as wc

EXACT_OPS = ("ABS", "NEG", "RELU", "SQRT", "RCP")
ALL_OPS = ("SQRT", "RELU", "RCP", "SIGMOID", "TANH", "EXP", "LOG", "ABS", "NEG")
REAL_DTYPES = ("float32", "bfloat16", "float16", "float64")
NONZERO_16 = 24                                                               # non-zeros per reduced line of a 16-bit ADD reduction
PSI = {"IDENTITY": lambda x: x, "ABS": np.abs, "NEG": np.negative, "RELU": lambda x: np.where(x > 0, x, 0 * x), "SQRT": np.sqrt,
       "RCP": lambda x: 1.0 / x}
VALUES = {"IDENTITY": range(-3, 4), "ABS": range(-3, 4), "NEG": range(-3, 4), "RELU": range(-3, 4), "SQRT": (0, 1, 4, 9, 16),
          "RCP": (-4.0, -2.0, -1.0, -0.5, -0.25, 0.25, 0.5, 1.0, 2.0, 4.0)}
REAL_BASES = [c for c in ec.CASES if c.dtype not in ec.CPLX]


class UCase:
    """a base case of ew_exact_cases with a unary operator per operand (by name; operands not named keep IDENTITY)"""

    def __init__(self, base, un, tag):
        self.base, self.un = base, {t: un.get(t, "IDENTITY") for t in "ABC"}
        self.id = "%s__%s" % (base.id, tag)
        self.kind, self.dtype, self.runs, self.env = base.kind, base.dtype, base.runs, base.env

    def __repr__(self):
        return self.id


CASES = []


def _add(base, tag, **un):
    CASES.append(UCase(base, un, tag))


def _build():
    i = 0
    for b in REAL_BASES:
        if b.kind == "permutation":
            _add(b, EXACT_OPS[i % 5].lower(), A=EXACT_OPS[i % 5])
        elif b.kind == "binary":
            a, c = EXACT_OPS[i % 5], EXACT_OPS[(i // 5 + i + 2) % 5]
            _add(b, "%s_%s" % (a.lower(), c.lower()), A=a, C=c)
        elif b.kind == "trinary":
            _add(b, "abs_neg_relu", A="ABS", B="NEG", C="RELU")
        elif b.op == "ADD":
            _add(b, "neg_relu", A="NEG", C="RELU")
            _add(b, "abs_neg" if i % 2 else "sqrt_abs", A="ABS" if i % 2 else "SQRT", C="NEG" if i % 2 else "ABS")
        elif b.op == "MAX":
            _add(b, "abs", A="ABS")
        elif b.op == "MIN":
            _add(b, "neg", A="NEG")
        else:
            _add(b, "rcp", A="RCP")
        i += 1


_build()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
NO_SWITCH = [c.id for c in CASES if not c.env]


# ---- plans -------------------------------------------------------------------------------------------------------------------------------
def make_plan(ct, ops, h, base, un):
    """the base case's plan with the operators `un` (tensor -> name); names go through ops' own table"""
    dt = xc._dt(ct, base.dtype)
    m, e, s, al = base.modes, base.extents, base.strides, base.align or 128
    u = {t: un.get(t, "IDENTITY") for t in "ABC"}
    with wc.hook_env(base):
        if base.kind == "permutation":
            return ops.permutation_plan(h, e("A"), m["A"], e("D"), m["D"], dtype=dt, strideA=s("A"), strideB=s("D"), alignment=al, opA=u["A"])
        if base.kind == "binary":
            if m["C"] == m["D"] and s("C") == s("D"):
                return ops.binary_plan(h, e("A"), m["A"], e("D"), m["D"], op=base.op, dtype=dt, alignment=al, opA=u["A"], opC=u["C"],
                                       strideA=s("A"), strideC=s("D"))
            import ctypes
            dA, dC, dD = (ops.tensor_descriptor(h, e(t), s(t), dt, al) for t in "ACD")
            opd = ctypes.c_void_p()
            st = ct.cutensorCreateElementwiseBinary(h.h, ctypes.byref(opd), dA, ct.i32(m["A"]), ops._unary(u["A"]), dC, ct.i32(m["C"]), ops._unary(u["C"]),
                                                    dD, ct.i32(m["D"]), ops._OPS[base.op], ct.compute_desc(ops._DTYPE_COMPUTE[dt]))
            for d in (dA, dC, dD):
                ct.cutensorDestroyTensorDescriptor(d)
            ct.check(st)
            return ops.Plan(h, opd, "binary", dt, workspace_limit=0)
        if base.kind == "trinary":
            return ops.trinary_plan(h, e("A"), m["A"], e("B"), m["B"], e("C"), m["C"], e("D"), m["D"], opAB=base.op[0], opABC=base.op[1], dtype=dt,
                                    alignment=al, strideA=s("A"), strideB=s("B"), strideC=s("C"), strideD=s("D"), opA=u["A"], opB=u["B"], opC=u["C"])
        return ops.reduction_plan(h, e("A"), m["A"], e("D"), m["D"], dtype=dt, strideA=s("A"), strideC=s("D"), op_reduce=ops._OPS[base.op],
                                  compute=base.compute, alignment=al, opA=u["A"], opC=u["C"], workspace_limit=1 << 24)


def describe(ct, ops, h, base, un):
    plan = make_plan(ct, ops, h, base, un)
    try:
        return wc.describe(ct, plan)
    finally:
        plan.destroy()


def plan_path(ct, ops, h, case):
    """the case plans onto its base case's path; returns the description as a dict"""
    d = describe(ct, ops, h, case.base, case.un)
    assert case.base.expect(d), "%s is off its path: %s" % (case.id, d.pairs)
    return {k: v for k, v in d.pairs}


# ---- data --------------------------------------------------------------------------------------------------------------------------------
def _pick(rng, shape, values):
    v = np.asarray(list(values), dtype=np.float64)
    return v[rng.integers(0, len(v), size=shape)]


def make_draw(case, draw, d):
    """the logical host tensors of one draw (float64, modes in descriptor order) by tensor name — what the device buffers hold"""
    b = case.base
    out = {}
    if b.kind != "reduction":
        for i, t in enumerate(ec.TENSORS[b.kind][:-1]):
            out[t] = _pick(ec._rng(b, draw, 100 + i), b.extents(t), VALUES[case.un[t]])
        return out
    kept, red, _ = ec._lines(b)
    rng = ec._rng(b, draw, 100)
    out["C"] = _pick(ec._rng(b, draw, 102), b.extents("D"), VALUES[case.un["C"]])
    if b.op == "ADD":
        A2 = _pick(rng, (kept, red), VALUES[case.un["A"]])
        if b.dtype in xd.H16 and red > NONZERO_16:           # mostly zeros: the sum of the line's magnitudes stays in the type's integer range
            keep = np.zeros((kept, red), dtype=bool)
            for k in range(kept):
                keep[k, rng.choice(red, size=NONZERO_16, replace=False)] = True
            A2 = np.where(keep, A2, 0.0)
    elif b.op in ("MAX", "MIN"):
        A2 = _pick(rng, (kept, red), range(-3, 4))
        A2[np.arange(kept), ec.spike_positions(b, d, draw)] = -100.0 if b.op == "MAX" else 100.0     # |-100| is the maximum, -(+100) the minimum
    else:
        return dict(out, A=np.asarray(ec.make_draw(b, draw, d)["A"], dtype=np.float64))      # MUL: -1 with a few -2 and -0.5 — all powers of two
    out["A"] = ec._from_lines(b, A2)
    return out


def reference(case, ins, run):
    """the exact result: the operators on the inputs (float64), then the base table's reference"""
    with np.errstate(all="raise"):
        return ec.reference(case.base, {t: PSI[case.un[t]](np.asarray(x, dtype=np.float64)) for t, x in ins.items()}, run)


def check_draw(case, ins, run):
    """conditions on one run's data, asserted before anything is launched: the values each operator takes, the accumulator bound"""
    b = case.base
    for t, x in ins.items():
        if b.kind == "reduction" and t == "A" and b.op in ("MAX", "MIN", "MUL"):
            continue
        assert set(np.unique(x)) <= set(float(v) for v in VALUES[case.un[t]]) | ({0.0} if b.kind == "reduction" else set()), (case.id, t)
    if b.kind == "reduction":
        alpha, beta = run[0]
        _, red = ec._red_axes(b)
        pa = np.abs(PSI[case.un["A"]](ins["A"]))
        if b.op == "ADD":
            bound = abs(alpha) * float(pa.sum(axis=tuple(red)).max())
        elif b.op == "MUL":
            bound = abs(alpha) * 2.0 ** 10
            assert float(np.abs(np.log2(np.abs(np.prod(PSI[case.un["A"]](ins["A"]), axis=tuple(red))))).max()) <= 10.0, case.id
        else:
            bound = abs(alpha) * float(pa.max())
        bound += abs(beta) * 4.0
        assert bound < xd.acc_limit(b.dtype) / 2, (case.id, bound)


def expected(case, ref):
    return ec.expected(case.base, ref)


def check_case(case, d):
    """every draw and run: the data conditions, the reference's representability, and for MAX / MIN that the spike decides every line and
    visits every forced position; returns the number of draws"""
    b = case.base
    n = ec.n_draws(b, d)
    seen = set()
    for draw in range(n):
        ins = make_draw(case, draw, d)
        for run in b.runs:
            check_draw(case, ins, run)
            expected(case, reference(case, ins, run))
        if b.kind == "reduction" and b.op in ("MAX", "MIN"):
            _, red = ec._red_axes(b)
            pa = PSI[case.un["A"]](ins["A"])
            ext = {"MAX": np.max, "MIN": np.min}[b.op](pa, axis=tuple(red))
            assert bool((ext == (100.0 if b.op == "MAX" else -100.0)).all()), case.id
            raw = {"MAX": np.max, "MIN": np.min}[b.op](ins["A"], axis=tuple(red))
            assert bool((raw != ext).all()), case.id                         # without the operator every line gives another value
            seen |= set(int(p) for p in ec.spike_positions(b, d, draw))
    if b.kind == "reduction" and b.op in ("MAX", "MIN"):
        kept, red, _ = ec._lines(b)
        missing = set(ec.forced_positions(red, d["splitR"], d["redPerSplit"])) - seen
        assert not missing, "%s: no spike at reduced indices %s" % (case.id, sorted(missing))
    return n


# ---- running a case -----------------------------------------------------------------------------------------------------------------------
def launch(plan, base, scal, ptrs, cptr, dptr, ws):
    if base.kind == "permutation":
        plan.permute(scal[0], ptrs["A"], dptr)
    elif base.kind == "binary":
        plan.binary(scal[0], ptrs["A"], scal[1], cptr, dptr)
    elif base.kind == "trinary":
        plan.trinary(scal[0], ptrs["A"], scal[1], ptrs["B"], scal[2], cptr, dptr)
    else:
        plan.reduce(scal[0], ptrs["A"], scal[1], cptr, dptr, ws.data_ptr(), plan.required_workspace)


def run_plan(ct, plan, case, d, what):
    """every draw and run of `case` on `plan` in NaN-guarded buffers: D exact, nothing outside D written, a separate C unchanged"""
    import torch
    b = case.base
    ws = torch.empty(max(plan.required_workspace, 256), dtype=torch.uint8, device="cuda")
    for draw in range(ec.n_draws(b, d)):
        ins = make_draw(case, draw, d)
        dev = {}
        for t in ec.TENSORS[b.kind][:-1]:
            if t != "C":
                dev[t] = ec._placed(b, t)
                dev[t].set(ec._host(b, ins[t]))
        for run in b.runs:
            scal, cmode = run
            check_draw(case, ins, run)
            want = expected(case, reference(case, ins, run))
            pd = ec._placed(b, "D")                                     # NaN everywhere
            pc = None
            if cmode == "inplace":
                pd.set(ec._host(b, ins["C"]))
            elif cmode == "separate":
                pc = ec._placed(b, "C" if "C" in b.modes else "D")
                pc.set(ec._host(b, ins["C"]))
            launch(plan, b, scal, {t: p.ptr for t, p in dev.items()}, pc.ptr if pc else pd.ptr, pd.ptr, ws)
            torch.cuda.synchronize()
            w = "%s (draw %d, scalars %s, C %s) %s" % (what, draw, scal, cmode, d)
            xd.assert_exact(pd.get(), want, w)
            pd.check_outside(w)
            if pc is not None:
                xd.assert_exact(pc.get(), ec._host(b, ins["C"]), w + ": C was written")
                pc.check_outside(w + " (C)")


def run_case(ct, ops, h, case):
    plan = make_plan(ct, ops, h, case.base, case.un)
    try:
        desc = wc.describe(ct, plan)
        assert case.base.expect(desc), "%s is off its path: %s" % (case.id, desc.pairs)
        d = {k: v for k, v in desc.pairs}
        run_plan(ct, plan, case, d, case.id)
    finally:
        plan.destroy()
    return d


if __name__ == "__main__":
    from cudalibrarysamples_amd import cutensor as ct_, ops as ops_
    mode_ = sys.argv[1]
    if mode_ == "production":
        assert os.environ.get("CTAMD_LIB_FLAVOUR") != "hooks" and "lib_hooks" not in ct_.LIB_PATH, ct_.LIB_PATH
    h_ = ops_.Handle()
    for cid in sys.argv[2:]:
        run_case(ct_, ops_, h_, BY_ID[cid])
        print("ok", cid, flush=True)
