"""The case table of the exact many-mode tests (tests/test_many_modes_cpu.py plans every case and checks every draw,
tests/test_gpu_many_modes_exact.py runs every case) — a helper module, not a conftest: permutations, binary operations and reductions
with more unfusable modes than the tiled kernels describe, which plan onto the mode-table kernels of kernels/elementwise_table.hip.

Data, scalars, references and the checks are those of tests/ew_exact_cases.py (integers in [-3, 3], scalars from {+-1, +-2, +-0.5}, the
reduction data of its operators, NaN-filled guarded buffers, zero tolerance, nothing outside D written, A and a separate C unchanged, at
least two draws); each case names its kernel with a predicate on the plan's description.  The buffers are laid out on the host and moved
as flat bytes (HostPlaced): a strided device copy of a 20-mode view is more dimensions than torch's device copy kernels take."""
import os
import string
import sys

import numpy as np

import ew_exact_cases as ew
import exact_cases as xc
import exact_data as xd
import workspace_cases as wc

EW_TABLE_TILE, EW_TABLE_GATHER, RED_TABLE = 5, 6, 3
GATHER = {"CUTENSOR_AMD_EW_TABLE": "gather"}        # hooks flavour: the gather kernel where the tile kernel applies
UNARY = {"ABS": np.abs, "NEG": np.negative}


class Case(ew.Case):
    """ew_exact_cases.Case with a unary operator on A (`un`) and strides scaled per tensor (`scale`: no stride-1 mode)"""

    def __init__(self, *a, un=None, scale=None, **kw):
        super().__init__(*a, **kw)
        self.un, self.scale = un, dict(scale or {})

    def strides(self, t):
        k = self.scale.get(t, 1)
        return [s * k for s in super().strides(t)]


CASES = []


def add(*a, **kw):
    c = Case(*a, **kw)
    assert all(c.id != o.id for o in CASES), c.id
    CASES.append(c)
    return c


def tiled(d):
    return d.get("op") == "elementwise" and d.get("variant") == EW_TABLE_TILE and d.get("kname") == "ew_table_tile_kernel"


def gather(d):
    return d.get("op") == "elementwise" and d.get("variant") == EW_TABLE_GATHER and d.get("kname") == "ew_table_gather_kernel"


def table_reduction(**want):
    return lambda d: d.get("op") == "reduction" and d.get("variant") == RED_TABLE and d.get("kname") == "reduce_table_kernel" and ew._is(**want)(d)


def modes_of(n):
    return string.ascii_lowercase[:n]


def ext_of(extents):
    return dict(zip(modes_of(len(extents)), extents))


SHORT = ew.SHORT
PERM_RUNS = [((1.0,), "none"), ((-0.5,), "none")]
M12, M14, M20 = modes_of(12), modes_of(14), modes_of(20)
E12, E14, E20 = ext_of([2] * 12), ext_of([2] * 14), ext_of([2] * 20)
MIXED9 = ext_of((3, 2, 5, 2, 3, 2, 2, 3, 2))
M9 = modes_of(9)
LONG8 = ext_of((70, 2, 3, 2, 2, 3, 2, 2))
M8 = modes_of(8)
OUTER20_D = "ktbrgoaqfsdnicpjmelh"
assert sorted(OUTER20_D) == sorted(M20) and not any(ord(y) - ord(x) == 1 for x, y in zip(OUTER20_D, OUTER20_D[1:]))


def permutation(name, dtype, ext, mA, mD, expect, **kw):
    return add("%s_perm_%s" % (SHORT[dtype], name), "permutation", dtype, ext, (mA, mD), expect, PERM_RUNS, **kw)


# ---- the tile kernel ------------------------------------------------------------------------------------------------------------------
for _dt in ("float32", "bfloat16", "float16", "float64", "complex64", "complex128"):
    permutation("rev12", _dt, E12, M12, M12[::-1], tiled)
    if _dt in ew.CPLX:
        permutation("rev12_conj", _dt, E12, M12, M12[::-1], tiled, conj=(True, False))
permutation("rev12_abs", "float32", E12, M12, M12[::-1], tiled, un="ABS")
permutation("rev12_neg", "float32", E12, M12, M12[::-1], tiled, un="NEG")
# the same plan under the switch: the predicate tells the two kernels apart (run in a child process)
REV12_GATHER = permutation("rev12_gather", "float32", E12, M12, M12[::-1], gather, env=GATHER)
# the two tile sets overlap: a leads both tensors
permutation("shared_lead14", "float32", E14, M14, "a" + M14[:0:-1], tiled)
# digits that are no powers of two
permutation("mixed9", "float32", MIXED9, M9, M9[::-1], tiled)
permutation("mixed9", "bfloat16", MIXED9, M9, M9[::-1], tiled)
permutation("mixed9", "complex128", MIXED9, M9, M9[::-1], tiled)
# a mode too long for the tile, cut, its last piece partial: leading A, and leading D
permutation("long_in_a", "float32", LONG8, M8, M8[::-1], tiled)
permutation("long_in_d", "float32", LONG8, M8[::-1], M8, tiled)
permutation("long_in_d", "float64", LONG8, M8[::-1], M8, tiled)
# identity order, every pitch padded on both sides by different amounts (nothing fuses), odd element offset, alignment of one element
permutation("padded_identity", "float32", MIXED9, M9, M9, tiled, pad={"A": (1,) * 9, "D": (2, 1, 2, 1, 2, 1, 2, 1, 2)}, off=3, align=4)
# 1 Mi elements: many outer digits, many tiles per workgroup
permutation("outer20", "float32", E20, M20, OUTER20_D, lambda d: tiled(d) and d.get("modes") == 20 and d.get("blocks") >= 4 * d.get("grid") > 4)

# ---- the gather kernel ----------------------------------------------------------------------------------------------------------------
permutation("broadcast8", "float32", ext_of([2] * 8), "hfdb", M8, gather)
permutation("no_unit_stride", "float32", MIXED9, M9, M9[::-1], gather, scale={"A": 2})
permutation("no_unit_stride", "complex64", MIXED9, M9, M9[::-1], gather, scale={"A": 2})


# ---- binary ---------------------------------------------------------------------------------------------------------------------------
def binary(name, dtype, ext, mA, mC, mD, expect, ops=None, **kw):
    """C in a buffer of its own; where C has D's layout also in place, and under ADD with gamma = 0 over a NaN D"""
    same = mC == mD and kw.get("pad", {}).get("C", 0) == kw.get("pad", {}).get("D", 0)
    for i, op in enumerate(ops or (("ADD", "MUL") if dtype in ew.CPLX else ew.BINOPS)):
        s = ew.EW_SCALARS[(i + len(name)) % 6]
        runs = [((s[0], s[2]), "separate")] + ([((s[1], s[0]), "inplace")] if same else []) + ([((s[2], 0.0), "none")] if op == "ADD" and same else [])
        add("%s_bin_%s_%s" % (SHORT[dtype], name, op.lower()), "binary", dtype, ext, (mA, mC, mD), expect, runs, op=op, **kw)


for _n, _e, _m in (("rev12", E12, M12), ("mixed9", MIXED9, M9)):
    binary(_n, "float32", _e, _m, _m[::-1], _m[::-1], tiled)                                            # C in D's layout, all four combiners
    binary(_n + "_c_pad", "float32", _e, _m, _m[::-1], _m[::-1], tiled, ops=("ADD", "MAX"), pad={"C": (1,) * len(_m)})
    binary(_n + "_c_order", "float32", _e, _m, _m, _m[::-1], tiled, ops=("ADD", "MUL"))               # C in A's mode order
binary("rev12", "complex64", E12, M12, M12[::-1], M12[::-1], tiled, conj=(True, True))
binary("mixed9", "bfloat16", MIXED9, M9, M9[::-1], M9[::-1], tiled, ops=("ADD", "MIN"))
binary("broadcast8", "float32", ext_of([2] * 8), "hfdb", M8, M8, gather, ops=("ADD", "MUL"))


# ---- reductions -----------------------------------------------------------------------------------------------------------------------
def reductions(name, dtype, ext, mA, mD, expect, ops=None, **kw):
    for i, op in enumerate(ops or (("ADD", "MUL") if dtype in ew.CPLX else ("ADD", "MUL", "MAX", "MIN"))):
        add("%s_red_%s_%s" % (SHORT[dtype], name, op.lower()), "reduction", dtype, ext, (mA, mD), expect, ew._red_runs(op, dtype, i + len(name)), op=op, **kw)


M10 = modes_of(10)
E10 = ext_of([2] * 10)
MIXED10 = ext_of((3, 2, 5, 2, 3, 2, 2, 3, 2, 2))
# every other mode kept: five kept and five reduced digits, in A's order and reversed
reductions("alt10", "float32", E10, M10, "acegi", table_reduction(kept=32, red=32))
reductions("alt10_rev", "float32", E10, M10, "igeca", table_reduction(kept=32, red=32), ops=("ADD", "MAX"))
reductions("mixed10", "float32", MIXED10, M10, "acegi", table_reduction(kept=180, red=48))
for _dt in ("bfloat16", "float64", "complex64"):
    reductions("alt10", _dt, E10, M10, "acegi", table_reduction(kept=32, red=32), ops=("ADD",))
reductions("mixed10_conj", "complex64", MIXED10, M10, "acegi", table_reduction(kept=180, red=48), ops=("ADD",), conj=(True, True))
reductions("alt10_acc64", "float32", E10, M10, "acegi", table_reduction(kept=32, red=32), ops=("ADD",), compute="64F")
# to a scalar: eight reduced digits that do not fuse (A's pitches padded), the range split four ways
reductions("to_scalar8", "float32", ext_of([2] * 8), M8, "", table_reduction(kept=1, red=256, splitR=(2, 4096)), ops=("ADD", "MIN"), pad={"A": (1,) * 8})
# only one group oversized
reductions("kept7_red1", "float32", ext_of([2] * 7 + [5]), M8, M8[6::-1], table_reduction(kept=128, red=5), ops=("ADD", "MIN"))
reductions("kept1_red7", "float32", ext_of([3] + [2] * 7), M8, "a", table_reduction(kept=3, red=128), ops=("ADD", "MUL"), pad={"A": (1,) * 8})
# 15 modes, two kept: the planner splits the reduced range (partials in the workspace, reduce_table_finalize_kernel)
M15 = modes_of(15)
reductions("split15", "float32", ext_of([2] * 15), M15, "ck", lambda d: table_reduction(kept=4, red=8192, splitR=(2, 4096))(d) and d.get("workspace") == d.get("splitR") * 4 * 4,
           ops=("ADD", "MUL"), pad={"A": (1,) * 8 + (0,) * 7})
reductions("split15_acc64", "float32", ext_of([2] * 15), M15, "ck", lambda d: table_reduction(kept=4, red=8192, splitR=(2, 4096))(d) and d.get("workspace") == d.get("splitR") * 4 * 8,
           ops=("ADD",), pad={"A": (1,) * 8 + (0,) * 7}, compute="64F")

BY_ID = {c.id: c for c in CASES}
# the 25-mode tensor of the reference's contraction_jit.cu (extent 2 throughout), three single modes moved to the front: seven groups
M25 = modes_of(25)
FRONT3_D = "fmt" + "".join(c for c in M25 if c not in "fmt")
NO_SWITCH = [c.id for c in CASES if not c.env]


# ---- plans ----------------------------------------------------------------------------------------------------------------------------
def make_plan(ct, ops, h, case):
    if case.un is None:
        return ew.make_plan(ct, ops, h, case)
    assert case.kind == "permutation"
    e, m, s = case.extents, case.modes, case.strides
    with wc.hook_env(case):
        return ops.permutation_plan(h, e("A"), m["A"], e("D"), m["D"], dtype=xc._dt(ct, case.dtype), strideA=s("A"), strideB=s("D"),
                                    alignment=case.align or 128, opA=ops._unary(case.un))


def plan_path(ct, ops, h, case):
    """the case's plan is on the path the case names (the planner needs no GPU); returns the description"""
    plan = make_plan(ct, ops, h, case)
    try:
        d = wc.describe(ct, plan)
        assert case.expect(d), "%s is off its path: %s" % (case.id, d)
        return {k: v for k, v in d.pairs}
    finally:
        plan.destroy()


# ---- data and references: ew_exact_cases', with the unary operator applied to A ------------------------------------------------------
def reference(case, ins, run):
    if case.un is not None:
        ins = dict(ins, A=UNARY[case.un](ins["A"]))
    return ew.reference(case, ins, run)


def check_case(case, d):
    """every draw and run: the data conditions and the reference's representability (ew_exact_cases.check_case), the operator included"""
    n = ew.check_case(case, d)
    if case.un is not None:
        for draw in range(n):
            ins = ew.make_draw(case, draw, d)
            for run in case.runs:
                ew.expected(case, reference(case, ins, run))
    return n


# ---- one tensor in a NaN-filled device buffer, laid out on the host -------------------------------------------------------------------
class HostPlaced:
    """exact_cases.Placed for any number of modes: the buffer is built, read back and checked on the host, and crosses as flat bytes"""

    def __init__(self, extents, dtype, off=0, strides=None):
        import torch
        self.extents, self.strides = list(extents), list(strides)
        self.tdt = xd.TORCH_DTYPES[dtype]
        self.es = torch.empty((), dtype=self.tdt).element_size()
        span = 1 + sum((e - 1) * s for e, s in zip(self.extents, self.strides)) if self.extents else 1
        self.start = xc.GUARD + off
        self.host = torch.full(((2 * xc.GUARD + off + span) * self.es,), 0xFF, dtype=torch.uint8)           # 0xFF..: a NaN in every type
        self.raw = self.host.cuda()
        self.ptr = self.raw.data_ptr() + self.start * self.es

    def _view(self, raw):
        rev = lambda x: list(reversed(x)) or [1]   # noqa: E731
        v = raw.view(self.tdt).as_strided(rev(self.extents), rev(self.strides), self.start)
        return v.permute(*reversed(range(v.dim()))) if self.extents else v.reshape(())

    def set(self, host):
        self._view(self.host).copy_(host)
        self.raw.copy_(self.host)

    def get(self):
        return self._view(self.raw.cpu()).clone()

    def check_outside(self, what):
        """every byte outside the tensor's own elements still 0xFF"""
        import torch
        back = self.raw.cpu()
        inside = torch.zeros(back.numel() // self.es, dtype=torch.bool)
        rev = lambda x: list(reversed(x)) or [1]   # noqa: E731
        inside.as_strided(rev(self.extents), rev(self.strides), self.start).fill_(True)
        touched = (back.view(-1, self.es) != 0xFF).any(dim=1) & ~inside
        assert not bool(touched.any()), "%s: %d elements outside the tensor written; the first at element %d (it starts at %d)" % (
            what, int(touched.sum()), int(torch.nonzero(touched)[0]), self.start)


def _placed(case, t):
    return HostPlaced(case.extents(t), case.dtype, off=case.off, strides=case.strides(t))


def run_case(ct, ops, h, case, make=None, check=None, expect=None, runs=None):
    """ew_exact_cases.run_case on HostPlaced buffers; A is checked unchanged too"""
    import torch
    make, check, expect = make or ew.make_draw, check or ew.check_draw, expect or ew.expected
    plan = make_plan(ct, ops, h, case)
    try:
        desc = wc.describe(ct, plan)
        assert case.expect(desc), "%s is off its path: %s" % (case.id, desc)
        d = {k: v for k, v in desc.pairs}
        ws = torch.empty(max(plan.required_workspace, 256), dtype=torch.uint8, device="cuda")
        for draw in range(ew.n_draws(case, d)):
            ins = make(case, draw, d)
            pa = _placed(case, "A")
            pa.set(ew._host(case, ins["A"]))
            for run in (runs or case.runs):
                scal, cmode = run
                check(case, ins, run, d)
                want = expect(case, reference(case, ins, run))
                pd = _placed(case, "D")                                     # NaN everywhere
                pc = None
                if cmode == "inplace":
                    pd.set(ew._host(case, ins["C"]))
                elif cmode == "separate":
                    pc = _placed(case, "C" if "C" in case.modes else "D")
                    pc.set(ew._host(case, ins["C"]))
                cptr = pc.ptr if pc else pd.ptr
                if case.kind == "permutation":
                    plan.permute(scal[0], pa.ptr, pd.ptr)
                elif case.kind == "binary":
                    plan.binary(scal[0], pa.ptr, scal[1], cptr, pd.ptr)
                else:
                    plan.reduce(scal[0], pa.ptr, scal[1], cptr, pd.ptr, ws.data_ptr(), plan.required_workspace)
                torch.cuda.synchronize()
                what = "%s (draw %d, scalars %s, C %s) %s" % (case.id, draw, scal, cmode, desc)
                xd.assert_exact(pd.get(), want, what)
                pd.check_outside(what)
                if pc is not None:
                    xd.assert_exact(pc.get(), ew._host(case, ins["C"]), what + ": C was written")
                    pc.check_outside(what + " (C)")
            xd.assert_exact(pa.get(), ew._host(case, ins["A"]), "%s (draw %d): A was written" % (case.id, draw))
            pa.check_outside("%s (draw %d) (A)" % (case.id, draw))
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
        if mode_ == "plan":
            plan_path(ct_, ops_, h_, BY_ID[cid])
        else:
            run_case(ct_, ops_, h_, BY_ID[cid])
        print("ok", cid, flush=True)
