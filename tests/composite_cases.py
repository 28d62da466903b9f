"""The case table of the exact, guarded tests of the three entry points built on top of the tiled kernels (tests/test_composite_cpu.py plans
every case and checks every draw, tests/test_gpu_composite_exact.py runs every case) — a helper module, not a conftest, the sibling of
tests/exact_cases.py and tests/ew_exact_cases.py for

  * cutensorContractTrinary   (exec_contraction.cpp: two pairwise plans through an intermediate at the head of the workspace),
  * cutensorBlockSparseContract (blocksparse.cpp: one dense plan per shape triple, contributions accumulated through D, untouched output
    blocks scaled or cleared),
  * cutensorPermute with CUTENSOR_OPERATION_DESCRIPTOR_PADDING_* (a fill of the whole padded buffer, then the inner plan at an element offset).

Each is host code that splits one call into several launches; what can go wrong is the arithmetic between the launches: which scalar a
step carries, where a temporary lies, which pointer and pitch a step gets, what alignment it may assume.

A case: id, kind, data type, extents, modes, first-mode pitch padding per tensor, an element offset and a descriptor alignment, operators,
its `runs` (scalars and where the beta source lives: "inplace", "separate", or "none" — beta = 0 and the buffer passed holds NaN) and a
predicate on ctamdDescribePlan.  Every tensor lives in a 0xFF-filled buffer (exact_cases.Placed, workspace_cases.GuardedBlocks); after
each launch the output is compared with ZERO tolerance, everything outside the output's own elements must still be 0xFF, every input and
a separate beta source must be unchanged byte for byte, and a workspace of exactly required_workspace bytes must have kept its guards.

The data rule (a condition on the data, asserted on the reference on the CPU — never a tolerance): operand values are integers; scalars
come from exact_cases.SCALARS32 / SCALARS16, complex ones have integer or half parts.
  * trinary: the intermediate of EACH of the three pair orders, computed in int64, is a value of the data type (|x| <= 256 for bf16, 2048
    for fp16, 2^24 for fp32, 2^53 for fp64; under a reduced compute descriptor below the limit of the type the operands are rounded to:
    TF32 |x| < 2^16); |alpha| sum |a||b||c| + |beta||d| stays below the accumulator's exact range (one binary digit less when a scalar has
    a half).  The result then does not depend on the order the library picks.
  * block-sparse: the contributions to one output block are accumulated through D in the data type: every prefix of them, in task order
    and in its reverse, is a value of the data type.
  * every exact output is a value of the output type: nothing rounds, 16-bit cases included (dense +-1 over short contracted ranges).
References are numpy on int64 / float64 (complex: complex128 of integers below 2^53) and never come from the library."""
import ctypes
import json
import os
import sys
import zlib

import numpy as np

import exact_cases as xc
import exact_data as xd
import workspace_cases as wc
from ew_exact_cases import CPLX, EW_BLOCK, EW_GENERIC, EW_ROWCOPY, EW_TRANSPOSE, EW_TRANSPOSE_ANY, NV, SHORT

KINDS = ("contraction_trinary", "blocksparse", "padded_permutation")
DTYPES = ("float32", "float64", "bfloat16", "float16", "complex64", "complex128")
EXACT_LIMIT = {"bfloat16": 2 ** 8, "float16": 2 ** 11, "float32": 2 ** 24, "float64": 2 ** 53, "complex64": 2 ** 24, "complex128": 2 ** 53}
ROUNDED_BELOW = {"16BF": 2 ** 8, "16F": 2 ** 11, "TF32": 2 ** 16}          # a reduced descriptor rounds the operands — the intermediate too
PAIRS = ((0, 1, 2), (0, 2, 1), (1, 2, 0))                                  # api.cpp, cutensorCreateContractionTrinary: pairs[3][3]
CSCALARS = [(1 + 1j, 0.0), (-2 + 0.5j, 1 - 0.5j), (0.5 - 1j, -0.5 + 2j), (-1j, 0.0), (1 - 2j, 1j), (2 + 0.5j, 0.0)]   # tests/test_gpu_c32x.py
NOT_SUPPORTED = 15
F32X = {"CUTENSOR_AMD_F32X": "force"}
ES = {"float32": 4, "float64": 8, "bfloat16": 2, "float16": 2, "complex64": 8, "complex128": 16}
TENSORS = {"contraction_trinary": "ABCDE", "blocksparse": "ABCD", "padded_permutation": "AD"}


class Case:
    def __init__(self, id, kind, dtype, ext, modes, expect=None, runs=(), pad=None, off=0, align=None, conj="", compute=None, env=None,
                 blocks=None, layout="own", padding=None, opA=None, refuse=None, strided=""):
        self.id, self.kind, self.dtype, self.ext, self.runs = id, kind, dtype, ext, list(runs)
        # (a trinary contraction's E has D's modes, a block-sparse D has C's)
        self.modes = dict(zip(TENSORS[kind], tuple(modes) + ((modes[-1],) if kind != "padded_permutation" else ())))
        self.expect = expect or (lambda d: True)
        self.pad = dict(pad or {})                 # tensor -> elements added to the first mode's pitch (block-sparse: one number per block)
        self.off, self.align, self.conj, self.compute, self.env = off, align, conj, compute, dict(env or {})
        self.blocks, self.layout = blocks, layout  # block-sparse: (coordinates of A's, B's, C's blocks); "own" / "strided" / "packed"
        self.padding, self.opA = padding, opA      # padded permutation: (left[], right[], value or None); a unary operator's name
        self.refuse = refuse                       # the status with which the library refuses the case (a documented limitation)
        self.strided = strided                     # block-sparse: the tensors whose descriptor carries per-block strides
        self.data_key = "%s %s %s %s" % (kind, dtype, sorted((k, str(v)) for k, v in ext.items()), modes)

    def __repr__(self):
        return self.id

    def extents(self, t):
        return [self.ext[c] for c in self.modes[t]]

    def strides(self, t):
        import guarded as gd
        return gd.packed_strides(self.extents(t), self.pad.get(t, 0))


CASES = []


def add(*a, **kw):
    c = Case(*a, **kw)
    assert all(c.id != o.id for o in CASES), c.id
    CASES.append(c)
    return c


def scalars(dtype):
    return CSCALARS if dtype in CPLX else xc.SCALARS16 if dtype in xd.H16 else xc.SCALARS32


def runs(dtype, i, where=("none", "inplace", "separate")):
    """one run per place of the beta source: beta = 0 for "none", beta != 0 for the others"""
    tab = scalars(dtype)
    zero, full = [s for s in tab if s[1] == 0], [s for s in tab if s[1] != 0]
    return [((zero if w == "none" else full)[(i + j) % 3], w) for j, w in enumerate(where)]


def align256(n):
    return (n + 255) // 256 * 256


# ---- trinary contractions ---------------------------------------------------------------------------------------------------------------
def _tri(order=None, step1=None, step2=None, more=None):
    def ok(d):
        if d.get("op") != "contraction_trinary" or d.get("intermediate_bytes", 0) <= 0 or "step1" not in d or "step2" not in d:
            return False
        return (order is None or d["order"] == list(order)) and (step1 is None or step1(d["step1"])) and (step2 is None or step2(d["step2"])) and \
            (more is None or more(d))
    return ok


def _split(s):
    return s.get("splitK", 1) > 1


def _ws_behind_t(d):
    """a split-K sub-plan's workspace lies behind the aligned intermediate"""
    return d["workspace"] > align256(d["intermediate_bytes"])


def _kname(*names):
    return lambda s: s.get("kname") in names


def trinary(name, dtype, ext, modes, expect, i=0, where=("none", "inplace", "separate"), **kw):
    add("tri_%s_%s" % (SHORT[dtype], name), "contraction_trinary", dtype, ext, modes, expect, runs(dtype, i, where), **kw)


T5 = dict(a=24, b=20, c=64, d=18, e=30)
T5_MODES = ("acd", "cb", "de", "abe")
T5_16 = dict(a=24, b=20, c=16, d=6, e=30)                      # 16-bit data: dense +-1 over 96 terms
SAMPLE = dict(m=24, a=4, b=6, n=8, r=12, k=8, i=4, j=16)       # tests/test_gpu_trinary.py::test_contraction_trinary
# one case per row of `pairs`
trinary("order_ab", "float32", T5, T5_MODES, _tri(order=(0, 1, 2)), 0)
trinary("order_ac", "float32", dict(T5, c=6, d=64), T5_MODES, _tri(order=(0, 2, 1)), 1)
trinary("order_bc", "float32", dict(a=64, b=48, c=40, d=4), ("ab", "bc", "cd", "ad"), _tri(order=(1, 2, 0)), 2)
trinary("sample", "float32", SAMPLE, ("mkajbi", "kni", "rj", "mnbra"), _tri(), 1)
# a contracted mode carried by all three inputs: T keeps k as a batch mode (L of step 1), step 2 contracts it
trinary("k_in_all", "float32", dict(a=12, b=10, c=9, k=33), ("ak", "bk", "ck", "abc"), _tri(step1=lambda s: s["L"] == 33 and s["K"] == 1, step2=lambda s: s["K"] == 33), 2)
# a batch mode in all three inputs and in E
trinary("batch_in_all", "float32", dict(l=3, a=20, k=17, b=13, c=11), ("lak", "lkb", "lbc", "lac"), _tri(step1=lambda s: s["L"] == 3, step2=lambda s: s["L"] == 3), 0)
# inputs that share no mode with each other but with the third
trinary("no_shared", "float32", dict(i=14, j=11, k=9, l=13, m=10), ("ik", "jl", "klm", "ijm"), _tri(), 1)
# a mode that only A carries and E does not: a step becomes a lone-reduce plan
trinary("lone", "float32", dict(a=20, k=17, s=5, b=13, c=11), ("aks", "kb", "bc", "ac"),
        _tri(more=lambda d: any(d[s].get("lone_reduce_A") == 1 or d[s].get("lone_reduce_B") == 1 for s in ("step1", "step2"))), 2)
# split-K in step 1 and in step 2: the sub-plan's partials behind the aligned intermediate, exactly required_workspace bytes
trinary("splitk_step1", "float32", dict(a=64, k=4096, b=16, c=64), ("ak", "kb", "bc", "ac"), _tri(order=(0, 1, 2), step1=_split, more=_ws_behind_t), 0)
trinary("splitk_step2", "float32", dict(a=8, b=8, c=64, k=4096), ("ak", "bk", "ck", "abc"), _tri(step2=_split, more=_ws_behind_t), 1)
# layout: padded pitches on all five tensors (D's differ from E's: a descriptor of its own); an odd element offset at element alignment
trinary("padded", "float32", T5, T5_MODES, _tri(order=(0, 1, 2)), 1, where=("none", "separate"), pad=dict(A=3, B=5, C=1, D=2, E=4))
trinary("padded_d_is_e", "float32", T5, T5_MODES, _tri(order=(0, 1, 2)), 2, pad=dict(A=1, B=2, C=3, D=5, E=5))
trinary("odd_offset", "float32", T5, T5_MODES, _tri(order=(0, 1, 2)), 2, off=3, align=4)
# data types
for _i, _dt in enumerate(DTYPES[1:]):
    trinary("types", _dt, T5_16 if _dt in xd.H16 else T5, T5_MODES, _tri(), _i)
    trinary("types_odd_offset", _dt, T5_16 if _dt in xd.H16 else T5, T5_MODES, _tri(), _i + 1, off=1, align=ES[_dt], pad=dict(A=1, B=1, C=1, D=1, E=1))
# conjugation, on data on which it is not a no-op
for _dt in CPLX:
    for _i, _cj in enumerate(("A", "B", "C", "D", "ABCD")):
        trinary("conj_" + _cj, _dt, dict(a=12, b=10, c=16, d=9, e=14), T5_MODES, _tri(), _i, where=("separate", "inplace"), conj=_cj)
# compute descriptors: fp32 data under the reduced ones (the pairwise steps take the reduced kernels), fp64 under 32F (they keep fp64)
for _i, _cd in enumerate(("16BF", "16F", "TF32")):
    trinary("compute_" + _cd.lower(), "float32", T5, T5_MODES, _tri(step1=_kname("gett_gen_f32x_kernel"), step2=_kname("gett_gen_f32x_kernel")), _i,
            compute=_cd, env=F32X)
trinary("compute_32f", "float64", T5, T5_MODES, _tri(step1=lambda s: s["family"] == 2 and s["kname"] == "gett_gen_kernel", step2=lambda s: s["kname"] == "gett_gen_kernel"),
        1, compute="32F")

# ---- block-sparse contractions ----------------------------------------------------------------------------------------------------------
# 'kil,kl->i' (the sample's equation): output blocks with two contributions (i0), one (i1), none (i2); a pair whose output block is absent
# (i3); sections of extent 1 (i1, k1); a mode with a single section (l).  'ik,kl->il': two free modes; two contributions (0,0), one (1,1)
# and (1,0), none (2,0), absent (0,1).  Section extents are odd: blocks packed back to back then have bases aligned to the element only.
BS1 = (("kil", "kl", "i"), ([(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 3, 0)], [(0, 0), (1, 0)], [(0,), (1,), (2,)]))
BS2 = (("ik", "kl", "il"), ([(0, 0), (0, 1), (1, 1)], [(0, 0), (1, 0), (1, 1)], [(0, 0), (1, 1), (1, 0), (2, 0)]))


def _bs(tasks, scale, split):
    return lambda d: d.get("op") == "blocksparse" and d["tasks"] == tasks and d["scale_plans"] == scale and len(d["kernels"]) >= 1 and (d["workspace"] > 0) == split


def blocksparse(name, dtype, k0, layout, i=0, **kw):
    """k0: the long section of the contracted mode (a split-K dense plan where it is long enough)"""
    split = k0 >= 1000
    for tag, (modes, blocks), ext, tasks in (("kil", BS1, dict(k=[k0, 1], i=[3, 1, 5, 7], l=[3]), 4), ("ikl", BS2, dict(i=[5, 1, 3], k=[k0, 3], l=[7, 1]), 5)):
        nA, nB = len(blocks[0]), len(blocks[1])
        pad = dict(A=[1 + j for j in range(nA)], B=[2 * (j % 2) + 1 + j for j in range(nB)]) if layout == "strided" else {}
        add("bs_%s_%s_%s" % (SHORT[dtype], tag, name), "blocksparse", dtype, ext, modes, _bs(tasks, 1, split), runs(dtype, i), blocks=blocks, layout=layout,
            pad=pad, strided="AB" if layout == "strided" else "", **kw)


for _i, _dt in enumerate(("float32", "float64", "bfloat16", "float16")):
    _short = 7 if _dt in xd.H16 else 33
    blocksparse("own", _dt, _short, "own", _i)
    blocksparse("strided", _dt, _short, "strided", _i + 1)
    blocksparse("packed", _dt, _short, "packed", _i + 2)
    if _dt not in xd.H16:         # (a section long enough for split-K: +-1 over thousands of terms leaves the 16-bit integer range)
        blocksparse("splitk", _dt, 4501, "own", _i)
        blocksparse("splitk_packed", _dt, 4501, "packed", _i + 1)
# documented limitations, asserted as the refusal status
for _dt in CPLX:
    add("bs_%s_refused" % SHORT[_dt], "blocksparse", _dt, dict(k=[7, 1], i=[3, 1, 5, 7], l=[3]), BS1[0], blocks=BS1[1], refuse=NOT_SUPPORTED)
add("bs_f32_strided_d_refused", "blocksparse", "float32", dict(k=[7, 1], i=[3, 1, 5, 7], l=[3]), BS1[0], blocks=BS1[1], refuse=NOT_SUPPORTED, strided="C",
    pad=dict(C=[1, 1, 1]))

# ---- padded permutations ----------------------------------------------------------------------------------------------------------------
PAD_RUNS = [((1.0,), "none"), ((-0.5,), "none")]


def _pp(variant=None, **more):
    def ok(d):
        if d.get("op") != "elementwise" or "pad" not in d or (variant is not None and d["variant"] != variant):
            return False
        return all(d.get(k) == v for k, v in more.items())
    return ok


def padded(name, dtype, ext, mA, mD, left, right, value, expect, **kw):
    add("pp_%s_%s" % (SHORT[dtype], name), "padded_permutation", dtype, ext, (mA, mD), expect, kw.pop("runs", PAD_RUNS), padding=(list(left), list(right), value), **kw)


def pad_geometry(case):
    """(padded extents, elements the fill writes, element offset of the interior)"""
    left, right, _ = case.padding
    full = [e + l + r for e, l, r in zip(case.extents("D"), left, right)]
    off, run = 0, 1
    for f, l in zip(full, left):
        off += l * run
        run *= f
    return full, run, off


# The inner plan is planned with the padding set, and the planner keeps EW_BLOCK and EW_TRANSPOSE_ANY for unpadded permutations
# (plan_elementwise.cpp): a padded permutation takes EW_TRANSPOSE, EW_ROWCOPY or EW_GENERIC.  One case per variant it can take, each with a
# pad offset that is a multiple of the 16-byte lane and one that is not (the interior then starts off the lanes and the inner plan loses
# the 16-byte variants: the predicate names what it takes instead); and the shapes that take EW_BLOCK / EW_TRANSPOSE_ANY without padding
# (UNPADDED_TAKES: tests/test_composite_cpu.py asserts that), with the variant they take with it.
UNPADDED_TAKES = {}
for _dt in ("float32", "bfloat16"):
    _nv = NV[_dt]
    _tr = dict(a=136, b=3, c=72)
    padded("transpose_lane", _dt, _tr, "abc", "cba", (_nv, 0, 1), (_nv, 2, 0), 7.5, _pp(EW_TRANSPOSE))
    padded("transpose_off_lane", _dt, _tr, "abc", "cba", (1, 0, 1), (2 * _nv - 1, 2, 0), -2.0, _pp(EW_GENERIC))
    padded("rowcopy_lane", _dt, dict(a=256, b=12, c=10), "abc", "acb", (2 * _nv, 1, 0), (0, 0, 2), -2.0, _pp(EW_ROWCOPY))
    padded("rowcopy_off_lane", _dt, dict(a=256, b=12, c=10), "abc", "acb", (3, 1, 0), (2 * _nv - 3, 0, 2), 7.5, _pp(EW_GENERIC))
    padded("generic_lane", _dt, dict(a=33, b=170, c=7), "abc", "acb", (_nv, 0, 1), (0, 2, 0), -2.0, _pp(EW_GENERIC), pad=dict(A=1))
    padded("generic_off_lane", _dt, dict(a=33, b=170, c=7), "abc", "acb", (1, 0, 1), (0, 2, 0), 7.5, _pp(EW_GENERIC), pad=dict(A=1))
    padded("block_shape_lane", _dt, dict(d=48, c=16, b=4, a=20), "dcba", "bcda", (0, 0, 0, 2), (0, 0, 0, 1), 7.5, _pp(EW_TRANSPOSE if _dt == "float32" else EW_GENERIC))
    padded("block_shape_off_lane", _dt, dict(d=7, c=3, b=5, a=100), "dcba", "bcda", (1, 0, 2, 0), (0, 1, 0, 3), -2.0, _pp(EW_GENERIC))
    padded("any_shape_lane", _dt, dict(a=77, b=5, c=131), "abc", "cba", (0, _nv, 0), (1, 0, 2), 7.5, _pp(EW_GENERIC), off=3, align=ES[_dt])
    padded("any_shape_off_lane", _dt, dict(a=77, b=5, c=131), "abc", "cba", (3, 1, 0), (0, 0, 2), -2.0, _pp(EW_GENERIC), off=3, align=ES[_dt])
    for _n, _v in (("block_shape_lane", EW_BLOCK), ("block_shape_off_lane", EW_BLOCK), ("any_shape_lane", EW_TRANSPOSE_ANY), ("any_shape_off_lane", EW_TRANSPOSE_ANY)):
        UNPADDED_TAKES["pp_%s_%s" % (SHORT[_dt], _n)] = _v
# data types: the wide ones on the transposing and the copying kernel; complex data with the default pad value (zero)
for _dt in ("float64", "float16", "complex64", "complex128"):
    _v = None if _dt in CPLX else 7.5
    padded("types_transpose", _dt, dict(a=136, b=3, c=72), "abc", "cba", (NV[_dt], 1, 0), (0, 0, 2), _v, _pp(EW_TRANSPOSE))
    padded("types_rowcopy", _dt, dict(a=256, b=12, c=10), "abc", "acb", (0, 1, 0), (NV[_dt], 0, 2), _v, _pp(EW_ROWCOPY))
    if _dt != "complex128":       # (a complex128 lane holds one element: every offset is a multiple of the lane)
        padded("types_off_lane", _dt, dict(a=33, b=20, c=7), "abc", "acb", (1, 0, 1), (0, 2, 0), _v, _pp(EW_GENERIC))
# pad values (16-bit data: _typed_value hands the value over as the 2 bytes of the type itself), -0.0 and +inf among them
for _dt in ("float32", "float64", "bfloat16", "float16"):
    for _n, _v in (("m0", -0.0), ("inf", float("inf"))):
        padded("value_" + _n, _dt, dict(a=33, b=20, c=7), "abc", "cab", (1, 2, 0), (2, 0, 1), _v, _pp())
# ... and the caller's own 2 bytes: bf16 -7.5 (0xC0F0), fp16 7.5 (0x4780), little-endian
padded("value_bytes", "bfloat16", dict(a=33, b=20, c=7), "abc", "cab", (1, 2, 0), (2, 0, 1), b"\xf0\xc0", _pp())
padded("value_bytes", "float16", dict(a=33, b=20, c=7), "abc", "cab", (1, 2, 0), (2, 0, 1), b"\x80\x47", _pp())
# opA = RELU with a negative pad value: the border holds the pad value untouched, only the interior is clipped (and scaled)
for _dt in ("float32", "bfloat16", "float64"):
    padded("relu", _dt, dict(a=33, b=20, c=7), "abc", "cab", (1, 2, 0), (2, 0, 1), -2.0, lambda d: _pp()(d) and d.get("unary") == [8, 1, 1], opA="RELU")
# padding patterns: left only, right only, zero on every mode, the fastest mode only, the slowest only (both sides: every case above)
for _n, _l, _r in (("left_only", (2, 1, 3), (0, 0, 0)), ("right_only", (0, 0, 0), (1, 3, 2)), ("zero", (0, 0, 0), (0, 0, 0)), ("fastest_only", (3, 0, 0), (2, 0, 0)),
                   ("slowest_only", (0, 0, 2), (0, 0, 1))):
    for _dt in ("float32", "float16"):
        padded(_n, _dt, dict(a=33, b=20, c=7), "abc", "cab", _l, _r, 7.5, _pp())
# total padded size below 16 bytes, and not a multiple of 16 bytes (the fill's tail); A with padded pitches; a D base aligned to the element only
for _dt in ("float32", "float64", "bfloat16", "float16", "complex64"):
    padded("tiny", _dt, dict(a=1), "a", "a", (0,), (0,) if ES[_dt] == 8 else (1,) if ES[_dt] == 4 else (4,), None if _dt in CPLX else 7.5, _pp())
    padded("tiny_odd_base", _dt, dict(a=1), "a", "a", (0,), (0,) if ES[_dt] == 8 else (1,) if ES[_dt] == 4 else (4,), None if _dt in CPLX else -2.0, _pp(),
           off=3 if ES[_dt] < 8 else 1, align=ES[_dt])       # (the bytes up to the first 16-byte boundary are all there is)
    padded("tail", _dt, dict(a=5, b=3), "ab", "ba", (1, 0), (1, 2), None if _dt in CPLX else -2.0, lambda d, e=ES[_dt]: _pp()(d) and d["pad"][0] * e % 16 != 0)
    padded("a_pitch", _dt, dict(a=33, b=20, c=7), "abc", "cab", (1, 2, 0), (2, 0, 1), None if _dt in CPLX else 7.5, _pp(), pad=dict(A=3))
    padded("odd_base", _dt, dict(a=33, b=20, c=7), "abc", "cab", (1, 2, 0), (2, 0, 1), None if _dt in CPLX else -2.0, _pp(), off=1, align=ES[_dt])
    padded("odd_base_tail", _dt, dict(a=5, b=3), "ab", "ba", (1, 0), (1, 2), None if _dt in CPLX else 7.5, _pp(), off=3 if ES[_dt] < 8 else 1, align=ES[_dt])
# PADDING_VALUE on complex data: a documented limitation
for _dt in CPLX:
    padded("value_refused", _dt, dict(a=33, b=20), "ab", "ba", (1, 0), (0, 1), b"\x00" * ES[_dt], None, refuse=NOT_SUPPORTED)

BY_ID = {c.id: c for c in CASES}
RUNNABLE = [c.id for c in CASES if c.refuse is None]
NO_SWITCH = [c.id for c in CASES if not c.env and c.refuse is None]


# ---- plans ----------------------------------------------------------------------------------------------------------------------------
def block_shapes(case, t):
    return wc.BlockLayout(case.ext, case.modes[t], case.blocks["ABCD".index(t) if t != "D" else 2]).shapes


def block_strides(case, t):
    import guarded as gd
    pads = case.pad.get(t) or [0] * len(block_shapes(case, t))
    return [gd.packed_strides(s, p) for s, p in zip(block_shapes(case, t), pads)]


def make_plan(ct, ops, h, case, unpadded=False):
    dt = xc._dt(ct, case.dtype)
    m, e, s, al = case.modes, case.extents, case.strides, case.align or 128
    with wc.hook_env(case):
        if case.kind == "contraction_trinary":
            op = {t: ct.OP_CONJ if t in case.conj else ct.OP_IDENTITY for t in "ABCD"}
            own_e = case.pad.get("E", 0) != case.pad.get("D", 0)
            return ops.contraction_trinary_plan(h, e("A"), m["A"], e("B"), m["B"], e("C"), m["C"], e("D"), m["D"], dtype=dt, compute=case.compute,
                                                alignment=al, strideA=s("A"), strideB=s("B"), strideC=s("C"), strideD=s("D"),
                                                strideE=s("E") if own_e else None, opA=op["A"], opB=op["B"], opC=op["C"], opD=op["D"], workspace_limit=None)
        if case.kind == "blocksparse":
            st = tuple(block_strides(case, t) if t in case.strided else None for t in "ABC")
            return ops.blocksparse_plan(h, case.ext, (m["A"], m["B"], m["C"]), case.blocks, dtype=dt, strides=st, workspace_limit=None)
        return ops.permutation_plan(h, e("A"), m["A"], e("D"), m["D"], dtype=dt, strideA=s("A"), alignment=al, padding=None if unpadded else case.padding,
                                    opA=case.opA or ct.OP_IDENTITY)


def describe(ct, plan):
    return json.loads(wc.describe(ct, plan).raw)


def plan_path(ct, ops, h, case):
    """the case's plan is on the path the case names (the planner needs no GPU); a refused case is refused with its status"""
    if case.refuse is not None:
        try:
            make_plan(ct, ops, h, case).destroy()
        except ct.CuTensorError as err:
            assert err.status == case.refuse, (case.id, err.status)
            return None
        raise AssertionError("%s was accepted (expected status %d)" % (case.id, case.refuse))
    plan = make_plan(ct, ops, h, case)
    try:
        d = describe(ct, plan)
        assert case.expect(d), "%s is off its path: %s" % (case.id, d)
        if case.kind == "padded_permutation":
            _, fill, off = pad_geometry(case)
            assert d["pad"] == [fill, off], (case.id, d["pad"], fill, off)
        return d
    finally:
        plan.destroy()


# ---- data -----------------------------------------------------------------------------------------------------------------------------
def _rng(case, draw, what):
    return np.random.default_rng([zlib.crc32(case.data_key.encode()), int(draw), what])


def _ints(rng, shape, values, cplx):
    v = np.asarray(list(values), dtype=np.int64)
    x = v[rng.integers(0, len(v), size=shape)]
    return x + 1j * v[rng.integers(0, len(v), size=shape)] if cplx else x


def _mag(x):
    return np.abs(x.real) + np.abs(x.imag)


def _part_max(x):
    return float(max(np.abs(x.real).max(), np.abs(x.imag).max())) if x.size else 0.0


def _half(scal):
    return any(float(p) != round(float(p)) for s in scal for p in (complex(s).real, complex(s).imag))


def _wide(case):
    return np.complex128 if case.dtype in CPLX else np.float64


def operand_values(case):
    """dense +-1 where an intermediate must stay a 16-bit integer (16-bit data, operands rounded to bf16), {+-1, +-2, +-3} elsewhere"""
    return (-1, 1) if case.dtype in xd.H16 or case.compute == "16BF" else (-3, -2, -1, 1, 2, 3)


def make_draw(case, draw):
    """the logical host tensors of one draw by tensor name (numpy int64, complex128 for complex data; modes in descriptor order;
    block-sparse: the dense tensors, zero where a block is absent)"""
    cplx = case.dtype in CPLX
    out = {}
    if case.kind == "padded_permutation":
        out["A"] = _ints(_rng(case, draw, 0), case.extents("A"), range(-3, 4), cplx)
        return out
    src = "D" if case.kind == "contraction_trinary" else "C"
    for i, t in enumerate("ABC" if case.kind == "contraction_trinary" else "AB"):
        out[t] = _ints(_rng(case, draw, i), bs_extents(case, t) if case.blocks else case.extents(t), operand_values(case), cplx)
    out[src] = _ints(_rng(case, draw, 7), bs_extents(case, "C") if case.blocks else case.extents("D"), range(-3, 4), cplx)
    if case.blocks:
        for t in "AB":
            keep = np.zeros(out[t].shape, dtype=bool)
            for sl in bs_layout(case, t).slices:
                keep[sl] = True
            out[t] = np.where(keep, out[t], 0)
    return out


def bs_extents(case, t):
    return [sum(case.ext[c]) for c in case.modes[t]]


def bs_layout(case, t):
    return wc.BlockLayout(case.ext, case.modes[t], case.blocks[{"A": 0, "B": 1, "C": 2, "D": 2}[t]])


# ---- trinary: reference and data rule ---------------------------------------------------------------------------------------------------
def _tri_ops(case, ins):
    return [np.conj(ins[t]) if t in case.conj else ins[t] for t in "ABC"]


def tri_reference(case, ins, scal):
    alpha, beta = scal
    m = case.modes
    acc = np.einsum("%s,%s,%s->%s" % (m["A"], m["B"], m["C"], m["E"]), *_tri_ops(case, ins), optimize=True)     # int64 (complex: complex128 of integers)
    ref = alpha * acc.astype(_wide(case))
    if beta:
        ref = ref + beta * (np.conj(ins["D"]) if "D" in case.conj else ins["D"]).astype(_wide(case))
    return ref.astype(_wide(case))


def tri_intermediates(case, ins):
    """per pair order the largest |part| of the intermediate T (modes of X and Y that Z or E still need), every sum in int64"""
    m = case.modes
    x = _tri_ops(case, ins)
    mm = [m["A"], m["B"], m["C"]]
    out = []
    for px, py, pz in PAIRS:
        both = "".join(dict.fromkeys(mm[px] + mm[py]))
        mT = "".join(c for c in both if c in mm[pz] or c in m["E"])
        if mT == both:          # nothing is summed: every entry of T is one product (no need to build it)
            out.append(_part_max(x[px]) * _part_max(x[py]) * (2 if case.dtype in CPLX else 1))
        else:
            out.append(_part_max(np.einsum("%s,%s->%s" % (mm[px], mm[py], mT), x[px], x[py], optimize=True)))
    return out


def tri_check(case, ins, scal):
    """the data rule of one run; returns the accumulator bound as a fraction of its limit"""
    alpha, beta = scal
    m = case.modes
    for (px, py, _), t in zip(PAIRS, tri_intermediates(case, ins)):
        assert t <= EXACT_LIMIT[case.dtype], "%s: the intermediate of order %s reaches %g: not a value of %s" % (case.id, (px, py), t, case.dtype)
        if case.compute in ROUNDED_BELOW:
            assert t < ROUNDED_BELOW[case.compute], "%s: the intermediate of order %s reaches %g: rounded under %s" % (case.id, (px, py), t, case.compute)
    bound = abs(complex(alpha).real) + abs(complex(alpha).imag)
    bound *= float(np.einsum("%s,%s,%s->%s" % (m["A"], m["B"], m["C"], m["E"]), *[_mag(ins[t]).astype(np.float64) for t in "ABC"], optimize=True).max())
    bound += (abs(complex(beta).real) + abs(complex(beta).imag)) * float(_mag(ins["D"]).max())
    limit = xd.acc_limit(case.dtype) / (2 if _half(scal) else 1)
    assert bound < limit, "%s: accumulator bound %g is not below %g" % (case.id, bound, limit)
    for t in case.conj:
        assert bool((ins[t].imag != 0).any()), "%s: conjugating %s is a no-op on this draw" % (case.id, t)
    if case.conj and (beta or case.conj != "D"):
        plain = Case(case.id, case.kind, case.dtype, case.ext, tuple(m[t] for t in "ABCD"), conj="" if beta else "D")
        assert not np.array_equal(tri_reference(plain, ins, scal), tri_reference(case, ins, scal)), "%s: conjugation does not show in the result" % case.id
    return bound / limit


# ---- block-sparse: tasks, reference and data rule ------------------------------------------------------------------------------------------
def bs_tasks(case):
    """(a, b, d) of every block pair that contributes to a stored output block, in the library's order (A's blocks outer, B's inner)"""
    mA, mB, mD = case.modes["A"], case.modes["B"], case.modes["D"]
    cA, cB, cD = case.blocks
    out = []
    for a, ca in enumerate(cA):
        for b, cb in enumerate(cB):
            sec = dict(zip(mA, ca))
            if any(sec.get(c, x) != x for c, x in zip(mB, cb)):
                continue
            sec.update(zip(mB, cb))
            dc = tuple(sec[c] for c in mD)
            if dc in [tuple(c) for c in cD]:
                out.append((a, b, [tuple(c) for c in cD].index(dc)))
    return out


def bs_reference(case, ins, scal):
    alpha, beta = scal
    m = case.modes
    ref = alpha * np.einsum("%s,%s->%s" % (m["A"], m["B"], m["D"]), ins["A"], ins["B"]).astype(np.float64)
    return ref + (beta * ins["C"] if beta else 0.0)


def _is_value(x, dtype):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float64)))
    return bool((xd.round_to(t, dtype) == t).all())


def bs_check(case, ins, scal):
    """every prefix of the contributions to an output block, in task order and reversed, is a value of the data type; the accumulator bound"""
    alpha, beta = scal
    m = case.modes
    la, lb, ld = (bs_layout(case, t) for t in "ABD")
    eq = "%s,%s->%s" % (m["A"], m["B"], m["D"])
    limit = xd.acc_limit(case.dtype) / (2 if _half(scal) else 1)
    worst = 0.0
    tasks = bs_tasks(case)
    for d, sl in enumerate(ld.slices):
        parts = [(np.einsum(eq, ins["A"][la.slices[a]], ins["B"][lb.slices[b]]), np.einsum(eq, np.abs(ins["A"][la.slices[a]]), np.abs(ins["B"][lb.slices[b]])))
                 for a, b, dd in tasks if dd == d]
        c = ins["C"][sl].astype(np.float64)
        for order in (parts, parts[::-1]):
            acc, mag = beta * c, abs(beta) * np.abs(c)
            for p, pm in order:
                worst = max(worst, float((abs(alpha) * pm + mag).max()))
                acc, mag = acc + alpha * p, np.abs(acc + alpha * p)
                assert _is_value(acc, case.dtype), "%s: a partial sum of output block %d is not a value of %s" % (case.id, d, case.dtype)
        total = beta * c + alpha * sum(p for p, _ in parts) if parts else beta * c
        assert np.array_equal(total, bs_reference(case, ins, scal)[sl]), (case.id, d)        # the dense reference is the sum of the stored pairs
    assert worst < limit, "%s: accumulator bound %g is not below %g" % (case.id, worst, limit)
    return worst / limit


# ---- padded permutation: reference -------------------------------------------------------------------------------------------------------
def pad_value(case):
    v = case.padding[2]
    if isinstance(v, bytes):          # 2 bytes of the type itself
        u = np.frombuffer(v, dtype=np.uint16)
        return float(u.view(np.float16)[0]) if case.dtype == "float16" else float((u.astype(np.uint32) << 16).view(np.float32)[0])
    return 0.0 if v is None else float(v)


def pp_reference(case, ins, scal):
    """(the padded buffer's exact content, the mask of its border)"""
    from ew_exact_cases import to_out
    left, right, _ = case.padding
    full, _, _ = pad_geometry(case)
    a = ins["A"].astype(_wide(case))
    if case.opA == "RELU":
        a = np.maximum(a, 0.0)
    inner = scal[0] * to_out(a, case.modes["A"], case.modes["D"])
    want = np.full(full, pad_value(case), dtype=_wide(case))
    at = tuple(slice(l, l + e) for l, e in zip(left, case.extents("D")))
    want[at] = inner
    border = np.ones(full, dtype=bool)
    border[at] = False
    return want, border


def expected(case, ref):
    """what a correct library stores — asserted ON THE REFERENCE: every exact output is a value of the data type, nothing rounds"""
    import torch
    r = torch.from_numpy(np.ascontiguousarray(ref).reshape(np.shape(ref)))
    want = xd.round_to(r, case.dtype)
    n = int((~((want == r) | (want.isnan() & r.isnan()))).sum())
    assert n == 0, "%s: %d exact outputs are not values of %s" % (case.id, n, case.dtype)
    return want


def check_case(case):
    """every draw and run of the case on the CPU: the data rule and the reference's representability; returns the runs checked"""
    n = 0
    for draw in (0, 1):
        ins = make_draw(case, draw)
        for scal, _ in case.runs:
            if case.kind == "contraction_trinary":
                tri_check(case, ins, scal)
                expected(case, tri_reference(case, ins, scal))
            elif case.kind == "blocksparse":
                bs_check(case, ins, scal)
                expected(case, bs_reference(case, ins, scal))
            else:
                want, border = pp_reference(case, ins, scal)
                expected(case, want)
                assert bool((want[border] == pad_value(case)).all()) and (border.any() or not any(case.padding[0] + case.padding[1]))
            n += 1
    return n


# ---- running a case ----------------------------------------------------------------------------------------------------------------------
def _host(case, x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x).reshape(np.shape(x))).to(xd.TORCH_DTYPES[case.dtype])


def _placed(case, t, host=None):
    p = xc.Placed(case.extents(t), case.dtype, off=case.off, strides=case.strides(t))
    if host is not None:
        p.set(_host(case, host))
    return p


def _unchanged(p, snap, what):
    import torch
    assert torch.equal(p.raw, snap), "%s was written" % what


def _workspace(plan):
    import guarded as gd
    ws = gd.guarded_workspace(plan.required_workspace, 0xFF)          # exactly required_workspace bytes between guards, at 128 (mod 256)
    return ws, (ws.ptr if plan.required_workspace else 0)


def run_trinary(ct, ops, h, case, plan, desc):
    import torch
    for draw in (0, 1):
        ins = make_draw(case, draw)
        dev = {t: _placed(case, t, ins[t]) for t in "ABC"}
        snap = {t: dev[t].raw.clone() for t in "ABC"}
        for scal, where in case.runs:
            tri_check(case, ins, scal)
            want = expected(case, tri_reference(case, ins, scal))
            pe = _placed(case, "E")                                   # 0xFF everywhere: a NaN in every type
            pd = None
            if where == "inplace":
                pe.set(_host(case, ins["D"]))
            elif where == "separate":
                pd = _placed(case, "D", ins["D"])
                dsnap = pd.raw.clone()
            ws, wsp = _workspace(plan)
            plan.contract_trinary(scal[0], dev["A"].ptr, dev["B"].ptr, dev["C"].ptr, scal[1], pd.ptr if pd else pe.ptr, pe.ptr, wsp, plan.required_workspace)
            torch.cuda.synchronize()
            what = "%s (draw %d, scalars %s, D %s) %s" % (case.id, draw, scal, where, desc)
            xd.assert_exact(pe.get(), want, what)
            pe.check_outside(what)
            ws.check(what)
            for t in "ABC":
                _unchanged(dev[t], snap[t], what + ": " + t)
            if pd is not None:
                _unchanged(pd, dsnap, what + ": D")


class PackedBlocks:
    """the blocks of a block-sparse tensor back to back in one allocation, at an odd element offset behind one guard: with odd block sizes
    the bases are aligned to the element size only"""

    def __init__(self, layout, dtype):
        self.layout = layout
        sizes = [int(np.prod(s)) for s in layout.shapes]
        self.starts = [sum(sizes[:i]) for i in range(len(sizes))]
        self.one = xc.Placed([sum(sizes)], dtype, off=1)
        self.raw = self.one.raw
        self.ptrs = (ctypes.c_void_p * len(sizes))(*[self.one.ptr + s * self.one.es for s in self.starts])

    def _view(self, i):
        shape = self.layout.shapes[i]
        st, run = [], 1
        for e in shape:
            st.append(run)
            run *= e
        v = self.one.buf.as_strided(list(reversed(shape)), list(reversed(st)), self.one.start + self.starts[i])
        return v.permute(*reversed(range(v.dim())))

    def set(self, dense):
        for i, sl in enumerate(self.layout.slices):
            self._view(i).copy_(dense[sl].to(self.one.buf.device))

    def get(self):
        import torch
        return torch.cat([self._view(i).cpu().reshape(-1) for i in range(len(self.starts))])

    def check_guard(self, what=""):
        self.one.check_outside(what)


class PlacedBlocks:
    """every block in a 0xFF-filled buffer of its own (exact_cases.Placed), its first mode's pitch padded by pads[i] elements"""

    def __init__(self, layout, dtype, pads=None):
        self.layout = layout
        self.t = [xc.Placed(s, dtype, (pads or [0] * len(layout.shapes))[i]) for i, s in enumerate(layout.shapes)]
        self.ptrs = (ctypes.c_void_p * len(self.t))(*[t.ptr for t in self.t])

    def set(self, dense):
        for sl, t in zip(self.layout.slices, self.t):
            t.set(dense[sl])

    def snapshot(self):
        return [t.raw.clone() for t in self.t]


def _bytes(b):
    return b.snapshot() if isinstance(b, PlacedBlocks) else [b.raw.clone()] if isinstance(b, PackedBlocks) else [t.raw.clone() for t in b.t]


def run_blocksparse(ct, ops, h, case, plan, desc):
    import torch
    lay = {t: bs_layout(case, t) for t in "ABD"}
    packed = case.layout == "packed"
    out = (lambda: PackedBlocks(lay["D"], case.dtype)) if packed else (lambda: wc.GuardedBlocks(lay["D"], case.dtype))
    for draw in (0, 1):
        ins = make_draw(case, draw)
        dev = {t: PackedBlocks(lay[t], case.dtype) if packed else PlacedBlocks(lay[t], case.dtype, case.pad.get(t)) for t in "AB"}
        for t in "AB":
            dev[t].set(_host(case, ins[t]))
        snap = {t: _bytes(dev[t]) for t in "AB"}
        for scal, where in case.runs:
            bs_check(case, ins, scal)
            ref = expected(case, bs_reference(case, ins, scal))
            want = torch.cat([ref[sl].reshape(-1) for sl in lay["D"].slices])
            D, C = out(), None
            if where == "inplace":
                D.set(_host(case, ins["C"]))
            elif where == "separate":
                C = out()
                C.set(_host(case, ins["C"]))
                csnap = _bytes(C)
            ws, wsp = _workspace(plan)
            al, be = plan.scalar(scal[0]), plan.scalar(scal[1])
            ct.check(ct.cutensorBlockSparseContract(h.h, plan.plan, ctypes.byref(al), dev["A"].ptrs, dev["B"].ptrs, ctypes.byref(be),
                                                    (C or D).ptrs, D.ptrs, wsp or None, plan.required_workspace, None))
            torch.cuda.synchronize()
            what = "%s (draw %d, scalars %s, C %s) %s" % (case.id, draw, scal, where, desc)
            xd.assert_exact(D.get(), want, what)
            D.check_guard(what)
            ws.check(what)
            for t in "AB":
                assert all(torch.equal(x, y) for x, y in zip(_bytes(dev[t]), snap[t])), "%s: %s was written" % (what, t)
            if C is not None:
                assert all(torch.equal(x, y) for x, y in zip(_bytes(C), csnap)), "%s: C was written" % what


def run_padded(ct, ops, h, case, plan, desc):
    import torch
    full, _, _ = pad_geometry(case)
    for draw in (0, 1):
        ins = make_draw(case, draw)
        pa = _placed(case, "A", ins["A"])
        snap = pa.raw.clone()
        for scal, _ in case.runs:
            ref, border = pp_reference(case, ins, scal)
            want = expected(case, ref)
            pd = xc.Placed(full, case.dtype, off=case.off)             # sized to the padded extents, inside guards
            plan.permute(scal[0], pa.ptr, pd.ptr)
            torch.cuda.synchronize()
            what = "%s (draw %d, alpha %s) %s" % (case.id, draw, scal[0], desc)
            got = pd.get()
            xd.assert_exact(got, want, what)
            if not got.is_complex() and border.any():                  # the border holds the pad value itself: -0.0 stays -0.0
                b = torch.from_numpy(border)
                assert bool((torch.signbit(got[b]) == bool(np.signbit(pad_value(case)))).all()), "%s: the sign of the border's zeros" % what
            pd.check_outside(what)
            _unchanged(pa, snap, what + ": A")


def run_case(ct, ops, h, case):
    if case.refuse is not None:
        return plan_path(ct, ops, h, case)
    plan = make_plan(ct, ops, h, case)
    try:
        d = describe(ct, plan)
        assert case.expect(d), "%s is off its path: %s" % (case.id, d)
        {"contraction_trinary": run_trinary, "blocksparse": run_blocksparse, "padded_permutation": run_padded}[case.kind](ct, ops, h, case, plan, d)
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
