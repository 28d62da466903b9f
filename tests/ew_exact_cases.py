"""The case table of the exact element-wise and reduction tests (tests/test_ew_exact_cpu.py plans every case and checks every draw,
tests/test_gpu_ew_exact.py runs every case) — a helper module, not a conftest, the sibling of tests/exact_cases.py for the other four entry
points: cutensorPermute, cutensorElementwiseBinaryExecute, cutensorElementwiseTrinaryExecute and cutensorReduce.

One case is one plan: kind, data type, extents, modes, operator(s), padded pitches per tensor, element offset and descriptor alignment, and
a predicate on the plan's description that proves the path.  A case carries its `runs`: scalars and where C lives ("inplace": C is D,
"separate": a buffer of its own, "none": no C term is read — D, which is then also passed as C, holds NaN).  Every tensor sits in a
NaN-filled buffer (exact_cases.Placed); after each launch D is compared with zero tolerance, everything outside D's elements (padding,
guards) must still be NaN, and a separate C must be unchanged.

Data (all of it integer-valued or powers of two, so that any correct kernel — any tile, split or order of combination — is exact):
  * permutation / binary / trinary: integers in [-3, 3] (complex: both parts), scalars from {+-1, +-2, +-0.5}.
  * ADD reductions: dense {+-1, +-2, +-3}; 16-bit data dense +-1 with signs flipped, first entries of a line first, until alpha * sum +
    beta * c lies in the type's exact integer range (256 for bf16, 2048 for fp16).  C: integers in [-3, 3].  |alpha| sum|a| + |beta c| is
    asserted below 2^24 / 2^53 (one binary digit less when a scalar is a half).
  * MAX / MIN: base values in [-3, 3] and one spike per kept element (+100 / -100).  Over the draws of a case the spikes cover reduced
    index 0 and red - 1, both sides of every split boundary j * redPerSplit (read from the description) and one position in each of the
    8-row, 4-row and single-row parts of the first and the last split (forced_positions), the rest go to (k * 7 + draw * 101) mod red.  The
    last draw is shifted by -200 (MAX) / +200 (MIN): all-negative / all-positive data, on which a zero identity or zero partial shows.
  * MUL: dense -1 with at most 10 entries of -2 and 10 of -0.5 per reduced line (16-bit: 4 and 2): every partial product is a power of two
    within 2^+-10, a dropped or doubled factor flips the sign or changes the magnitude.  Complex: factors from {-1, i, -i} and up to 10
    entries of +-2.
References are numpy on int64 / float64.  expected() asserts ON THE REFERENCE that every output is a value of the data type: nothing
rounds, so the comparison needs no rounding rule.

Kernels no case reaches:
  * reduce_generic_cplx_kernel<double> and ew_generic_cplx_kernel<double>: a complex128 lane holds one element, so every 16-byte-aligned
    complex128 tensor with a stride-1 mode is taken by the tiled kernels (RED_COL / RED_ROW; EW_TRANSPOSE / EW_ROWCOPY).  The generic
    kernels would need a descriptor alignment below 16 — cutensorCreateTensorDescriptor refuses an alignment below the element size
    (INVALID_VALUE) — or a tensor without a stride-1 mode, which packed and padded layouts do not have."""
import os
import sys
import zlib

import numpy as np

import exact_cases as xc
import exact_data as xd
import workspace_cases as wc

EW_TRANSPOSE, EW_ROWCOPY, EW_GENERIC, EW_BLOCK, EW_TRANSPOSE_ANY = 0, 1, 2, 3, 4
RED_COL, RED_ROW, RED_GENERIC = 0, 1, 2
NV = {"float32": 4, "float64": 2, "bfloat16": 8, "float16": 8, "complex64": 2, "complex128": 1}       # elements of a 16-byte lane
SHORT = {"float32": "f32", "float64": "f64", "bfloat16": "bf16", "float16": "f16", "complex64": "c64", "complex128": "c128"}
CPLX = ("complex64", "complex128")
EXACT_INT = {"bfloat16": 256, "float16": 2048}
LANES_ONLY = {"CUTENSOR_AMD_EW_ANY": "0"}          # hooks flavour: transpositions of small tensors stay on the 16-byte-lane kernels
TENSORS = {"permutation": "AD", "binary": "ACD", "trinary": "ABCD", "reduction": "AD"}
MAX_DRAWS = 16


class Case:
    def __init__(self, id, kind, dtype, ext, modes, expect, runs, op="ADD", pad=None, off=0, align=None, env=None, conj=(False, False),
                 compute=None):
        self.id, self.kind, self.dtype, self.ext, self.expect, self.runs = id, kind, dtype, ext, expect, list(runs)
        self.modes = dict(zip(TENSORS[kind], modes))
        self.op = op                                  # reduction / binary: one operator; trinary: (opAB, opABC)
        self.pad = dict(pad or {})                    # tensor -> elements added to the first mode's extent, or one number per mode
        self.off, self.align, self.env = off, align, dict(env or {})
        self.conjA, self.conjC = conj
        self.compute = compute
        self.data_key = "%s %s %s %s" % (kind, dtype, sorted(ext.items()), modes)

    def __repr__(self):
        return self.id

    def extents(self, t):
        return [self.ext[c] for c in self.modes[t]]

    def strides(self, t):
        e, p = self.extents(t), self.pad.get(t, 0)
        p = list(p) if isinstance(p, (tuple, list)) else [p] + [0] * len(e)
        s, run = [], 1
        for i, x in enumerate(e):
            s.append(run)
            run *= x + p[i]
        return s


CASES = []


def add(*a, **kw):
    c = Case(*a, **kw)
    assert all(c.id != o.id for o in CASES), c.id
    CASES.append(c)
    return c


def _is(**want):
    """the description has these values; splitR / tile0 / E0 may be given as a (low, high) range"""
    def ok(d):
        for k, v in want.items():
            g = d.get(k)
            if g is None or (not (v[0] <= g <= v[1]) if isinstance(v, tuple) else g != v):
                return False
        return True
    return ok


# ---- reductions ----------------------------------------------------------------------------------------------------------------------
def _red_runs(op, dtype, i):
    """ADD: C identical to D, C a separate buffer, beta = 0 over a NaN D; the other operators: beta = 0 over NaN, and C identical to D"""
    tab = xc.SCALARS16 if dtype in xd.H16 else xc.SCALARS32
    zero = [s for s in tab if s[1] == 0.0]
    full = [s for s in tab if s[1] != 0.0]
    runs = [(zero[i % len(zero)], "none"), (full[i % len(full)], "inplace")]
    if op == "ADD":
        runs.append((full[(i + 1) % len(full)], "separate"))
    return runs


def reductions(name, dtype, ext, mA, mD, expect, ops=None, **kw):
    for i, op in enumerate(ops or (("ADD", "MUL") if dtype in CPLX else ("ADD", "MUL", "MAX", "MIN"))):
        add("%s_red_%s_%s" % (SHORT[dtype], name, op.lower()), "reduction", dtype, ext, (mA, mD), lambda d, e=expect: d.get("op") == "reduction" and e(d),
            _red_runs(op, dtype, i + len(name)), op=op, **kw)


SPLIT = (2, 4096)
# RED_COL fp32 without a split: the 8-, 4- and single-row loops (45 = 5 x 8 + 4 + 1); A's pitch padded; D's pitch padded
reductions("col", "float32", dict(a=64, b=45, c=24), "abc", "ac", _is(variant=RED_COL, splitR=1))
reductions("col_padA", "float32", dict(a=64, b=45, c=24), "abc", "ac", _is(variant=RED_COL, splitR=1), pad={"A": 4})
reductions("col_padD", "float32", dict(a=64, b=45, c=24), "abc", "ac", _is(variant=RED_COL, splitR=1), pad={"D": 1}, off=4, align=16)
# several reduced digits that do not fuse (A's h pitch padded): every row of the unrolled loops is decoded (rd_offset)
reductions("col_digits", "float32", dict(m=40, h=9, k=7, v=12), "mhkv", "mv", _is(variant=RED_COL), pad={"A": (0, 4, 0, 0)})
reductions("col_split", "float32", dict(a=8, b=67), "ab", "a", _is(variant=RED_COL, splitR=2))                # the last split is ragged
reductions("row", "float32", dict(a=4096, b=6), "ab", "b", _is(variant=RED_ROW, splitR=1))
reductions("row_scalar", "float32", dict(a=64, b=48), "ab", "", _is(variant=RED_ROW, splitR=1))
reductions("row_split", "float32", dict(a=16388, b=3), "ab", "b", _is(variant=RED_ROW, splitR=SPLIT))
reductions("row_split_padA", "float32", dict(a=16388, b=3), "ab", "b", _is(variant=RED_ROW, splitR=SPLIT), pad={"A": 12})
reductions("gen_split", "float32", dict(a=33, b=131), "ab", "a", _is(variant=RED_GENERIC, rowAny=0, splitR=2))          # a lane per kept element
reductions("gen_digits", "float32", dict(a=33, b=7, c=5, e=3), "abce", "ac", _is(variant=RED_GENERIC, rowAny=0), pad={"A": (0, 2, 1, 0)}, off=3, align=4)
reductions("rowany", "float32", dict(a=77, b=5, c=3), "abc", "bc", _is(variant=RED_GENERIC, rowAny=1, splitR=1))
reductions("rowany_split", "float32", dict(a=8195, b=3), "ab", "b", _is(variant=RED_GENERIC, rowAny=1, splitR=SPLIT))
reductions("rowany_digits", "float32", dict(a=131, b=9, c=7), "abc", "c", _is(variant=RED_GENERIC, rowAny=1), pad={"A": 3}, off=1, align=4)
# fp32 data accumulated in fp64 (launch_generic_t<float, double>, double partials, reduce_finalize_kernel<float, double>)
reductions("acc64_gen_split", "float32", dict(a=64, b=131), "ab", "a", lambda d: _is(variant=RED_GENERIC, rowAny=0, splitR=SPLIT)(d) and d.get("workspace") == d.get("splitR") * 64 * 8,
           compute="64F")
reductions("acc64_rowany_split", "float32", dict(a=16388, b=3), "ab", "b", lambda d: _is(variant=RED_GENERIC, rowAny=1, splitR=SPLIT)(d) and d.get("workspace") == d.get("splitR") * 3 * 8,
           compute="64F")
# the wide kernels: the same shapes, the extents scaled to each type's lane
for _dt in ("float64", "bfloat16", "float16", "complex64", "complex128"):
    _nv = NV[_dt]
    _a = 16 * _nv
    reductions("col", _dt, dict(a=_a, b=45, c=24), "abc", "ac", _is(variant=RED_COL, splitR=1))
    reductions("col_pad", _dt, dict(a=_a, b=45, c=6), "abc", "ac", _is(variant=RED_COL, splitR=1), pad={"A": _nv, "D": 1})
    reductions("col_split", _dt, dict(a=8, b=67), "ab", "a", _is(variant=RED_COL, splitR=SPLIT))
    reductions("row", _dt, dict(a=1024 * _nv, b=6), "ab", "b", _is(variant=RED_ROW, splitR=1))
    reductions("row_scalar", _dt, dict(a=16 * _nv, b=48), "ab", "", _is(variant=RED_ROW, splitR=1))
    reductions("row_split", _dt, dict(a=16392 if _nv == 8 else 16388, b=3), "ab", "b", _is(variant=RED_ROW, splitR=SPLIT))
# complex128 at odd extents is still tiled (a lane holds one element): RED_COL, splitR 4, reduce_finalize_cplx_kernel<double>
reductions("col_odd_split", "complex128", dict(a=33, b=131), "ab", "a", _is(variant=RED_COL, splitR=4))
# the complex element-gather kernel and its finalize, with conjugation of A and of C
reductions("gen_split", "complex64", dict(a=33, b=131), "ab", "a", _is(variant=RED_GENERIC, splitR=2))
reductions("gen_split_conjA", "complex64", dict(a=33, b=131), "ab", "a", _is(variant=RED_GENERIC, splitR=2), conj=(True, False))
reductions("gen_split_conjC", "complex64", dict(a=33, b=131), "ab", "a", _is(variant=RED_GENERIC, splitR=2), conj=(False, True))
reductions("col_conjAC", "complex64", dict(a=32, b=45, c=6), "abc", "ac", _is(variant=RED_COL), conj=(True, True))
for _dt in ("bfloat16", "float16", "float64"):
    reductions("rowany", _dt, dict(a=77, b=5, c=3), "abc", "bc", _is(variant=RED_GENERIC, rowAny=1))
    reductions("gen", _dt, dict(a=33, b=7, c=5), "abc", "ac", _is(variant=RED_GENERIC, rowAny=0))
    reductions("gen_split", _dt, dict(a=33, b=131), "ab", "a", _is(variant=RED_GENERIC, rowAny=0, splitR=2))
    reductions("rowany_split", _dt, dict(a=8195, b=3), "ab", "b", _is(variant=RED_GENERIC, rowAny=1, splitR=SPLIT))

# ---- permutation / binary / trinary ---------------------------------------------------------------------------------------------------
EW_SCALARS = [(1.0, 1.0, 1.0), (-2.0, 0.5, -1.0), (0.5, -1.0, 2.0), (-1.0, 2.0, -0.5), (2.0, -0.5, 1.0), (-0.5, -2.0, -2.0)]
BINOPS = ("ADD", "MUL", "MAX", "MIN")
TRIOPS = (("ADD", "ADD"), ("MUL", "ADD"), ("ADD", "MUL"), ("MAX", "MIN"), ("MIN", "MAX"))          # test_combiners' pairs and (ADD, ADD)


def permutation(name, dtype, ext, mA, mD, expect, **kw):
    add("%s_perm_%s" % (SHORT[dtype], name), "permutation", dtype, ext, (mA, mD), lambda d, e=expect: d.get("op") == "elementwise" and d.get("form") is None and e(d),
        [((1.0,), "none"), ((-0.5,), "none")], **kw)


def binary(name, dtype, ext, mA, mC, mD, expect, ops=None, **kw):
    """C in place (where C has D's layout) and C in a buffer of its own; ADD also with gamma = 0 and NaN where C would be"""
    same = mC == mD and kw.get("pad", {}).get("C", 0) == kw.get("pad", {}).get("D", 0)
    for i, op in enumerate(ops or (("ADD", "MUL") if dtype in CPLX else BINOPS)):
        s = EW_SCALARS[(i + len(name)) % 6]
        runs = [((s[0], s[2]), "separate")] + ([((s[1], s[0]), "inplace")] if same else []) + ([((s[2], 0.0), "none")] if op == "ADD" and same else [])
        add("%s_bin_%s_%s" % (SHORT[dtype], name, op.lower()), "binary", dtype, ext, (mA, mC, mD), lambda d, e=expect: d.get("op") == "elementwise" and d.get("form") is None and e(d),
            runs, op=op, **kw)


def trinary(name, dtype, ext, mA, mB, mC, mD, expect, ops=TRIOPS, **kw):
    """every form with C identical to D and with C in a buffer of its own"""
    same = mC == mD and kw.get("pad", {}).get("C", 0) == kw.get("pad", {}).get("D", 0)
    for i, op in enumerate(ops):
        s, s2 = EW_SCALARS[(i + len(name)) % 6], EW_SCALARS[(i + len(name) + 3) % 6]
        add("%s_tri_%s_%s_%s" % (SHORT[dtype], name, op[0].lower(), op[1].lower()), "trinary", dtype, ext, (mA, mB, mC, mD),
            lambda d, e=expect: d.get("op") == "elementwise" and d.get("form") == "trinary" and e(d), ([(s, "inplace")] if same else []) + [(s2, "separate")], op=op, **kw)


# EW_TRANSPOSE fp32, tiles of 64 / 128 / 256 along dim0, interior and edge tiles; padded A and D pitches (multiples of 4)
for _n, _ext, _t0 in (("t64", dict(a=72, b=3, c=132), 64), ("t256", dict(a=68, b=2, c=256), 256), ("t128", dict(a=72, b=3, c=128), 128)):
    permutation("transpose_" + _n, "float32", _ext, "abc", "cba", _is(variant=EW_TRANSPOSE, tile0=_t0), env=LANES_ONLY)
    permutation("transpose_%s_pad" % _n, "float32", _ext, "abc", "cba", _is(variant=EW_TRANSPOSE, tile0=_t0), env=LANES_ONLY, pad={"A": 4, "D": 8}, off=4, align=16)
    binary("transpose_" + _n, "float32", _ext, "abc", "cba", "cba", _is(variant=EW_TRANSPOSE, tile0=_t0))
# ... with a C whose fastest mode is not D's (sC0 != 1), and a padded C
binary("transpose_c_order", "float32", dict(a=72, b=4, c=132), "cba", "cab", "abc", _is(variant=EW_TRANSPOSE))
binary("transpose_c_pad", "float32", dict(a=72, b=3, c=132), "abc", "cba", "cba", _is(variant=EW_TRANSPOSE), pad={"A": 4, "C": 4, "D": 8})
# EW_ROWCOPY: fp32, 16-bit, wide
for _dt in ("float32", "bfloat16", "float16", "float64", "complex64", "complex128"):
    permutation("rowcopy", _dt, dict(a=256, b=12, c=10), "abc", "acb", _is(variant=EW_ROWCOPY))
    permutation("rowcopy_pad", _dt, dict(a=256, b=12, c=10), "abc", "acb", _is(variant=EW_ROWCOPY), pad={"A": 8, "D": 16})
    binary("rowcopy_pad", _dt, dict(a=256, b=12, c=10), "abc", "acb", "acb", _is(variant=EW_ROWCOPY), pad={"A": 8, "C": 16, "D": 16})
# one fused mode >= 8192, cut into rows (E0 in [256, 4096], E1 = E / E0)
binary("flat_row_cut", "float32", dict(a=12288), "a", "a", "a", lambda d: _is(variant=EW_ROWCOPY, E0=(256, 4096))(d) and d.get("E0") * d.get("E1") == 12288)
permutation("flat_row_cut", "bfloat16", dict(a=64, b=256), "ab", "ab", lambda d: _is(variant=EW_ROWCOPY, E0=(256, 4096))(d) and d.get("E0") * d.get("E1") == 16384)
# EW_GENERIC: permutation, and the binary form at extents the element-wise transposer refuses (E0 < 16)
for _dt in ("float32", "bfloat16", "float64", "complex64"):
    permutation("generic", _dt, dict(a=33, b=170, c=7), "abc", "acb", _is(variant=EW_GENERIC), pad={"A": 1, "D": 2}, off=3, align=16 // NV[_dt])
    binary("generic_small", _dt, dict(a=9, b=35, c=13), "cba", "abc", "abc", _is(variant=EW_GENERIC), off=1, align=16 // NV[_dt])
binary("generic_c_order", "float32", dict(a=9, b=35, c=13), "cba", "bac", "abc", _is(variant=EW_GENERIC), pad={"C": 1})
# EW_BLOCK: vector and scalar lanes, a padded outer mode on both sides (the shapes of test_block_permutation_bit_exact_at_alpha_one, shrunk)
for _dt in ("float32", "bfloat16", "float16"):
    permutation("block_vec", _dt, dict(d=48, c=16, b=4, a=20), "dcba", "bcda", _is(variant=EW_BLOCK))
    permutation("block_scalar", _dt, dict(d=7, c=3, b=5, a=100), "dcba", "bcda", _is(variant=EW_BLOCK))
    permutation("block_pad", _dt, dict(d=24, c=10, b=6, a=17), "dcba", "bcda", _is(variant=EW_BLOCK), pad={"A": (0, 0, 5, 0), "D": (0, 0, 9, 0)})
    permutation("block_pad_vec", _dt, dict(d=24, c=10, b=8, a=17), "dcba", "bcda", _is(variant=EW_BLOCK), pad={"A": (0, 0, 8, 0), "D": (0, 0, 16, 0)})
# EW_TRANSPOSE_ANY: element form (with and without C) and the 16-bit pair form; descriptor alignment 4 / 2 at an odd element offset
permutation("any", "float32", dict(a=77, b=5, c=131), "abc", "cba", _is(variant=EW_TRANSPOSE_ANY, tile0=64), off=3, align=4)
permutation("any_pad", "float32", dict(a=77, b=5, c=131), "abc", "cba", _is(variant=EW_TRANSPOSE_ANY, tile0=64), off=3, align=4, pad={"A": 3, "D": 1})
binary("any", "float32", dict(a=77, b=5, c=131), "abc", "cba", "cba", _is(variant=EW_TRANSPOSE_ANY, tile0=64), off=3, align=4)
binary("any_pad", "float32", dict(a=77, b=5, c=131), "abc", "cba", "cba", _is(variant=EW_TRANSPOSE_ANY, tile0=64), off=3, align=4, pad={"A": 3, "C": 1, "D": 1})
for _dt in ("bfloat16", "float16"):
    permutation("any", _dt, dict(a=77, b=5, c=131), "abc", "cba", _is(variant=EW_TRANSPOSE_ANY, tile0=64), off=3, align=2)
    permutation("any_pair", _dt, dict(a=130, b=3, c=134), "abc", "cba", _is(variant=EW_TRANSPOSE_ANY, tile0=128), off=2, align=4)
    permutation("any_pair_pad", _dt, dict(a=130, b=3, c=134), "abc", "cba", _is(variant=EW_TRANSPOSE_ANY, tile0=128), off=2, align=4, pad={"A": 2, "D": 6})
    binary("any", _dt, dict(a=77, b=5, c=131), "abc", "cba", "cba", _is(variant=EW_TRANSPOSE_ANY, tile0=64), off=3, align=2)
    # 16-bit EW_TRANSPOSE, narrow and wide tiles (the shapes of test_16bit_vector_permutes_are_exact)
    permutation("transpose_narrow", _dt, dict(a=136, b=3, c=72), "abc", "cba", _is(variant=EW_TRANSPOSE, tile0=64), env=LANES_ONLY)
    permutation("transpose_narrow_pad", _dt, dict(a=136, b=3, c=72), "abc", "cab", _is(variant=EW_TRANSPOSE, tile0=64), env=LANES_ONLY, pad={"A": 8, "D": 16})
    permutation("transpose_w256", _dt, dict(a=128, b=2, c=256), "abc", "cba", _is(variant=EW_TRANSPOSE, tile0=256))
    permutation("transpose_w128", _dt, dict(a=64, b=3, c=128), "abc", "cab", _is(variant=EW_TRANSPOSE, tile0=128))
    binary("transpose_narrow", _dt, dict(a=136, b=3, c=72), "abc", "cba", "cba", _is(variant=EW_TRANSPOSE, tile0=64))
    binary("transpose_w128", _dt, dict(a=64, b=3, c=128), "abc", "cba", "cba", _is(variant=EW_TRANSPOSE, tile0=128))
# 8- and 16-byte elements: transposition (edge tiles), padded, with conj(A)
for _dt in ("float64", "complex64", "complex128"):
    permutation("transpose", _dt, dict(a=130, b=3, c=66), "abc", "cba", _is(variant=EW_TRANSPOSE))
    permutation("transpose_pad", _dt, dict(a=130, b=3, c=66), "abc", "cba", _is(variant=EW_TRANSPOSE), pad={"A": 2, "D": 4})
    binary("transpose", _dt, dict(a=130, b=3, c=66), "abc", "cba", "cba", _is(variant=EW_TRANSPOSE))
    if _dt in CPLX:
        permutation("transpose_conjA", _dt, dict(a=130, b=3, c=66), "abc", "cba", _is(variant=EW_TRANSPOSE), conj=(True, False))
        binary("transpose_conjAC", _dt, dict(a=130, b=3, c=66), "abc", "cba", "cba", _is(variant=EW_TRANSPOSE), conj=(True, True))
        if _dt == "complex64":      # (a complex128 lane holds one element: at the 16-byte alignment its descriptor needs, it is always tiled)
            binary("generic_conjA", _dt, dict(a=33, b=7, c=5), "abc", "cba", "cba", _is(variant=EW_GENERIC), conj=(True, False))
# a mode of D absent from A (stride 0: broadcast)
binary("broadcast", "float32", dict(a=20, b=12), "b", "ab", "ab", lambda d: True)

# trinary: one pass with E = A / E = B
T1 = dict(a=132, b=36, c=20)
trinary("e_is_a", "float32", T1, "abc", "cab", "abc", "abc", _is(passes=1, bothPermuted=0, swapAB=0))
trinary("e_is_b", "float32", T1, "cab", "abc", "abc", "abc", _is(passes=1, bothPermuted=0, swapAB=1))
trinary("e_is_a_c_order", "float32", T1, "abc", "cab", "bca", "abc", _is(passes=1, bothPermuted=0, swapAB=0), ops=TRIOPS[:2])
# one pass, two tiles (tile0 64 / 128), edge tiles; padded pitches
trinary("two_tiles_64", "float32", dict(a=132, b=8, c=68), "cba", "cab", "abc", "abc", _is(passes=1, bothPermuted=1, tile0=64))
trinary("two_tiles_128", "float32", dict(a=520, b=4, c=76), "cba", "cab", "abc", "abc", _is(passes=1, bothPermuted=1, tile0=128))
trinary("two_tiles_pad", "float32", dict(a=132, b=8, c=68), "cba", "cab", "abc", "abc", _is(passes=1, bothPermuted=1), pad={"A": 4, "B": 8, "C": 4, "D": 4},
        ops=TRIOPS[:3])
# two passes — with C identical to D the single launch of the element-gather kernel runs instead (variant_inplace).  16-bit data: the two
# passes round alpha * perm(A) to the data type in between; on this data alpha * a is a value of the type, so that changes nothing
for _dt in ("float32", "float64", "bfloat16", "float16"):
    trinary("two_pass", _dt, dict(a=68, b=33, c=12), "cba", "bac", "abc", "abc", _is(passes=2, variant_inplace=EW_GENERIC))
    trinary("two_pass_ragged", _dt, dict(a=66, b=35, c=44), "cba", "cab", "abc", "abc", _is(passes=2, variant_inplace=EW_GENERIC), ops=TRIOPS[:2])
trinary("two_pass_pad", "float32", dict(a=68, b=33, c=12), "cba", "bac", "abc", "abc", _is(passes=2, variant_inplace=EW_GENERIC),
        pad={"A": 3, "B": 1, "C": 2, "D": 2}, ops=TRIOPS[:3])
trinary("two_pass_pad", "bfloat16", dict(a=68, b=33, c=12), "cba", "bac", "abc", "abc", _is(passes=2, variant_inplace=EW_GENERIC),
        pad={"A": 3, "B": 1, "C": 2, "D": 2}, ops=TRIOPS[:3], off=1, align=2)
# a mode of D absent from B (stride 0): plans as the two-tile form
trinary("broadcast", "float32", dict(a=20, b=12), "ba", "b", "ab", "ab", lambda d: True)

BY_ID = {c.id: c for c in CASES}
NO_SWITCH = [c.id for c in CASES if not c.env]


# ---- plans ----------------------------------------------------------------------------------------------------------------------------
def _binary_plan(ct, ops, h, case, dt):
    """ops.binary_plan where C has D's descriptor; else the ABI with descriptors of their own for C and D"""
    import ctypes
    m, e, s = case.modes, case.extents, case.strides
    conj = [ct.OP_CONJ if c else ct.OP_IDENTITY for c in (case.conjA, case.conjC)]
    if m["C"] == m["D"] and s("C") == s("D"):
        return ops.binary_plan(h, e("A"), m["A"], e("D"), m["D"], op=case.op, dtype=dt, alignment=case.align or 128, opA=conj[0], opC=conj[1],
                               strideA=s("A"), strideC=s("D"))
    dA, dC, dD = (ops.tensor_descriptor(h, e(t), s(t), dt, case.align or 128) for t in "ACD")
    opd = ctypes.c_void_p()
    st = ct.cutensorCreateElementwiseBinary(h.h, ctypes.byref(opd), dA, ct.i32(m["A"]), conj[0], dC, ct.i32(m["C"]), conj[1], dD, ct.i32(m["D"]),
                                            ops._OPS[case.op], ct.compute_desc(ops._DTYPE_COMPUTE[dt]))
    for d in (dA, dC, dD):
        ct.cutensorDestroyTensorDescriptor(d)
    ct.check(st)
    return ops.Plan(h, opd, "binary", dt, workspace_limit=0)


def make_plan(ct, ops, h, case):
    dt = xc._dt(ct, case.dtype)
    m, e, s, al = case.modes, case.extents, case.strides, case.align or 128
    conjA, conjC = (ct.OP_CONJ if c else ct.OP_IDENTITY for c in (case.conjA, case.conjC))
    with wc.hook_env(case):
        if case.kind == "permutation":
            return ops.permutation_plan(h, e("A"), m["A"], e("D"), m["D"], dtype=dt, strideA=s("A"), strideB=s("D"), alignment=al, opA=conjA)
        if case.kind == "binary":
            return _binary_plan(ct, ops, h, case, dt)
        if case.kind == "trinary":
            return ops.trinary_plan(h, e("A"), m["A"], e("B"), m["B"], e("C"), m["C"], e("D"), m["D"], opAB=case.op[0], opABC=case.op[1], dtype=dt,
                                    alignment=al, strideA=s("A"), strideB=s("B"), strideC=s("C"), strideD=s("D"))
        return ops.reduction_plan(h, e("A"), m["A"], e("D"), m["D"], dtype=dt, strideA=s("A"), strideC=s("D"), op_reduce=ops._OPS[case.op],
                                  compute=case.compute, alignment=al, opA=conjA, opC=conjC, workspace_limit=1 << 24)


def plan_path(ct, ops, h, case):
    """the case's plan is on the path the case names (the planner needs no GPU); returns the description"""
    plan = make_plan(ct, ops, h, case)
    try:
        d = wc.describe(ct, plan)
        assert case.expect(d), "%s is off its path: %s" % (case.id, d)
        return {k: v for k, v in d.pairs}
    finally:
        plan.destroy()


# ---- data ------------------------------------------------------------------------------------------------------------------------------
def _rng(case, draw, what):
    return np.random.default_rng([zlib.crc32(case.data_key.encode()), int(draw), what])


def _ints(rng, shape, values, cplx):
    v = np.asarray(values, dtype=np.int64)
    x = v[rng.integers(0, len(v), size=shape)]
    return x + 1j * v[rng.integers(0, len(v), size=shape)] if cplx else x


def _red_axes(case):
    mA, mD = case.modes["A"], case.modes["D"]
    return [i for i, c in enumerate(mA) if c in mD], [i for i, c in enumerate(mA) if c not in mD]


def _lines(case):
    """(kept elements, reduced elements per kept one, the axis order that makes A a [kept][reduced] matrix with the first mode fastest)"""
    kept, red = _red_axes(case)
    e = case.extents("A")
    return int(np.prod([e[i] for i in kept])) if kept else 1, int(np.prod([e[i] for i in red])), kept[::-1] + red[::-1]


def _from_lines(case, A2):
    """[kept][reduced] (column-major linear indices over the kept / the reduced modes in A's order) -> A with its modes in descriptor order"""
    _, _, perm = _lines(case)
    e = case.extents("A")
    return np.ascontiguousarray(np.transpose(A2.reshape([e[i] for i in perm]), np.argsort(perm)))


def _kept_linear(case, X):
    """a tensor with D's modes -> its values by the kept linear index of _lines"""
    mA, mD = case.modes["A"], case.modes["D"]
    order = [mD.index(c) for c in mA if c in mD]
    return np.transpose(X, order[::-1]).reshape(-1)


def forced_positions(red, splitR, per):
    """reduced indices a spike must visit: the ends, both sides of every split boundary, and one index in each of the 8-row, 4-row and
    single-row parts of the first and of the last split (reduce.hip: r + 8 <= rEnd, r + 4 <= rEnd, r < rEnd)"""
    pos = {0, red - 1}
    for j in range(1, splitR):
        pos |= {j * per - 1, j * per}
    for b, e in ((0, min(per, red)), ((splitR - 1) * per, red)):
        n = e - b
        n8 = n // 8 * 8
        if n8:
            pos.add(b + n8 // 2)
        t = b + n8
        if e - t >= 4:
            pos.add(t + 1)
            t += 4
        if t < e:
            pos.add(t)
    return sorted(p for p in pos if 0 <= p < red)


def n_draws(case, d):
    if case.kind == "reduction" and case.op in ("MAX", "MIN"):
        kept, red, _ = _lines(case)
        n = -(-len(forced_positions(red, d["splitR"], d["redPerSplit"])) // kept)
        assert n <= MAX_DRAWS, (case.id, n)
        return max(2, n)
    return 2


def spike_positions(case, d, draw):
    kept, red, _ = _lines(case)
    forced = forced_positions(red, d["splitR"], d["redPerSplit"])
    k = np.arange(kept)
    pos = (k * 7 + draw * 101) % red
    idx = draw * kept + k
    take = idx < len(forced)
    pos[take] = np.asarray(forced)[idx[take]]
    return pos


def _mul_counts(dtype):
    return (4, 2) if dtype in xd.H16 else (10, 10)


def make_draw(case, draw, d):
    """the logical host tensors of one draw (numpy int64 / float64 / complex128, modes in descriptor order) by tensor name"""
    cplx = case.dtype in CPLX
    out = {}
    if case.kind != "reduction":
        for i, t in enumerate(TENSORS[case.kind][:-1]):
            out[t] = _ints(_rng(case, draw, i), case.extents(t), range(-3, 4), cplx)
        return out
    kept, red, _ = _lines(case)
    rng = _rng(case, draw, 0)
    out["C"] = _ints(_rng(case, draw, 2), case.extents("D"), range(-3, 4), cplx)
    if case.op == "ADD":
        A2 = _ints(rng, (kept, red), (-1, 1) if case.dtype in xd.H16 else (-3, -2, -1, 1, 2, 3), cplx)
        if case.dtype in xd.H16:      # signs repaired until alpha * sum + beta * c is an exact integer of the type for every run of the case
            L = EXACT_INT[case.dtype]
            c = _kept_linear(case, out["C"])
            for (alpha, beta), _ in case.runs:
                v = alpha * A2.sum(axis=1) + beta * c
                for k in np.flatnonzero(np.abs(v) > L):
                    sign = 1 if v[k] * alpha > 0 else -1                      # the entries to flip: those that push |v| up
                    n = int(np.ceil((abs(v[k]) - L) / (2 * abs(alpha))))
                    at = np.flatnonzero(A2[k] == sign)[:n]
                    A2[k, at] = -sign
    elif case.op in ("MAX", "MIN"):
        spike = 100 if case.op == "MAX" else -100
        A2 = rng.integers(-3, 4, size=(kept, red))
        A2[np.arange(kept), spike_positions(case, d, draw)] = spike
        if draw == n_draws(case, d) - 1:
            A2 = A2 - 2 * spike                                               # all-negative for MAX, all-positive for MIN
    elif cplx:                                                                # MUL: unit factors other than +1, a few +-2
        A2 = np.asarray([-1, 1j, -1j])[rng.integers(0, 3, size=(kept, red))]
        for k in range(kept):
            at = rng.choice(red, size=min(red, int(rng.integers(0, 11))), replace=False)
            A2[k, at] = rng.choice([-2.0, 2.0], size=len(at))
    else:                                                                     # MUL: -1, a few -2 and -0.5
        n2, n05 = _mul_counts(case.dtype)
        A2 = np.full((kept, red), -1.0)
        for k in range(kept):
            a, b = int(rng.integers(0, n2 + 1)), int(rng.integers(0, n05 + 1))
            at = rng.choice(red, size=min(red, a + b), replace=False)
            A2[k, at[:a]] = -2.0
            A2[k, at[a:]] = -0.5
    out["A"] = _from_lines(case, A2)
    return out


# ---- references -------------------------------------------------------------------------------------------------------------------------
F = {"ADD": np.add, "MUL": np.multiply, "MAX": np.maximum, "MIN": np.minimum}


def to_out(x, mX, mD):
    """x (modes mX) in D's mode order, extent 1 where D has a mode that x lacks (broadcast)"""
    present = [c for c in mD if c in mX]
    x = np.transpose(x, [mX.index(c) for c in present])
    return x.reshape([x.shape[present.index(c)] if c in mX else 1 for c in mD])


def reference(case, ins, run):
    """the exact result of one run, float64 / complex128, D's modes in descriptor order"""
    scal, cmode = run
    m = case.modes
    wide = np.complex128 if case.dtype in CPLX else np.float64
    shape = case.extents("D")
    A = np.conj(ins["A"]) if case.conjA else ins["A"]
    C = ins.get("C")
    if C is not None:
        C = (np.conj(C) if case.conjC else C).astype(wide)
    if case.kind == "reduction":
        alpha, beta = scal
        _, red = _red_axes(case)
        if case.op == "ADD":
            acc = A.sum(axis=tuple(red))                                       # int64 (complex: complex128 of integers below 2^53)
        else:
            acc = {"MUL": np.prod, "MAX": np.max, "MIN": np.min}[case.op](A, axis=tuple(red))
        ref = alpha * to_out(np.asarray(acc).astype(wide), "".join(c for c in m["A"] if c in m["D"]), m["D"])
        return np.broadcast_to(ref + (beta * C if beta else 0.0), shape).astype(wide)
    pa = to_out(A.astype(wide), m["A"], m["D"])
    if case.kind == "permutation":
        ref = scal[0] * pa
    elif case.kind == "binary":
        ref = F[case.op](scal[0] * pa, scal[1] * to_out(C, m["C"], m["D"]))
    else:
        pb = to_out(ins["B"].astype(wide), m["B"], m["D"])
        ref = F[case.op[1]](F[case.op[0]](scal[0] * pa, scal[1] * pb), scal[2] * to_out(C, m["C"], m["D"]))
    return np.broadcast_to(ref, shape).astype(wide)


def check_draw(case, ins, run, d):
    """the conditions on one run's data, asserted before anything is launched; returns the accumulator bound as a fraction of its limit"""
    scal, _ = run
    mag = lambda x: np.abs(x.real) + np.abs(x.imag)   # noqa: E731
    half = any(float(s) != round(float(s)) for s in scal)
    if case.kind != "reduction":
        assert all(mag(x).max() <= (6 if case.dtype in CPLX else 3) for x in ins.values()), case.id
        return 0.0
    alpha, beta = scal
    _, red = _red_axes(case)
    A = ins["A"]
    assert case.op in ("MAX", "MIN") or bool((A != 0).all()), "%s: a zero among the reduced elements" % case.id
    limit = xd.acc_limit(case.dtype) / (2 if half else 1)
    cmax = float(mag(ins["C"]).max()) if ins["C"].size else 0.0
    if case.op == "ADD":
        bound = abs(alpha) * float(mag(A).sum(axis=tuple(red)).max()) + abs(beta) * cmax
    elif case.op == "MUL":
        p = np.abs(np.prod(A, axis=tuple(red)))
        assert float(np.abs(np.log2(p)).max()) <= 10.0, "%s: a product outside 2^+-10" % case.id
        bound = abs(alpha) * 2.0 ** 10 + abs(beta) * cmax
    else:
        bound = abs(alpha) * float(np.abs(A).max()) + abs(beta) * cmax
    assert bound < limit, "%s: accumulator bound %g is not below %g" % (case.id, bound, limit)
    return bound / limit


def expected(case, ref):
    """what a correct kernel stores — asserted ON THE REFERENCE: every exact output is a value of the data type, so nothing rounds"""
    import torch
    r = torch.from_numpy(np.ascontiguousarray(ref).reshape(np.shape(ref)))          # (reshape: a 0-dim result stays 0-dim)
    want = xd.round_to(r, case.dtype)
    n = int((want != r).sum())
    assert n == 0, "%s: %d exact outputs are not values of %s" % (case.id, n, case.dtype)
    if case.dtype in xd.H16 and case.kind == "reduction" and case.op == "ADD":
        assert float(r.abs().max()) <= EXACT_INT[case.dtype], case.id
    return want


def check_case(case, d):
    """every draw and run of the case: the data conditions, the reference's representability, the spike coverage; returns the draws"""
    n = n_draws(case, d)
    seen = set()
    for draw in range(n):
        ins = make_draw(case, draw, d)
        for run in case.runs:
            check_draw(case, ins, run, d)
            expected(case, reference(case, ins, run))
        if case.kind == "reduction" and case.op in ("MAX", "MIN"):
            pos = spike_positions(case, d, draw)
            spike = (100 if case.op == "MAX" else -100) * (-1 if draw == n - 1 else 1)
            _, red = _red_axes(case)
            ext = {"MAX": np.max, "MIN": np.min}[case.op](ins["A"], axis=tuple(red))
            assert bool((ext == spike).all()), case.id           # the spike IS the extreme value of its line, all-negative draw included
            seen |= set(int(p) for p in pos)
    if case.kind == "reduction" and case.op in ("MAX", "MIN"):
        kept, red, _ = _lines(case)
        missing = set(forced_positions(red, d["splitR"], d["redPerSplit"])) - seen
        assert not missing, "%s: no spike at reduced indices %s" % (case.id, sorted(missing))
    return n


# ---- running a case ----------------------------------------------------------------------------------------------------------------------
def _placed(case, t):
    return xc.Placed(case.extents(t), case.dtype, off=case.off, strides=case.strides(t))


def _host(case, x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x).reshape(np.shape(x))).to(xd.TORCH_DTYPES[case.dtype])


def run_case(ct, ops, h, case, make=None, check=None, expect=None, runs=None):
    """`make`, `check`, `expect` and `runs` default to this table's make_draw, check_draw, expected and the case's own runs
    (tests/rounding_ew.py passes those of the rounding regime)"""
    import torch
    make, check, expect = make or make_draw, check or check_draw, expect or expected
    plan = make_plan(ct, ops, h, case)
    try:
        desc = wc.describe(ct, plan)
        assert case.expect(desc), "%s is off its path: %s" % (case.id, desc)
        d = {k: v for k, v in desc.pairs}
        ws = torch.empty(max(plan.required_workspace, 256), dtype=torch.uint8, device="cuda")
        for draw in range(n_draws(case, d)):
            ins = make(case, draw, d)
            dev = {}
            for t in TENSORS[case.kind][:-1]:
                if t != "C":
                    dev[t] = _placed(case, t)
                    dev[t].set(_host(case, ins[t]))
            for run in (runs or case.runs):
                scal, cmode = run
                check(case, ins, run, d)
                want = expect(case, reference(case, ins, run))
                pd = _placed(case, "D")                                     # NaN everywhere
                pc = None
                if cmode == "inplace":
                    pd.set(_host(case, ins["C"]))
                elif cmode == "separate":
                    pc = _placed(case, "C" if "C" in case.modes else "D")
                    pc.set(_host(case, ins["C"]))
                cptr = pc.ptr if pc else pd.ptr
                if case.kind == "permutation":
                    plan.permute(scal[0], dev["A"].ptr, pd.ptr)
                elif case.kind == "binary":
                    plan.binary(scal[0], dev["A"].ptr, scal[1], cptr, pd.ptr)
                elif case.kind == "trinary":
                    plan.trinary(scal[0], dev["A"].ptr, scal[1], dev["B"].ptr, scal[2], cptr, pd.ptr)
                else:
                    plan.reduce(scal[0], dev["A"].ptr, scal[1], cptr, pd.ptr, ws.data_ptr(), plan.required_workspace)
                torch.cuda.synchronize()
                what = "%s (draw %d, scalars %s, C %s) %s" % (case.id, draw, scal, cmode, desc)
                xd.assert_exact(pd.get(), want, what)
                pd.check_outside(what)
                if pc is not None:
                    xd.assert_exact(pc.get(), _host(case, ins["C"]), what + ": C was written")
                    pc.check_outside(what + " (C)")
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
