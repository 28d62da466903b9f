"""Far-strided tensors: the arena, the placement and the case table (tests/test_far_planner_cpu.py plans every case and checks the routing
rules, tests/test_far_arena_cpu.py runs the arena on CPU tensors against wrong stand-in kernels, tests/test_gpu_far_strides.py runs every
case) — a helper module, not a conftest, in the style of tests/exact_cases.py and tests/ew_exact_cases.py.

A far tensor has small extents and one inflated pitch: its slowest mode's stride is chosen so that the tensor's byte span reaches a
target next to 2^31 or 2^32 from below, while it touches a few hundred kilobytes.  One tensor of a case is far; it lives in the arena,
the others in exact_cases.Placed buffers.

The arena is ONE buffer of 3 x (2^bits + 2^(bits-4)) bytes filled with 0xFF (a NaN in every type); the far tensor starts one third in, at
byte 2^bits + 2^(bits-4) (plus the case's element offset), and spans at most 2^bits + 2^(bits-5) bytes.  An offset truncated to `bits`
bits, sign-extended from them, or off by +-2^(bits-1) or +-2^bits therefore lands INSIDE the allocation: it shows as a NaN in the result,
as an element that was not written, or as a byte of the arena that is no longer 0xFF — never as an access outside the buffer.  bits = 32
on the GPU (12.8 GiB); the CPU test of the harness itself uses bits = 16.

After each launch the far tensor's elements are read through its strided view and compared, then re-poisoned through an integer view of
the same element size, then the WHOLE arena must be 0xFF again (checked in chunks of at most 1 GiB).  A far input gets the same check:
nothing wrote into it or around it.

Data and references are those of tests/exact_data.py (contractions) and tests/ew_exact_cases.py (element-wise, reductions): integer-
valued, two draws, compared bit for bit.  No tolerance appears anywhere.

The table carries its own computation of the three quantities the planner routes by (operand span, full span with the batch modes,
16-bit tile span), written from the rule in csrc/host/plan_contraction.cpp and not read back from the library, and every case states
on which side of which limit it sits (`sides`).

The mixed fp64 x complex128 cases take their data and reference from tests/rc64_cases.py, the converting and the complex-trinary
element-wise cases their plans, data conditions and references from tests/convert_cases.py and tests/cplx_trinary_cases.py."""
import json
import sys

import numpy as np

import convert_cases as cv
import cplx_trinary_cases as ct3
import ew_exact_cases as ew
import exact_cases as xc
import exact_data as xd
import rc64_cases as rc
import workspace_cases as wc

RING, REG, GENK, SIMPLE, TABLE = "gett_f32_stream_kernel", "gett_f32_kernel", "gett_gen_kernel", "gett_simple_kernel", "gett_wide_kernel"
RING_LIMIT = (1 << 32) - (1 << 20)       # rank_contraction_choices: operand span of a ring kernel
RAG_LIMIT = (1 << 31) - (1 << 20)        # rank_contraction_choices: full span of a RAG twin
TILE_LIMIT = 1 << 31                     # pick_h16_choice: span of one 256-row x 64-k tile


def targets(bits=32, shift=11):
    """LO31, HI31, LO32, HI32 at a scale of `bits` offset bits: 2^(bits-1) and 2^bits -+ 2^(bits-shift)"""
    d = 1 << (bits - shift)
    return (1 << (bits - 1)) - d, (1 << (bits - 1)) + d, (1 << bits) - d, (1 << bits) + d


LO31, HI31, LO32, HI32 = targets(32)
ES = {"bfloat16": 2, "float16": 2, "float32": 4, "float64": 8, "complex64": 8, "complex128": 16}


# ---- the arena -------------------------------------------------------------------------------------------------------------------------
class Arena:
    CHUNK = 1 << 30

    def __init__(self, bits=32, device="cuda"):
        import torch
        self.bits = bits
        self.base = (1 << bits) + (1 << (bits - 4))
        self.size = 3 * self.base
        self.max_span = (1 << bits) + (1 << (bits - 5))
        self.raw = torch.full((self.size,), 0xFF, dtype=torch.uint8, device=device)
        self.sweeps = 0

    def place(self, extents, strides, dtype, off=0):
        return Far(self, extents, strides, dtype, off)

    def reset(self):
        self.raw.fill_(0xFF)

    def check_clean(self, what, origin=None):
        """every byte of the arena is 0xFF (in chunks of at most 1 GiB); on a failure the arena is refilled for the next case"""
        import torch
        words = self.raw.view(torch.int64)
        step = self.CHUNK // 8
        bad = torch.zeros((), dtype=torch.int64, device=self.raw.device)
        for i in range(0, words.numel(), step):
            bad += (words[i:i + step] != -1).sum()
        self.sweeps += 1
        n = int(bad)
        if n:
            first = None
            for i in range(0, self.size, self.CHUNK):
                hit = torch.nonzero(self.raw[i:i + self.CHUNK] != 0xFF)
                if hit.numel():
                    first = i + int(hit[0])
                    break
            self.reset()
            rel = first - (origin if origin is not None else self.base)
            raise AssertionError("%s: %d 8-byte words of the arena outside the far tensor's elements were written; the first byte at %+d "
                                 "from the tensor's first element (%+.4f x 2^%d)" % (what, n, rel, rel / 2.0 ** self.bits, self.bits))


class Far(xc.Placed):
    """a tensor in the arena: the interface of exact_cases.Placed (view, set, get, ptr); check_outside re-poisons the tensor's own elements
    and then asserts the whole arena clean, so it comes AFTER the tensor was read"""

    def __init__(self, arena, extents, strides, dtype, off=0):
        import torch
        self.arena = arena
        self.extents, self.strides = list(extents), list(strides)
        self.tdt = xd.TORCH_DTYPES[dtype]
        self.es = torch.empty((), dtype=self.tdt).element_size()
        self.span_bytes = (1 + sum((e - 1) * s for e, s in zip(self.extents, self.strides))) * self.es
        assert all(s > 0 for s in self.strides) and self.span_bytes <= arena.max_span, (self.span_bytes, arena.max_span)
        self.byte0 = arena.base + off * self.es
        self.start = self.byte0 // self.es
        self.raw = arena.raw
        self.buf = arena.raw.view(self.tdt)
        self.ptr = arena.raw.data_ptr() + self.byte0
        self.packed = False

    def repoison(self):
        """0xFF into exactly the tensor's elements, through an integer view of the same element size (16-byte elements: two int64)"""
        import torch
        it = {1: torch.uint8, 2: torch.int16, 4: torch.int32}.get(self.es, torch.int64)
        w = self.es // min(self.es, 8)
        rev = lambda x: list(reversed(x))   # noqa: E731
        v = self.raw.view(it).as_strided(rev(self.extents) + [w], [s * w for s in rev(self.strides)] + [1], self.start * w)
        v.fill_(0xFF if it == torch.uint8 else -1)

    def check_outside(self, what):
        self.repoison()
        self.arena.check_clean(what, self.byte0)


# ---- placement -------------------------------------------------------------------------------------------------------------------------
def padded_strides(extents, pad=0):
    """packed strides, first mode fastest; pad: elements added to the first mode's extent, or one number per mode"""
    p = list(pad) if isinstance(pad, (tuple, list)) else [pad] + [0] * len(extents)
    s, run = [], 1
    for i, x in enumerate(extents):
        s.append(run)
        run *= x + p[i]
    return s


def byte_span(extents, strides, es):
    return (1 + sum((e - 1) * s for e, s in zip(extents, strides))) * es


def far_strides(extents, es, target, pad=0, quantity=None, grain=None):
    """packed (padded) strides whose slowest pitch is the largest multiple of 16 bytes (or of `grain` elements: a converting plan's lane is
    16 bytes of its NARROWER type) at which quantity(strides) — default: the byte span — is still <= target; asserts that the next such
    pitch would pass the target"""
    s = padded_strides(extents, pad)
    assert len(extents) >= 2 and extents[-1] > 1, extents
    q = quantity or (lambda st: byte_span(extents, st, es))
    g = grain or max(1, 16 // es)
    at = lambda p: q(s[:-1] + [p * g])   # noqa: E731
    lo = -(-s[-1] // g)
    assert at(lo) <= target, "the packed tensor already passes the target"
    assert at(lo + 1) > at(lo), "the quantity does not depend on the slowest pitch"
    hi = lo + 1
    while at(hi) <= target:
        hi *= 2
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if at(mid) <= target else (lo, mid)
    assert at(lo) <= target < at(lo + 1)
    return s[:-1] + [lo * g]


# ---- contraction cases -----------------------------------------------------------------------------------------------------------------
class FarCase(xc.Case):
    """an exact_cases.Case with one far tensor ("A", "B", "C" or "D"): `target` bytes for `quantity` ("full": the tensor's byte span, the
    default; "span": the span without the batch modes; "tile": the 16-bit tile span).  `pads`: first-mode padding per tensor.  `sweep`: run
    every rank algo = r, r < 12, whose kernel is this one (None: the planner's choice).  `sides`: (quantity, tensor, "<" or ">=", limit) —
    asserted from this module's own span computation.  `section`: the group of the summary the case counts in.  `real`: 0 / 1 — A / B is real
    fp64 in a complex128 contraction (data and reference of tests/rc64_cases.py).  `flat`: the one plan the case runs is the first rank
    on the 96 x 96 ring-3 kernel with split-K (the tile that has a flat entry), and every launch must take the flat entry."""

    def __init__(self, id, dtype, ext, modes, expect, far, target, section, quantity="full", pads=None, sweep=None, sides=(), compute=None, real=None,
                 flat=False, **kw):
        xc.Case.__init__(self, id, dtype, ext, modes, expect, **kw)
        self.far, self.target, self.quantity, self.section = far, target, quantity, section
        self.pads, self.sweep, self.sides, self.compute = dict(pads or {}), sweep, list(sides), compute
        self.real, self.flat = real, flat
        self.conj = (self.conjA, self.conjB, self.conjC)
        self.kind = "contraction"
        self._strides = {}

    def tdtype(self, t):
        return "float64" if self.real is not None and t == "AB"[self.real] else self.dtype

    def dtypes(self):
        return self.tdtype("A"), self.tdtype("B")

    def tmodes(self, t):
        return self.modes[{"A": 0, "B": 1, "C": 2, "D": 2}[t]]

    def strides(self, t):
        if t not in self._strides:
            e, pad = self.extents(self.tmodes(t)), self.pads.get(t, 0)
            if t == self.far:
                q = None if self.quantity == "full" else (lambda st: quantities(self, {t: st})[t][self.quantity])
                self._strides[t] = far_strides(e, ES[self.tdtype(t)], self.target, pad, q)
            else:
                self._strides[t] = padded_strides(e, pad)
        return self._strides[t]

    def needs_rag(self):
        """fp32: the ring kernel's RAG twin runs — ragged K, or an operand without strict 16-byte lanes, as the case constructs it"""
        m = xd.Modes(*self.modes[:3])
        k = int(np.prod([self.ext[c] for c in m.K])) if m.K else 1
        loose = (self.align or 128) < 16 or self.off % 4 != 0 or any(s % 4 for t in "AB" for s in self.strides(t) if s != 1)
        return k % 32 != 0 or loose


def quantities(case, strides=None):
    """per operand: the byte span without the batch modes ("span"), with them ("full") and the span of one 256-row x 64-k tile ("tile"), as
    csrc/host/plan_contraction.cpp states them: span = 1 + sum (extent - 1) |stride| over the operand's free and contracted modes, full
    adds the batch modes, tile = 1 + sum over the free modes (min(extent, 256) - 1) stride + 64 x the stride of the fastest contracted
    mode — the one with the smallest stride in kernel-A (kernel-B when only that one has a stride-1 contracted mode); kernel-A is the
    caller's B when D's fastest free mode lives in A.  (Modes that fuse keep the spans; the tile span is used only where no fused free
    group passes 256.)"""
    strides = strides or {}
    m = xd.Modes(*case.modes[:3])
    st = {t: dict(zip(case.tmodes(t), strides.get(t) or case.strides(t))) for t in "AB"}
    ext = case.ext
    batch = [c for c in m.A if c in m.B and c in m.C]
    out = {}
    for t, ms in (("A", m.A), ("B", m.B)):
        es = ES[case.tdtype(t)]
        span = 1 + sum((ext[c] - 1) * st[t][c] for c in ms if c not in batch)
        full = span + sum((ext[c] - 1) * st[t][c] for c in batch)
        out[t] = {"span": span * es, "full": full * es}
    if m.K:
        sD = dict(zip(m.C, padded_strides(case.extents(m.C), case.pads.get("D", 0)) if case.far == "D" else case.strides("D")))
        freeA = [c for c in m.A if c in m.C and c not in batch]
        freeB = [c for c in m.B if c in m.C and c not in batch]
        swapped = min([sD[c] for c in freeA] or [1 << 62]) < min([sD[c] for c in freeB] or [1 << 62])
        kA, kB = ("B", "A") if swapped else ("A", "B")
        contig = lambda t: any(st[t][c] == 1 for c in m.K)   # noqa: E731
        follow = kB if (not contig(kA) and contig(kB)) else kA
        k0 = min(m.K, key=lambda c: st[follow][c])
        for t, free in (("A", freeA), ("B", freeB)):
            out[t]["tile"] = (1 + sum((min(ext[c], 256) - 1) * st[t][c] for c in free) + 64 * st[t][k0]) * ES[case.tdtype(t)]
    return out


def check_sides(case):
    q = quantities(case)
    for name, t, rel, limit in case.sides:
        v = q[t][name]
        assert (v < limit) if rel == "<" else (v >= limit), "%s: %s of %s is %d, expected %s %d" % (case.id, name, t, v, rel, limit)
    t = case.far
    assert byte_span(case.extents(case.tmodes(t)), case.strides(t), ES[case.tdtype(t)]) <= (1 << 32) + (1 << 27), "%s: the far tensor passes the arena's span" % case.id
    if case.far in "AB":
        v = q[case.far][case.quantity]
        assert case.target - (1 << 16) <= v <= case.target, (case.id, v, case.target)     # reached from below, within one pitch step
    return q


def check_routing(case, d, q=None):
    """the planner's three addressing rules on one plan description, with this module's spans"""
    q = q or quantities(case)
    for t in "AB":
        if d.get("kname") == RING:
            assert q[t]["span"] < RING_LIMIT, "%s: a ring kernel on an operand span of %d bytes: %s" % (case.id, q[t]["span"], d)
            if case.needs_rag():
                assert q[t]["full"] < RAG_LIMIT, "%s: a RAG twin on a full span of %d bytes: %s" % (case.id, q[t]["full"], d)
        if d.get("family") == 1:
            assert q[t]["tile"] < TILE_LIMIT, "%s: a family-1 plan on a tile span of %d bytes: %s" % (case.id, q[t]["tile"], d)


CASES = []


def add(*a, **kw):
    c = FarCase(*a, **kw)
    assert all(c.id != o.id for o in CASES), c.id
    CASES.append(c)
    return c


def _k(*names, **more):
    return lambda d: d.get("kname") in names and all(d.get(k) == v for k, v in more.items())


_T = {LO31: "lo31", HI31: "hi31", LO32: "lo32", HI32: "hi32"}
_S = xc.SCALARS32

# fp32 ring kernel, whole K-tiles (no RAG twin): operand span in [2^31, 2^32), every ring rank among the first 12
for _li, (_mA, _mB) in enumerate(xc.LAYOUTS):
    _L = xc.LNAME[(_mA, _mB)]
    for _far in "AB":
        for _tg in (HI31, LO32):
            add("f32_ring_%s_far%s_%s" % (_L, _far, _T[_tg]), "float32", dict(m=96, n=96, k=128), (_mA, _mB, "mn"), _k(RING), _far, _tg, "f32 ring", sweep=RING,
                sides=[("span", _far, ">=", 1 << 31), ("span", _far, "<", RING_LIMIT)], alpha=_S[_li][0], beta=_S[_li][1])
        # past the ring's limit: the register-staged kernel
        add("f32_reg_%s_far%s_hi32" % (_L, _far), "float32", dict(m=96, n=96, k=128), (_mA, _mB, "mn"), _k(REG), _far, HI32, "f32 register kernel",
            sides=[("span", _far, ">=", RING_LIMIT)], alpha=-2.0, beta=1.0)
        # RAG twins (k = 100): below the 2^31 limit on the ring, above it on the register-staged kernel
        add("f32_rag_%s_far%s_lo31" % (_L, _far), "float32", dict(m=96, n=96, k=100), (_mA, _mB, "mn"), _k(RING), _far, LO31, "f32 RAG twin", sweep=RING,
            sides=[("full", _far, "<", RAG_LIMIT)], alpha=0.5, beta=-0.5)
        add("f32_rag_%s_far%s_hi31" % (_L, _far), "float32", dict(m=96, n=96, k=100), (_mA, _mB, "mn"), _k(REG), _far, HI31, "f32 register kernel",
            sides=[("full", _far, ">=", RAG_LIMIT)], alpha=1.0, beta=1.0)
# the far stride on the second of two contracted modes: it lives in the K odometer's wrap term, the free modes stay near
for _mA, _mB, _far, _n in (("kmj", "knj", "A", "km"), ("mkj", "knj", "A", "mk"), ("kmj", "knj", "B", "kn"), ("kmj", "nkj", "B", "nk")):
    for _tg in (HI31, LO32):
        add("f32_ring_wrap_%s_far%s_%s" % (_n, _far, _T[_tg]), "float32", dict(m=96, n=96, k=32, j=4), (_mA, _mB, "mn"), _k(RING), _far, _tg, "f32 ring",
            sweep=RING, sides=[("span", _far, ">=", 1 << 31), ("span", _far, "<", RING_LIMIT)], alpha=-2.0, beta=0.0)
    # (a RAG twin on several contracted modes takes whole K-tiles only: it is the odd element offset that takes the lanes away)
    add("f32_rag_wrap_%s_far%s_lo31" % (_n, _far), "float32", dict(m=96, n=96, k=32, j=4), (_mA, _mB, "mn"), _k(RING), _far, LO31, "f32 RAG twin",
        sweep=RING, sides=[("full", _far, "<", RAG_LIMIT)], off=3, align=4, alpha=1.0, beta=0.0)
# a batch mode carries the span: the operand span is small, full_span_bytes decides, the descriptor base moves by the batch offset
for _far, _mA, _mB in (("A", "kml", "knl"), ("B", "mkl", "nkl")):
    add("f32_rag_batch_far%s_lo31" % _far, "float32", dict(m=96, n=96, k=100, l=2), (_mA, _mB, "mnl"), _k(RING), _far, LO31, "f32 RAG twin", sweep=RING,
        sides=[("span", _far, "<", 1 << 20), ("full", _far, "<", RAG_LIMIT)], alpha=-2.0, beta=1.0)
    add("f32_rag_batch_far%s_hi31" % _far, "float32", dict(m=96, n=96, k=100, l=2), (_mA, _mB, "mnl"), _k(REG), _far, HI31, "f32 register kernel",
        sides=[("span", _far, "<", 1 << 20), ("full", _far, ">=", RAG_LIMIT)], alpha=0.5, beta=0.0)
# the small, strided form of the 5.4-GB test: UNFUSED (63 x 45 x 37, two batches, M and N unfused in D) on the register-staged kernel;
# once with the batch mode slowest (the far pitch is the batch stride), once with a free mode slowest
UNFUSED_INNER_BATCH = ("klab", "klcd", "acbdl")
for _far in "AB":
    add("f32_reg_unfused_far%s" % _far, "float32", xc.UNFUSED, xc.UNFUSED_MODES, _k(REG), _far, HI32, "f32 register kernel", pads=dict(D=1, C=3),
        alpha=-2.0, beta=1.0)
    add("f32_reg_unfused_free_far%s" % _far, "float32", xc.UNFUSED, UNFUSED_INNER_BATCH, _k(REG), _far, HI32, "f32 register kernel", pads=dict(D=1, C=3),
        alpha=0.5, beta=-0.5)
# far D (beta = 0) and far C (beta != 0, D near, C's other pitches different from D's) past 2^32 bytes: every fp32 epilogue and fold
HEAD_SMALL = dict(a=96, b=4, c=4, d=64, e=96)          # the headline 'abcd,dcbe->ae' on one 96 x 96 output tile, A K-contiguous
for _far, _al, _be in (("D", -2.0, 0.0), ("C", 0.5, -0.5)):
    # (a two-mode far C: its only pitch is the far one; D's pitch is padded, so neither equals the packed pitch nor the other's)
    _p = dict(D=4) if _far == "C" else {}
    add("f32_reg_unfused_far%s" % _far, "float32", xc.UNFUSED, xc.UNFUSED_MODES, _k(REG), _far, HI32, "f32 far C/D", pads=dict(dict(D=1, C=3), **_p),
        alpha=_al, beta=_be)
    # the ring kernel's epilogue: rows with 16-byte lanes (aligned base) ...
    add("f32_ring_rows_far%s" % _far, "float32", dict(m=100, n=52, k=128), ("km", "kn", "mn"), _k(RING), _far, HI32, "f32 far C/D", sweep=RING, off=4, align=16,
        pads=_p, alpha=_al, beta=_be)
    # ... and its scalar form (odd element offset: no lanes anywhere, the RAG twin)
    add("f32_ring_scalar_far%s" % _far, "float32", dict(m=100, n=52, k=100), ("mk", "kn", "mn"), _k(RING), _far, HI32, "f32 far C/D", sweep=RING, off=3, align=4,
        pads=dict(D=1) if _far == "C" else {}, alpha=_al, beta=_be)
    # split-K folds: the shape the planner splits by itself, and the flat-entry fold of a one-tile shape
    add("f32_splitk_fold_far%s" % _far, "float32", dict(m=100, n=60, k=4099), ("mk", "kn", "mn"), lambda d: d.get("family") == 0 and d.get("splitK", 1) > 1,
        _far, HI32, "f32 split-K fold", off=3, align=4, pads=dict(D=1) if _far == "C" else {}, alpha=_al, beta=_be)
    add("f32_one_tile_far%s" % _far, "float32", dict(m=96, n=96, k=4096), ("km", "kn", "mn"), _k(RING), _far, HI32, "f32 far C/D", sweep=RING, pads=_p,
        alpha=_al, beta=_be)
    # the flat entry and its fold: one output tile of the 96 x 96 ring-3 kernel, eight slices, one K-contiguous operand
    add("f32_flat_fold_far%s" % _far, "float32", HEAD_SMALL, ("dcba", "ebcd", "ea"), lambda d: d.get("kname") == RING and d.get("splitK") == 8 and d.get("blocks") == 8,
        _far, HI32, "f32 flat-entry fold", sweep=RING, flat=True, env={"CUTENSOR_AMD_F32_SPLITK": "8"}, ws_limit=1 << 30, pads=_p, alpha=_al, beta=_be)

# ---- the general family: fp64, complex64, complex128 (with conjugation) on UNFUSED; far A, B, D, C and a split-K fold into a far D ----------
for _dt, _sh in (("float64", "f64"), ("complex64", "c64"), ("complex128", "c128")):
    for _mA, _mB, _n in (("kabl", "kcdl", "km_kn"), ("abkl", "cdkl", "mk_nk")):
        _conj = (True, False, True) if (_dt == "complex128" and _n == "mk_nk") else (False, False, False)
        for _far, _al, _be in (("A", -2.0, 1.0), ("B", 0.5, -0.5), ("D", -2.0, 0.0), ("C", 1.0, 1.0)):
            add("%s_gen_%s_far%s" % (_sh, _n, _far), _dt, xc.UNFUSED, (_mA, _mB, "acbdl"), wc._family(2, GENK), _far, HI32, "general family " + _sh,
                pads=dict(D=1, C=3), conj=_conj, alpha=_al, beta=_be)
    add("%s_gen_splitk_farD" % _sh, _dt, wc.ODD, ("mk", "kn", "mn"), wc._family(2, GENK, True), "D", HI32, "general family " + _sh, alpha=-2.0, beta=0.0)
    add("%s_gen_splitk_farC" % _sh, _dt, wc.ODD, ("mk", "kn", "mn"), wc._family(2, GENK, True), "C", HI32, "general family " + _sh, pads=dict(D=1),
        alpha=0.5, beta=1.0)
# fp32 under a reduced-precision compute descriptor (gett_gen_f32x_kernel; +-3 and their sums below 2^24 are exact in every such format)
F32X, F64X = {"CUTENSOR_AMD_F32X": "force"}, {"CUTENSOR_AMD_F64X": "force"}
for _mA, _mB, _n in (("kabl", "kcdl", "km_kn"), ("abkl", "cdkl", "mk_nk")):
    for _far, _al, _be in (("A", -2.0, 1.0), ("B", 0.5, -0.5), ("D", -2.0, 0.0), ("C", 1.0, 1.0)):
        _m3 = (_mA, _mB, "acbdl")
        add("f32x_gen_%s_far%s" % (_n, _far), "float32", xc.UNFUSED, _m3, _k("gett_gen_f32x_kernel"), _far, HI32, "general family f32x", pads=dict(D=1, C=3),
            compute="TF32", env=F32X, alpha=_al, beta=_be)
        add("f64x_gen_%s_far%s" % (_n, _far), "float64", xc.UNFUSED, _m3, _k("gett_gen_f64x_kernel"), _far, HI32, "general family f64x", pads=dict(D=1, C=3),
            compute="32F", env=F64X, alpha=_al, beta=_be)
        # complex64 under a reduced-precision descriptor (gett_gen_c32x_kernel), complex128 under COMPUTE_DESC_32F (f64x, complex)
        add("c32x_gen_%s_far%s" % (_n, _far), "complex64", xc.UNFUSED, _m3, _k("gett_gen_c32x_kernel"), _far, HI32, "general family c32x", pads=dict(D=1, C=3),
            compute="TF32", env=F32X, conj=(False, _n == "mk_nk", False), alpha=_al, beta=_be)
        add("c64x_gen_%s_far%s" % (_n, _far), "complex128", xc.UNFUSED, _m3, _k("gett_gen_f64x_kernel"), _far, HI32, "general family f64x", pads=dict(D=1, C=3),
            compute="32F", env=F64X, alpha=_al, beta=_be)
        # real fp64 x complex128 (gett_gen_rc64_kernel): the real operand as A and as B
        for _real in (0, 1):
            add("rc64_gen_%s_real%s_far%s" % (_n, "AB"[_real], _far), "complex128", xc.UNFUSED, _m3, rc.tiled(_real, split=False), _far, HI32, "general family rc64",
                pads=dict(D=1, C=3), real=_real, conj=(False, False, _far == "C"), alpha=complex(-2, 1), beta=complex(0.5, -0.5) if _be else 0.0)
# their split-K folds into a far D (k = 4099 / 3001 / 517: the planner splits by itself)
add("f32x_gen_splitk_farD", "float32", dict(m=100, n=60, k=4099), ("mk", "kn", "mn"), lambda d: d.get("kname") == "gett_gen_f32x_kernel" and d.get("splitK", 1) > 1,
    "D", HI32, "general family f32x", compute="TF32", env=F32X, alpha=0.5, beta=0.0)
add("c32x_gen_splitk_farD", "complex64", dict(m=100, n=60, k=4099), ("mk", "kn", "mn"), lambda d: d.get("kname") == "gett_gen_c32x_kernel" and d.get("splitK", 1) > 1,
    "D", HI32, "general family c32x", compute="TF32", env=F32X, alpha=0.5, beta=0.0)
for _real in (0, 1):
    add("rc64_gen_splitk_real%s_farD" % "AB"[_real], "complex128", xc.UNFUSED_LONG, xc.UNFUSED_MODES, rc.tiled(_real, split=True), "D", HI32, "general family rc64",
        pads=dict(C=3), real=_real, alpha=complex(-2, 1), beta=0.0)
# gett_gen_f64x_kernel's own fold (gen_f64x_splitk_reduce_kernel): unforced routing never splits K on this path (f64x_decide), the switch
# that every f64x case here runs under does.  Sums of 4099 products of +-3 (complex: both parts) stay far below 2^24: exact in fp32.
for _dt, _sh in (("float64", "f64x"), ("complex128", "c64x")):
    add("%s_gen_splitk_farD" % _sh, _dt, dict(m=100, n=60, k=4099), ("mk", "kn", "mn"), lambda d: d.get("kname") == "gett_gen_f64x_kernel" and d.get("splitK", 1) > 1,
        "D", HI32, "general family f64x", compute="32F", env=F64X, alpha=0.5, beta=0.0)
    add("%s_gen_splitk_farC" % _sh, _dt, dict(m=100, n=60, k=4099), ("mk", "kn", "mn"), lambda d: d.get("kname") == "gett_gen_f64x_kernel" and d.get("splitK", 1) > 1,
        "C", HI32, "general family f64x", compute="32F", env=F64X, pads=dict(D=1), alpha=-2.0, beta=1.0)

# ---- 16-bit: family 1 (LDS-DMA) with tile spans next to 2^31, family 2 past it --------------------------------------------------------
H16 = dict(m=264, n=136, k=128)
_fam1 = lambda d: d.get("family") == 1          # noqa: E731
for _i, _dt in enumerate(("bfloat16", "float16")):
    _sh = ew.SHORT[_dt]
    _s = xc.SCALARS16
    # K-contiguous far operand with a far row pitch / free-contiguous far operand with a far K stride; as A and as B
    for _far, _mA, _mB, _n in (("A", "km", "kn", "kcontig"), ("A", "mk", "kn", "fcontig"), ("B", "km", "kn", "kcontig"), ("B", "km", "nk", "fcontig")):
        _ext = H16 if _far == "A" else dict(m=136, n=264, k=128)
        add("%s_h16_%s_far%s_tile_lo31" % (_sh, _n, _far), _dt, _ext, (_mA, _mB, "mn"), _fam1, _far, LO31, "16-bit family 1", quantity="tile",
            sides=[("tile", _far, "<", TILE_LIMIT)], alpha=_s[_i][0], beta=_s[_i][1])
        add("%s_h16_%s_far%s_tile_hi31" % (_sh, _n, _far), _dt, _ext, (_mA, _mB, "mn"), wc._family(2, GENK), _far, HI31, "16-bit general family", quantity="tile",
            sides=[("tile", _far, ">=", TILE_LIMIT)], alpha=_s[_i + 2][0], beta=_s[_i + 2][1])
    # two M modes (a = 8, b = 33): the slow one carries the far stride, the rows of one 256-row tile are spread across it
    for _far, _mA, _mB, _mC, _n in (("A", "kab", "kn", "abn", "kcontig"), ("A", "akb", "kn", "abn", "fcontig"), ("B", "km", "kab", "mab", "kcontig"),
                                     ("B", "km", "akb", "mab", "fcontig")):
        _ext = dict(a=8, b=33, k=128, **({"n": 136} if _far == "A" else {"m": 136}))
        add("%s_h16_two_free_%s_far%s_tile_lo31" % (_sh, _n, _far), _dt, _ext, (_mA, _mB, _mC), _fam1, _far, LO31, "16-bit family 1", quantity="tile",
            sides=[("tile", _far, "<", TILE_LIMIT)], alpha=_s[1][0], beta=_s[1][1])
        add("%s_h16_two_free_%s_far%s_tile_hi31" % (_sh, _n, _far), _dt, _ext, (_mA, _mB, _mC), wc._family(2, GENK), _far, HI31, "16-bit general family",
            quantity="tile", sides=[("tile", _far, ">=", TILE_LIMIT)], alpha=_s[2][0], beta=_s[2][1])
    # the whole span past 2^32 with a small tile span: 520 rows whose pitch puts 255 rows at 2^31 - 2^21 bytes; the 64-bit base moves
    add("%s_h16_520_rows_farA" % _sh, _dt, dict(m=520, n=136, k=128), ("km", "kn", "mn"), _fam1, "A", LO31, "16-bit family 1", quantity="tile",
        sides=[("tile", "A", "<", TILE_LIMIT), ("full", "A", ">=", 1 << 32)], alpha=_s[3][0], beta=_s[3][1])
    # far D / far C past 2^32 on the one-tile epilogue
    add("%s_h16_farD" % _sh, _dt, H16, ("km", "kn", "mn"), _fam1, "D", HI32, "16-bit family 1", alpha=_s[3][0], beta=0.0)
    add("%s_h16_farC" % _sh, _dt, H16, ("km", "kn", "mn"), _fam1, "C", HI32, "16-bit family 1", pads=dict(D=8), alpha=_s[1][0], beta=_s[1][1])
    # the general family's 16-bit path, far A / B / D / C
    for _far, _al, _be in (("A", -1.0, 2.0), ("B", 2.0, -1.0), ("D", -2.0, 0.0), ("C", 1.0, 1.0)):
        add("%s_gen_far%s" % (_sh, _far), _dt, dict(m=77, n=53, k=91, j=3), ("mkj", "jkn", "mn"), wc._family(2, GENK), _far, HI32, "16-bit general family",
            pads=dict(D=1) if _far == "C" else {}, alpha=_al, beta=_be)
    # ... on UNFUSED in both layouts, as the other element paths (the general family forced: a child process)
    for _mA, _mB, _n in (("kabl", "kcdl", "km_kn"), ("abkl", "cdkl", "mk_nk")):
        for _far, _al, _be in (("A", -1.0, 2.0), ("B", 2.0, -1.0), ("D", -2.0, 0.0), ("C", 1.0, 1.0)):
            add("%s_gen_unfused_%s_far%s" % (_sh, _n, _far), _dt, xc.UNFUSED, (_mA, _mB, "acbdl"), wc._family(2, GENK), _far, HI32, "16-bit general family",
                pads=dict(D=1, C=3), env=wc.GEN, group="far_gen_force", alpha=_al, beta=_be)
    # ... and its split-K fold into a far D (k = 3001 splits)
    add("%s_gen_splitk_farD" % _sh, _dt, wc.ODD, ("mk", "kn", "mn"), wc._family(2, GENK, True), "D", HI32, "16-bit general family", env=wc.GEN,
        group="far_gen_force", alpha=-1.0, beta=0.0)
# the variants the existing tests force, and the persistent kernel: one child process per switch value, each with an arena of its own
for _w in ("4p", "4m", "4m4", "8m", "4q"):
    _env = {"CUTENSOR_AMD_H16_WAVES": _w}
    _want = xc._h16_variant(_w)
    _ext = dict(m=520, n=264, k=192)
    for _dt in ("bfloat16", "float16"):
        _sh = ew.SHORT[_dt]
        for _far, _mA, _mB in (("A", "km", "kn"), ("B", "mk", "kn")):          # (a far row pitch: a far K stride over this many K-tiles would pass the arena)
            add("%s_h16_%s_far%s_tile_lo31" % (_sh, _w, _far), _dt, _ext, (_mA, _mB, "mn"), _want, _far, LO31, "16-bit forced variants", quantity="tile",
                sides=[("tile", _far, "<", TILE_LIMIT)], env=_env, group="far_h16_" + _w, alpha=-1.0, beta=2.0)
        add("%s_h16_%s_farD" % (_sh, _w), _dt, _ext, ("km", "kn", "mn"), _want, "D", HI32, "16-bit forced variants", env=_env, group="far_h16_" + _w,
            alpha=2.0, beta=0.0)
        add("%s_h16_%s_farC" % (_sh, _w), _dt, _ext, ("km", "kn", "mn"), _want, "C", HI32, "16-bit forced variants", env=_env, group="far_h16_" + _w,
            pads=dict(D=8), alpha=1.0, beta=1.0)

# ---- gett_simple and the mode-table kernel: far A and far D, fp32 and fp64 ---------------------------------------------------------------
for _dt, _sh in (("float32", "f32"), ("float64", "f64")):
    for _far, _be in (("A", -0.5), ("D", 0.0)):
        add("%s_mode_table_far%s" % (_sh, _far), _dt, xc.WIDE_EXT, (xc.WIDE_A, xc.WIDE_B, xc.WIDE_C), _k(TABLE), _far, HI32, "mode-table kernel", ws_limit=None,
            alpha=-2.0, beta=_be)
        # (fp32 data reaches gett_simple under COMPUTE_DESC_64F, fp64 data with the general family switched off: a child process)
        add("%s_simple_far%s" % (_sh, _far), _dt, wc.ODD, ("mk", "kn", "mn"), _k(SIMPLE), _far, HI32, "gett_simple", alpha=0.5, beta=_be,
            **(dict(compute="64F") if _dt == "float32" else dict(env={"CUTENSOR_AMD_GEN": "0"}, group="far_gen0")))

BY_ID = {c.id: c for c in CASES}
IN_PROCESS = [c.id for c in CASES if c.group is None]
GROUPS = sorted({c.group for c in CASES if c.group})


# ---- element-wise and reduction cases ----------------------------------------------------------------------------------------------------
class FarEw(ew.Case):
    """a case of tests/ew_exact_cases.py (its data, its runs, its path predicate) with one tensor's slowest pitch inflated"""

    def __init__(self, id, base, far, section, target=HI32, expect=None):
        b = ew.BY_ID[base] if isinstance(base, str) else base
        m = tuple(b.modes[t] for t in ew.TENSORS[b.kind])
        ew.Case.__init__(self, id, b.kind, b.dtype, b.ext, m, expect or b.expect, b.runs, op=b.op, pad=b.pad, off=b.off, align=b.align, env=b.env,
                         conj=(b.conjA, b.conjC), compute=b.compute)
        self.far, self.target, self.section, self.data_key = far, target, section, b.data_key
        # a converting case (convert_cases.Case: A's type differs from D's) or a complex trinary one (cplx_trinary_cases.Case)
        self.flavour = "convert" if isinstance(b, cv.Case) else "cplx_trinary" if isinstance(b, ct3.Case) else "plain"
        self.pair, self.dtypeA, self.conj3 = getattr(b, "pair", None), getattr(b, "dtypeA", b.dtype), getattr(b, "conj3", None)
        if self.kind == "reduction" and far == "D":       # C shares D's descriptor: a separate C would be a second far tensor
            self.runs = [r for r in self.runs if r[1] != "separate"]
        if self.kind == "binary" or (self.kind == "trinary" and far == "C"):      # C and D differ in layout: C in a buffer of its own
            self.runs = [r for r in self.runs if r[1] == "separate"]
        if self.kind == "trinary" and far == "D":         # C has a descriptor of its own, with near pitches: it cannot be the far D
            self.runs = [r for r in self.runs if r[1] != "inplace"]
        assert self.runs, id

    def tdtype(self, t):
        return self.dtypeA if t == "A" else self.dtype

    def alignment(self, t):
        return self.align[t] if isinstance(self.align, dict) else (self.align or 128)

    def strides(self, t):
        if t != self.far:
            return ew.Case.strides(self, t)
        return far_strides(self.extents(t), ES[self.tdtype(t)], self.target, self.pad.get(t, 0), grain=cv.lane(self.pair) if self.pair else None)


EW_CASES = []


def add_ew(*a, **kw):
    c = FarEw(*a, **kw)
    assert all(c.id != o.id for o in EW_CASES), c.id
    EW_CASES.append(c)
    return c


# one case per kernel variant the plan description names, at its smallest shape with partial tiles: far A (source pitch), far D, and far C
# for the binary form
_PERM = ["f32_perm_transpose_t64", "f32_perm_transpose_t128", "f32_perm_transpose_t256", "f32_perm_rowcopy", "bf16_perm_rowcopy", "f32_perm_block_pad",
         "bf16_perm_block_vec", "f32_perm_generic", "bf16_perm_generic", "f64_perm_generic", "c64_perm_generic", "f32_perm_any", "f16_perm_any_pair",
         "f64_perm_transpose", "c64_perm_transpose_conjA", "c128_perm_transpose", "f64_perm_rowcopy", "c128_perm_rowcopy",
         "bf16_perm_transpose_narrow", "f16_perm_transpose_w256", "bf16_perm_transpose_w128"]
for _b in _PERM:
    for _far in "AD":
        add_ew("%s_far%s" % (_b, _far), _b, _far, "permutation")
_BIN = ["f32_bin_transpose_t64_add", "f32_bin_transpose_c_order_add", "f32_bin_rowcopy_pad_add", "bf16_bin_rowcopy_pad_max", "f32_bin_generic_small_mul",
        "f32_bin_any_add", "f64_bin_transpose_add", "c64_bin_transpose_conjAC_mul", "c128_bin_transpose_add", "f16_bin_transpose_narrow_min",
        "c64_bin_generic_conjA_add"]
for _b in _BIN:
    for _far in "ACD":
        add_ew("%s_far%s" % (_b, _far), _b, _far, "binary")

# reductions: ADD on every variant, MAX on one variant per real data type; far A with the far stride on a kept mode or on a reduced one (as
# the base case's slowest mode of A is), far D without and with a split (the partials go through the finalize kernel into a far D)
_RED = ["f32_red_col_add", "f32_red_col_digits_add", "f32_red_col_split_add", "f32_red_row_add", "f32_red_row_split_add", "f32_red_gen_split_add",
        "f32_red_gen_digits_add", "f32_red_rowany_add", "f32_red_rowany_split_add", "f32_red_rowany_digits_add", "f32_red_acc64_gen_split_add",
        "f32_red_acc64_rowany_split_add", "f32_red_col_max", "f32_red_rowany_split_max"]
for _dt in ("float64", "bfloat16", "float16", "complex64", "complex128"):
    _sh = ew.SHORT[_dt]
    _RED += ["%s_red_col_add" % _sh, "%s_red_col_split_add" % _sh, "%s_red_row_add" % _sh, "%s_red_row_split_add" % _sh]
    if _dt not in ew.CPLX:
        _RED += ["%s_red_col_max" % _sh, "%s_red_gen_split_add" % _sh, "%s_red_rowany_add" % _sh]
_RED += ["c64_red_gen_split_add", "c64_red_gen_split_conjA_add", "c128_red_col_odd_split_add"]
for _b in _RED:
    _c = ew.BY_ID[_b]
    _slow_kept = _c.modes["A"][-1] in _c.modes["D"]
    add_ew("%s_farA_%s" % (_b, "kept" if _slow_kept else "reduced"), _b, "A", "reduction")
    if len(_c.modes["D"]) >= 2:
        add_ew("%s_farD" % _b, _b, "D", "reduction")
# far A with the far stride on a reduced slowest mode and on a kept one, for the variants whose base case has only one of the two
def _red_case(dtype, ext, mA, mD, i, compute=None, **want):
    return ew.Case("x", "reduction", dtype, ext, (mA, mD), lambda d: d.get("op") == "reduction" and ew._is(**want)(d), ew._red_runs("ADD", dtype, i), compute=compute)


for _dt in ("float32", "float64", "bfloat16", "complex64"):
    _sh, _nv = ew.SHORT[_dt], ew.NV[_dt]
    add_ew("%s_red_col_slowest_farA_reduced" % _sh, _red_case(_dt, dict(a=16 * _nv, c=6, b=45), "acb", "ac", 0, variant=ew.RED_COL, splitR=1), "A", "reduction")
    add_ew("%s_red_row_slowest_farA_kept" % _sh, _red_case(_dt, dict(b=64 * _nv, a=5, c=3), "bac", "ac", 1, variant=ew.RED_ROW, splitR=1), "A", "reduction")

# far D without and with a split, per variant (named in the predicate): the partials of a split go through the finalize kernel into the far D.
# Every D has two kept modes, so that it has a slowest pitch to inflate.
SPLIT = ew.SPLIT
FAR_D_REDUCTIONS = []
for _dt in ("float32", "float64", "bfloat16", "float16", "complex64", "complex128"):
    _nv = ew.NV[_dt]
    _long = 16392 if _nv == 8 else 16388
    FAR_D_REDUCTIONS += [
        ("col", _dt, dict(a=16 * _nv, b=45, c=6), "abc", "ac", None, dict(variant=ew.RED_COL, splitR=1)),
        ("col_split", _dt, dict(a=8, b=67, c=2), "abc", "ac", None, dict(variant=ew.RED_COL, splitR=SPLIT)),
        ("row", _dt, dict(a=1024 * _nv, b=3, c=2), "abc", "bc", None, dict(variant=ew.RED_ROW, splitR=1)),
        ("row_split", _dt, dict(a=_long, b=3, c=2), "abc", "bc", None, dict(variant=ew.RED_ROW, splitR=SPLIT))]
    if _dt != "complex128":           # (a complex128 lane holds one element: always tiled)
        FAR_D_REDUCTIONS += [
            ("gen", _dt, dict(a=33, b=7, c=5), "abc", "ac", None, dict(variant=ew.RED_GENERIC, splitR=1)),
            ("gen_split", _dt, dict(a=33, b=131, c=2), "abc", "ac", None, dict(variant=ew.RED_GENERIC, splitR=SPLIT))]
    if _dt not in ew.CPLX:
        FAR_D_REDUCTIONS += [
            ("rowany", _dt, dict(a=77, b=5, c=3), "abc", "bc", None, dict(variant=ew.RED_GENERIC, rowAny=1, splitR=1)),
            ("rowany_split", _dt, dict(a=8195, b=3, c=2), "abc", "bc", None, dict(variant=ew.RED_GENERIC, rowAny=1, splitR=SPLIT))]
# fp32 accumulated in fp64
FAR_D_REDUCTIONS += [
    ("acc64_gen", "float32", dict(a=33, b=7, c=5), "abc", "ac", "64F", dict(variant=ew.RED_GENERIC, rowAny=0, splitR=1)),
    ("acc64_gen_split", "float32", dict(a=64, b=131, c=2), "abc", "ac", "64F", dict(variant=ew.RED_GENERIC, rowAny=0, splitR=SPLIT)),
    ("acc64_rowany", "float32", dict(a=77, b=5, c=3), "abc", "bc", "64F", dict(variant=ew.RED_GENERIC, rowAny=1, splitR=1)),
    ("acc64_rowany_split", "float32", dict(a=16388, b=3, c=2), "abc", "bc", "64F", dict(variant=ew.RED_GENERIC, rowAny=1, splitR=SPLIT))]
for _i, (_n, _dt, _ext, _mA, _mD, _cmp, _want) in enumerate(FAR_D_REDUCTIONS):
    add_ew("%s_red_%s_far_D" % (ew.SHORT[_dt], _n), _red_case(_dt, _ext, _mA, _mD, _i, compute=_cmp, **_want), "D",
           "reduction far D, split" if _want["splitR"] != 1 else "reduction far D")

# the converting kernels: two widening and two narrowing pairs x row copy, transposition, gather; the binary form with a far C
for _pair in (("bfloat16", "float32"), ("float32", "float64"), ("float32", "bfloat16"), ("float64", "float32")):
    _pn = cv._name(_pair)
    for _b, _fars in (("perm_rowcopy", "AD"), ("perm_transpose", "AD"), ("perm_generic", "AD"), ("bin_transpose_add", "ACD"), ("bin_generic_pad_min", "ACD")):
        for _far in _fars:
            add_ew("%s_%s_far%s" % (_pn, _b, _far), cv.BY_ID["%s_%s" % (_pn, _b)], _far, "converting")

# complex trinary: the tiled forms (E = A, row copy, two tiles, two passes) and the gather kernel, each tensor far in turn
for _prefix in ("c64_tri_e_is_a_", "c128_tri_e_is_a_", "c64_tri_rowcopy_", "c128_tri_two_tiles_", "c64_tri_two_tiles_", "c128_tri_two_pass_", "c64_tri_two_pass_odd_",
                "c64_tri_gather_e_", "c64_tri_gather_two_pass_"):
    _b = next(c for c in ct3.CASES if c.id.startswith(_prefix) and not any(c.conj3))
    _e_form = any(x in _prefix for x in ("_e_is_a_", "_rowcopy_", "_gather_e_"))
    for _far in "ABCD":
        # (the one-pass E forms need A in D's layout: with a far A or a far D the plan is the two-pass form, on the same kernels)
        _exp = None
        if _e_form and _far in "AD":
            _exp = ct3._want(passes=2, variant_inplace=ew.EW_GENERIC)
        add_ew("%s_far%s" % (_b.id, _far), _b, _far, "complex trinary gather" if "gather" in _prefix else "complex trinary tiled", expect=_exp)

EW_BY_ID = {c.id: c for c in EW_CASES}


# ---- running a contraction case ------------------------------------------------------------------------------------------------------------
LAUNCHES = []        # (section, kernel name or element-wise variant, case id) of every launch


def make_plan(ct, ops, h, case, algo=None):
    e, m = case.extents, case.modes
    kw = dict(workspace_limit=case.ws_limit)
    if algo is not None:
        kw["algo"] = algo
    if case.compute:
        kw["compute"] = case.compute
    conj = [ct.OP_CONJ if c else ct.OP_IDENTITY for c in (case.conjA, case.conjB, case.conjC)]
    if case.real is not None:
        kw["dtypeA" if case.real == 0 else "dtypeB"] = ct.R_64F
    with wc.hook_env(case):
        return ops.contraction_plan(h, e(m[0]), m[0], e(m[1]), m[1], e(m[2]), m[2], dtype=xc._dt(ct, case.dtype), strideA=case.strides("A"),
                                    strideB=case.strides("B"), strideC=case.strides("C"), strideD=case.strides("D"), alignment=case.align or 128,
                                    opA=conj[0], opB=conj[1], opC=conj[2], **kw)


def plans(ct, ops, h, case):
    """(rank, plan, description) of every plan the case runs: the planner's choice, or every rank below 12 on the kernel the case sweeps"""
    if case.sweep is None:
        p = make_plan(ct, ops, h, case)
        return [(None, p, wc.describe(ct, p))]
    out = []
    for r in range(256 if case.flat else 12):
        try:
            p = make_plan(ct, ops, h, case, algo=r)
        except ct.CuTensorError:
            break
        d = wc.describe(ct, p)
        if d.get("kname") == case.sweep and (not case.flat or (d.get("splitK", 1) > 1 and (d.get("bm"), d.get("bn"), d.get("pf"), d.get("nt")) == (96, 96, 3, 0))):
            out.append((r, p, d))
            if case.flat:
                break
        else:
            p.destroy()
    return out


def plan_paths(ct, ops, h, case):
    """every plan of the case is on its path and obeys the routing rules; at least one plan; returns the descriptions"""
    q = check_sides(case)
    ps = plans(ct, ops, h, case)
    try:
        assert ps, "%s: no rank below 12 plans %s" % (case.id, case.sweep)
        for r, p, d in ps:
            assert case.expect(d), "%s (rank %s) is off its path: %s" % (case.id, r, d)
            check_routing(case, d, q)
    finally:
        for _, p, _ in ps:
            p.destroy()
    return [d for _, _, d in ps]


_HOST = {}


def check_rc64_draw(case, A, B, C):
    """the mixed cases' draws: the real operand real fp64, every part of every element an integer of {+-1, +-2, +-3} (C: [-3, 3]), and the
    largest possible |sum| (times |alpha|, plus |beta c|, by parts) below 2^53"""
    import torch
    assert (A.dtype, B.dtype) == tuple(xd.TORCH_DTYPES[d] for d in case.dtypes()) and C.dtype == torch.complex128, case.id
    for x, lo in ((A, 1), (B, 1), (C, 0)):
        for part in ((x.real, x.imag) if x.is_complex() else (x,)):
            assert bool((part == part.round()).all()) and lo <= float(part.abs().min()) and float(part.abs().max()) <= 3, case.id
    m = xd.Modes(*case.modes[:3])
    k = int(np.prod([case.ext[c] for c in m.K])) if m.K else 1
    l1 = lambda z: abs(complex(z).real) + abs(complex(z).imag)   # noqa: E731
    assert l1(case.alpha) * k * 3 * 6 + l1(case.beta) * 6 < 2.0 ** 53, case.id


def _host(case, swap):
    key = (case.data_key, swap)
    if key not in _HOST:
        if len(_HOST) >= 2:
            _HOST.clear()
        if case.real is not None:
            A, B, C = rc.make_inputs(case, swap)
            check_rc64_draw(case, A, B, C)
            ref = rc.reference(case, A, B, C)
        else:
            A, B, C = xd.make_exact(case, swap)
            xd.check_draw(case, A, B, C, swap)
            ref = xd.exact_reference(case, A, B, C)
        _HOST[key] = (A, B, C, xd.expected(case, ref)[0])
    return _HOST[key]


def _place(case, t, arena):
    e = case.extents(case.tmodes(t))
    if t == case.far:
        return arena.place(e, case.strides(t), case.tdtype(t), case.off)
    return xc.Placed(e, case.tdtype(t), off=case.off, strides=case.strides(t))


def run_case(ct, ops, h, case, arena):
    import torch
    ps = plans(ct, ops, h, case)
    out = []
    try:
        assert ps, "%s: no rank below 12 plans %s" % (case.id, case.sweep)
        for rank, plan, d in ps:
            assert case.expect(d) and case.gpu_expect(d), "%s (rank %s) is off its path: %s" % (case.id, rank, d)
            check_routing(case, d)
            ws = torch.empty(max(plan.required_workspace, 256), dtype=torch.uint8, device="cuda")
            for swap in (False, True):
                A, B, C, want = _host(case, swap)
                what = "%s (rank %s, draw %d) %s" % (case.id, rank, int(swap), d)
                dev = {"A": _place(case, "A", arena), "B": _place(case, "B", arena), "D": _place(case, "D", arena)}
                host = {"A": A, "B": B}
                if case.beta:
                    dev["C"], host["C"] = _place(case, "C", arena), C
                for t, x in host.items():
                    dev[t].set(x)
                flat0 = ct.flat_start_count() if case.flat else 0
                plan.contract(case.alpha, dev["A"].ptr, dev["B"].ptr, case.beta, dev["C"].ptr if case.beta else 0, dev["D"].ptr, ws.data_ptr(),
                              plan.required_workspace)
                torch.cuda.synchronize()
                assert not case.flat or ct.flat_start_count() == flat0 + 1, "%s: the launch did not take the flat entry" % what
                got = {t: p.get() for t, p in dev.items()}
                for t, p in dev.items():                                  # (the far tensor: re-poisoned, then the whole arena)
                    p.check_outside("%s: outside %s" % (what, t))
                xd.assert_exact(got["D"], want, what)
                for t, x in host.items():
                    xd.assert_exact(got[t], x, "%s: input %s changed" % (what, t))
                LAUNCHES.append((case.section, d.get("kname") + (" split-K" if d.get("splitK", 1) > 1 else "") + (" flat" if case.flat else ""), case.id))
            out.append(d)
    except BaseException:
        arena.reset()
        raise
    finally:
        for _, p, _ in ps:
            p.destroy()
    return out


# ---- running an element-wise or reduction case (the steps of ew_exact_cases.run_case, one tensor in the arena) --------------------------------
def _ew_placed(case, t, arena, layout=None):
    lt = layout or t
    if lt == case.far:
        return arena.place(case.extents(lt), case.strides(lt), case.tdtype(t), case.off)
    return xc.Placed(case.extents(lt), case.tdtype(t), off=case.off, strides=case.strides(lt))


def ew_plan(ct, ops, h, case):
    return {"plain": ew.make_plan, "convert": cv.make_plan, "cplx_trinary": ct3.make_plan}[case.flavour](ct, ops, h, case)


def ew_plan_path(ct, ops, h, case):
    """the plan is on the path the case names (the planner needs no GPU); returns the description"""
    plan = ew_plan(ct, ops, h, case)
    try:
        d = wc.describe(ct, plan)
        assert case.expect(d), "%s is off its path: %s" % (case.id, d)
        return {k: v for k, v in d.pairs}
    finally:
        plan.destroy()


def ew_check_case(case, d):
    """the data conditions of every draw and run, by the self-checks of the table the case comes from; returns the number of draws"""
    if case.flavour == "convert":
        cv.check_case(case)
    elif case.flavour == "cplx_trinary":
        ct3.check_case(case)
    else:
        return ew.check_case(case, d)
    return 2


def _ew_reference(case, ins, run, d):
    if case.flavour == "cplx_trinary":
        ct3.check_run(case, run)
        return ct3.reference(case, ins, run)
    ew.check_draw(case, ins, run, d)
    return ew.reference(case, ins, run)


def run_ew_case(ct, ops, h, case, arena):
    import torch
    plan = ew_plan(ct, ops, h, case)
    try:
        desc = wc.describe(ct, plan)
        assert case.expect(desc), "%s is off its path: %s" % (case.id, desc)
        d = {k: v for k, v in desc.pairs}
        ws = torch.empty(max(plan.required_workspace, 256), dtype=torch.uint8, device="cuda")
        for draw in range(ew.n_draws(case, d)):
            ins = ew.make_draw(case, draw, d)
            for run in case.runs:
                scal, cmode = run
                want = ew.expected(case, _ew_reference(case, ins, run, d))
                what = "%s (draw %d, scalars %s, C %s) %s" % (case.id, draw, scal, cmode, desc)
                dev, host = {}, {}
                for t in ew.TENSORS[case.kind][:-1]:
                    if t != "C":
                        dev[t], host[t] = _ew_placed(case, t, arena), cv.host(ins[t], case.tdtype(t))
                        dev[t].set(host[t])
                pd = dev["D"] = _ew_placed(case, "D", arena)
                if cmode == "inplace":
                    pd.set(cv.host(ins["C"], case.dtype))
                elif cmode == "separate":
                    dev["C"], host["C"] = _ew_placed(case, "C", arena, "C" if "C" in case.modes else "D"), cv.host(ins["C"], case.dtype)
                    dev["C"].set(host["C"])
                cptr = dev["C"].ptr if "C" in dev else pd.ptr
                if case.kind == "permutation":
                    plan.permute(scal[0], dev["A"].ptr, pd.ptr)
                elif case.kind == "binary":
                    plan.binary(scal[0], dev["A"].ptr, scal[1], cptr, pd.ptr)
                elif case.kind == "trinary":
                    plan.trinary(scal[0], dev["A"].ptr, scal[1], dev["B"].ptr, scal[2], cptr, pd.ptr)
                else:
                    plan.reduce(scal[0], dev["A"].ptr, scal[1], cptr, pd.ptr, ws.data_ptr(), plan.required_workspace)
                torch.cuda.synchronize()
                got = {t: p.get() for t, p in dev.items()}
                for t, p in dev.items():
                    p.check_outside("%s: outside %s" % (what, t))
                xd.assert_exact(got["D"], want, what)
                for t, x in host.items():
                    xd.assert_exact(got[t], x, "%s: input %s changed" % (what, t))
                LAUNCHES.append((case.section, "%s variant %s" % (d.get("form") or d.get("op"), d.get("variant")), case.id))
    except BaseException:
        arena.reset()
        raise
    finally:
        plan.destroy()
    return d


# every section of the two tables and what a full run must have launched in it: each entry is a kernel label (or a part of one) of LAUNCHES
_GEN = lambda k: [k, k + " split-K"]          # noqa: E731
SECTIONS = {
    "f32 ring": [RING], "f32 RAG twin": [RING], "f32 register kernel": [REG], "f32 far C/D": [RING, REG], "f32 split-K fold": [" split-K"],
    "f32 flat-entry fold": [RING + " split-K flat"],
    "general family f64": _GEN(GENK), "general family c64": _GEN(GENK), "general family c128": _GEN(GENK), "general family f32x": _GEN("gett_gen_f32x_kernel"),
    "general family c32x": _GEN("gett_gen_c32x_kernel"), "general family rc64": _GEN("gett_gen_rc64_kernel"), "general family f64x": _GEN("gett_gen_f64x_kernel"),
    "16-bit family 1": ["gett_h16"], "16-bit general family": _GEN(GENK),
    "16-bit forced variants": [xc.H16_VARIANTS[w] for w in ("4p", "4m", "4m4", "8m", "4q")],
    "mode-table kernel": [TABLE], "gett_simple": [SIMPLE],
    "permutation": ["elementwise variant %d" % v for v in range(5)], "binary": ["elementwise variant %d" % v for v in (0, 1, 2, 4)],
    "converting": ["elementwise variant %d" % v for v in (0, 1, 2)],
    "complex trinary tiled": ["trinary variant 0", "trinary variant 1"], "complex trinary gather": ["trinary variant 2"],
    "reduction": ["reduction variant %d" % v for v in range(3)], "reduction far D": ["reduction variant %d" % v for v in range(3)],
    "reduction far D, split": ["reduction variant %d" % v for v in range(3)]}
assert set(SECTIONS) == {c.section for c in CASES} | {c.section for c in EW_CASES}, set(SECTIONS) ^ ({c.section for c in CASES} | {c.section for c in EW_CASES})


def missing_launches(launches):
    """(section, label) of SECTIONS that no launch matches"""
    got = summary(launches)
    return [(sec, want) for sec, wants in SECTIONS.items() for want in wants if not any(want in k for k in got.get(sec, {}))]


def summary(launches):
    """section -> {kernel: launches}"""
    out = {}
    for sec, k, _ in launches:
        out.setdefault(sec, {})
        out[sec][k] = out[sec].get(k, 0) + 1
    return out


def free_memory_ok():
    import torch
    return torch.cuda.mem_get_info()[0] >= 20 << 30


if __name__ == "__main__":
    # `python far_cases.py run|plan ids...`: the cases whose switch the library reads once per process, with an arena of their own
    from cudalibrarysamples_amd import cutensor as ct_, ops as ops_
    mode_ = sys.argv[1]
    h_ = ops_.Handle()
    arena_ = None
    if mode_ == "run":
        assert free_memory_ok(), "less than 20 GiB of device memory free"
        arena_ = Arena()
    for cid in sys.argv[2:]:
        if mode_ == "plan":
            plan_paths(ct_, ops_, h_, BY_ID[cid])
        else:
            run_case(ct_, ops_, h_, BY_ID[cid], arena_)
        print("ok", cid, flush=True)
    print("LAUNCHES", json.dumps(LAUNCHES))
