"""Integer-valued data for the contraction kernels: generator, reference and comparator (tests/test_exact_data_cpu.py checks the data,
tests/test_gpu_exact.py runs every contraction path on it) — a helper module, not a conftest.

On data whose products and partial sums are all exactly representable in the accumulator, floating-point addition is associative: any
correct kernel — any tile order, split-K factor, fold, atomics order, MFMA shape — returns exactly the integer answer.  The tolerance is
zero, and one wrong, missing or doubled product anywhere fails.

make_exact(case, swap): A, B, C of the case's data type, all values integers, fixed seed.
  * fp32 / fp64 / complex data: both operands dense, values (complex: both parts) from {+-1, +-2, +-3}.
  * 16-bit data: one operand dense +-1; the other carries +-1 at a density that keeps about 1024 non-zero terms per output (bf16 holds
    integers exactly only up to 256, fp16 up to 2048: |sum| then has sigma = 32) — and at least one non-zero at every contracted index, so
    that no element of the dense operand is multiplied by zeros only.  `swap` exchanges the roles: the second draw of each case.
  * C: integers in [-3, 3].
check_draw(): every element of the dense operand non-zero, every contracted index live in the other one, and the accumulator bound —
for every output sum_k |a| |b| (times max(1, |alpha|), plus |beta c|) stays below 2^24 where the kernel accumulates in fp32 (fp32, bf16,
fp16, complex64 data) and below 2^53 for fp64 / complex128; one binary digit less when alpha or beta is a half.  The bound is computed
from the draw (the largest |a| over A's free modes times the largest |b| over B's, summed over the contracted indices: an upper bound of
every output's sum) and asserted before anything is launched.

exact_reference(): the integer result.  Small cases: numpy.einsum on int64 (complex: int64 planes).  Larger ones: an fp64 einsum — exact
on this data in any order, so BLAS on the CPU or on the device both qualify — plus 4096 sampled outputs recomputed as plain int64 dot
products that go through no BLAS.  Lone modes of 16-bit data (modes of one operand only) are reduced into a 16-bit temporary by the
library (contraction_route.cpp, split_lone_modes): the reference rounds the exact lone-mode sum once to the data type, then contracts exactly.
expected(): the exact value rounded once (to nearest even) to the output type, and the share of outputs that this rounding changes: at
most 1 % for 16-bit outputs, none for the others; asserted on the reference, never on a kernel's result.

assert_exact(got, want): equal as numbers at every element (-0 = +0), no tolerance."""
import zlib

import numpy as np
import torch

TORCH_DTYPES = {"bfloat16": torch.bfloat16, "float16": torch.float16, "float32": torch.float32, "float64": torch.float64,
                "complex64": torch.complex64, "complex128": torch.complex128}
H16 = ("bfloat16", "float16")
TERMS_16 = 1024                                            # non-zero terms per output of 16-bit data
INT64_WORK = 2.5e8                                         # multiply-adds up to which numpy.einsum on int64 computes every output
SAMPLES = 4096
MAX_UNREPRESENTABLE = 0.01


def acc_limit(dtype):
    return 2.0 ** 53 if dtype in ("float64", "complex128") else 2.0 ** 24


class Modes:
    """the mode groups of a contraction 'A, B -> C' (labels as characters)"""

    def __init__(self, mA, mB, mC):
        self.A, self.B, self.C = mA, mB, mC
        self.K = [c for c in mA if c in mB and c not in mC]                  # contracted
        self.loneA = [c for c in mA if c not in mB and c not in mC]          # summed out of A alone
        self.loneB = [c for c in mB if c not in mA and c not in mC]
        self.eq = "%s,%s->%s" % (mA, mB, mC)


def _rng(case, swap, what):
    return np.random.default_rng([zlib.crc32(case.data_key.encode()), int(swap), what])


def _dense(rng, shape, values):
    v = np.asarray(values, dtype=np.int8)
    return v[rng.integers(0, len(v), size=shape, dtype=np.int8 if len(v) < 127 else np.int64)]


def _sparse_pm1(rng, modes_x, ext, k_modes, density, one_per_k):
    """+-1 at `density`, every index of the contracted modes live: a dead one gets one entry at a random place of the other modes"""
    shape = [ext[c] for c in modes_x]
    k_axes = [modes_x.index(c) for c in k_modes]
    r_axes = [i for i in range(len(shape)) if i not in k_axes]
    K = int(np.prod([shape[i] for i in k_axes])) if k_axes else 1
    R = int(np.prod([shape[i] for i in r_axes])) if r_axes else 1
    sign = (rng.integers(0, 2, size=(K, R), dtype=np.int8) * 2 - 1).astype(np.int8)
    if one_per_k:        # exactly one entry per contracted index, no two in one place of the other modes where they fit
        x = np.zeros((K, R), dtype=np.int8)
        x[np.arange(K), np.arange(K) % R] = sign[np.arange(K), np.arange(K) % R]
    else:
        keep = rng.random((K, R), dtype=np.float32) < density if density < 1.0 else np.ones((K, R), dtype=bool)
        x = np.where(keep, sign, np.int8(0))
        dead = np.flatnonzero(~keep.any(axis=1))
        at = rng.integers(0, R, size=dead.size)
        x[dead, at] = sign[dead, at]
    x = x.reshape([shape[i] for i in k_axes] + [shape[i] for i in r_axes])
    return np.ascontiguousarray(np.transpose(x, np.argsort(k_axes + r_axes)))


def _to_torch(x, dtype):
    t = TORCH_DTYPES[dtype]
    if isinstance(x, tuple):
        return torch.complex(torch.from_numpy(x[0]).to(torch.float64), torch.from_numpy(x[1]).to(torch.float64)).to(t)
    return torch.from_numpy(x).to(t)


def make_exact(case, swap=False):
    """(A, B, C): logical CPU tensors (dimensions in the order of the case's mode strings) of the case's data type"""
    m = Modes(*case.modes[:3])
    ext, dtype = case.ext, case.dtype
    sA, sB, sC = ([ext[c] for c in x] for x in (m.A, m.B, m.C))
    if dtype in H16:
        nk = int(np.prod([ext[c] for c in m.K])) if m.K else 1
        density = min(1.0, TERMS_16 / nk)
        dense_vals = case.dense_values or (-1, 1)
        if not swap:
            A = _dense(_rng(case, swap, 0), sA, dense_vals)
            B = _sparse_pm1(_rng(case, swap, 1), m.B, ext, m.K, density, case.one_per_k)
        else:
            B = _dense(_rng(case, swap, 1), sB, dense_vals)
            A = _sparse_pm1(_rng(case, swap, 0), m.A, ext, m.K, density, case.one_per_k)
    elif TORCH_DTYPES[dtype].is_complex:
        vals = (-3, -2, -1, 1, 2, 3)
        ra, rb = _rng(case, swap, 0), _rng(case, swap, 1)
        A = (_dense(ra, sA, vals), _dense(ra, sA, vals))
        B = (_dense(rb, sB, vals), _dense(rb, sB, vals))
    else:
        vals = (-3, -2, -1, 1, 2, 3)
        A, B = _dense(_rng(case, swap, 0), sA, vals), _dense(_rng(case, swap, 1), sB, vals)
    rc = _rng(case, swap, 2)
    C = rc.integers(-3, 4, size=sC, dtype=np.int8)
    if TORCH_DTYPES[dtype].is_complex:
        C = (C, rc.integers(-3, 4, size=sC, dtype=np.int8))
    return _to_torch(A, dtype), _to_torch(B, dtype), _to_torch(C, dtype)


def _mag(x):
    return (x.real.abs() + x.imag.abs()) if x.is_complex() else x.abs()


def _group_max(x, modes_x, m, lone):
    """the largest |x| over the free modes (summed over the lone ones) per index of the contracted and batch modes"""
    a = _mag(x).to(torch.float64)
    keep = [c for c in modes_x if c in m.K or (c in m.A and c in m.B and c in m.C)]
    lone_dims = [i for i, c in enumerate(modes_x) if c in lone]
    if lone_dims:
        a = a.sum(dim=lone_dims, keepdim=True)
    free = [i for i, c in enumerate(modes_x) if c not in keep and c not in lone]
    if free:
        a = a.amax(dim=free, keepdim=True)
    return a.reshape([x.shape[i] for i, c in enumerate(modes_x) if c in keep]), "".join(keep)


def check_draw(case, A, B, C, swap=False):
    """the invariants of the draw; returns the accumulator bound reached as a fraction of the limit"""
    m = Modes(*case.modes[:3])
    for name, x in (("A", A), ("B", B), ("C", C)):
        w = x.to(torch.complex128 if x.is_complex() else torch.float64)
        parts = (w.real, w.imag) if x.is_complex() else (w,)
        assert all(bool((p == p.round()).all()) for p in parts), "%s: %s holds a value that is not an integer" % (case.id, name)
    dense, other, modes_o = (A, B, m.B) if not swap else (B, A, m.A)
    if dense.is_complex():
        assert bool((dense.real != 0).all()) and bool((dense.imag != 0).all()), "%s: a zero in the dense operand" % case.id
    else:
        assert bool((dense != 0).all()), "%s: a zero in the dense operand" % case.id
    # every contracted index (and every index of the other operand's lone modes) has a non-zero in the other operand
    live_modes = [c for c in modes_o if c in m.K]
    red = [i for i, c in enumerate(modes_o) if c not in live_modes]
    live = _mag(other) != 0
    if red:
        live = live.sum(dim=red) > 0
    assert bool(live.all()), "%s: %d contracted indices are multiplied by zeros only" % (case.id, int((~live).sum()))
    uA, kA = _group_max(A, m.A, m, m.loneA)
    uB, kB = _group_max(B, m.B, m, m.loneB)
    batch = "".join(c for c in kA if c not in m.K)
    bound = float(torch.einsum("%s,%s->%s" % (kA, kB, batch), uA, uB).max()) if (kA or kB) else float(uA * uB)
    alpha, beta = abs(case.alpha), abs(case.beta)
    total = max(1.0, alpha) * bound + beta * float(_mag(C).max()) * (2 if C.is_complex() else 1)
    limit = acc_limit(case.dtype)
    if any(float(s) != round(float(s)) for s in (alpha, beta)):
        limit /= 2                       # halves: one binary digit goes to the fraction
    assert total < limit, "%s: accumulator bound %g is not below %g" % (case.id, total, limit)
    return total / limit


def round_to(x, dtype):
    """x (fp64 / complex128, exact) rounded once, to nearest even, to the data type — back in the wide type"""
    t = TORCH_DTYPES[dtype]
    if dtype in H16:
        # fp64 -> fp32 is exact for |x| < 2^24 in steps of 1/2; fp32 -> 16 bits rounds to nearest even: ONE rounding
        return x.to(torch.float32).to(t).to(torch.float64)
    return x.to(t).to(x.dtype)


def _planes(x):
    w = x.to(torch.complex128 if x.is_complex() else torch.float64).numpy()
    if x.is_complex():
        return np.rint(w.real).astype(np.int64), np.rint(w.imag).astype(np.int64)
    return (np.rint(w).astype(np.int64),)


def _sample_planes(x, modes_x, modes_c):
    """the operand's integer planes with its output modes in front (contiguous: one sample's slice is one block); the other modes' labels"""
    front = [i for i, c in enumerate(modes_x) if c in modes_c]
    rest = [i for i, c in enumerate(modes_x) if c not in modes_c]
    small = torch.int16 if x.dtype in (torch.bfloat16, torch.float16) or float(_mag(x).max()) < 2 ** 15 else torch.int64
    parts = (x.real, x.imag) if x.is_complex() else (x,)
    return tuple(p.to(small).permute(front + rest).contiguous().numpy() for p in parts), "".join(modes_x[i] for i in rest)


def _int_einsum(eq, a, b, conjA=False, conjB=False):
    """numpy.einsum on int64; complex operands as (real, imaginary) planes"""
    e = lambda x, y: np.einsum(eq, x, y, optimize=True)   # noqa: E731  (int64: no BLAS whatever the path)
    if len(a) == 1:
        return (e(a[0], b[0]),)
    ai = -a[1] if conjA else a[1]
    bi = -b[1] if conjB else b[1]
    return e(a[0], b[0]) - e(ai, bi), e(a[0], bi) + e(ai, b[0])


def _from_planes(p):
    if len(p) == 1:
        return torch.from_numpy(np.asarray(p[0], dtype=np.float64))
    return torch.complex(torch.from_numpy(np.asarray(p[0], dtype=np.float64)), torch.from_numpy(np.asarray(p[1], dtype=np.float64)))


def work(case):
    return float(np.prod([float(v) for v in case.ext.values()]))


def _reduce_lone(case, x, modes_x, lone):
    """16-bit data: the library's first step — the lone modes summed (exactly here) and rounded once to the data type"""
    if not lone:
        return x, modes_x
    dims = [modes_x.index(c) for c in lone]
    s = x.to(torch.complex128 if x.is_complex() else torch.float64).sum(dim=dims)
    rest = "".join(c for c in modes_x if c not in lone)
    return (round_to(s, case.dtype) if case.dtype in H16 else s), rest


def contract_exact(case, A, B, device=None):
    """sum over the contracted (and lone) modes, exact, as fp64 / complex128 on the CPU; plus the number of sampled int64 checks done"""
    m = Modes(*case.modes[:3])
    A, mA = _reduce_lone(case, A, m.A, m.loneA)
    B, mB = _reduce_lone(case, B, m.B, m.loneB)
    eq = "%s,%s->%s" % (mA, mB, m.C)
    if work(case) <= INT64_WORK:
        return _from_planes(_int_einsum(eq, _planes(A), _planes(B), case.conjA, case.conjB)), 0
    wide = torch.complex128 if A.is_complex() else torch.float64
    dev = device or "cpu"
    a, b = A.to(dev).to(wide), B.to(dev).to(wide)
    acc = torch.einsum(eq, a.conj() if case.conjA else a, b.conj() if case.conjB else b).cpu()
    del a, b
    # sampled outputs once more as int64 dot products: numpy.einsum on integer slices, no BLAS
    rng = _rng(case, 0, 7)
    ext_c = [case.ext[c] for c in m.C]
    idx = [rng.integers(0, e, SAMPLES) for e in ext_c]
    for i, e in enumerate(ext_c):                  # the last indices of every mode: edge tiles
        idx[i][64 * i: 64 * i + 64] = e - 1 - np.arange(64) % min(e, 8)
    pa, ra = _sample_planes(A, mA, m.C)
    pb, rb = _sample_planes(B, mB, m.C)
    for s in range(SAMPLES):
        at = {c: int(idx[i][s]) for i, c in enumerate(m.C)}
        sa = tuple(at[c] for c in mA if c in at)
        sb = tuple(at[c] for c in mB if c in at)
        want = _int_einsum("%s,%s->" % (ra, rb), tuple(p[sa].astype(np.int64) for p in pa), tuple(p[sb].astype(np.int64) for p in pb),
                           case.conjA, case.conjB)
        got = acc[tuple(at[c] for c in m.C)]
        g = (got.real.item(), got.imag.item()) if acc.is_complex() else (got.item(),)
        assert all(float(w) == v for w, v in zip(want, g)), "%s: the fp64 reference differs from the int64 dot product at %r: %r vs %r" % (
            case.id, at, g, [int(w) for w in want])
    return acc, SAMPLES


def exact_reference(case, A, B, C, device=None):
    """alpha * sum + beta * C, exact (fp64 / complex128 CPU tensor, logical order of C's modes)"""
    acc, _ = contract_exact(case, A, B, device)
    ref = case.alpha * acc
    if case.beta:
        c = C.to(acc.dtype)
        ref = ref + case.beta * (c.conj() if case.conjC else c)
    return ref


def expected(case, ref):
    """(what a correct kernel stores: ref rounded once to the output type; the share of outputs that the rounding changes)"""
    want = round_to(ref, case.dtype)
    share = float((want != ref).sum()) / max(ref.numel(), 1)
    limit = MAX_UNREPRESENTABLE if case.dtype in H16 else 0.0
    assert share <= limit, "%s: %.3f %% of the exact outputs are not values of %s (limit %.1f %%)" % (case.id, 100 * share, case.dtype, 100 * limit)
    return want, share


def assert_exact(got, want, what=""):
    """got == want as numbers at every element (-0 = +0; a NaN never equals); no tolerance.  Reports the count, the first indices and
    got - want there: on integer data the number of products that are missing or doubled."""
    wide = torch.complex128 if (got.is_complex() or want.is_complex()) else torch.float64
    g, w = got.to(wide).cpu(), want.to(wide).cpu()
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = ~(g == w)
    n = int(bad.sum())
    if n:
        where = torch.nonzero(bad)[:8]
        lines = ["  %s: got %r, expected %r, got - expected = %r" % (tuple(int(i) for i in ix), g[tuple(ix)].item(), w[tuple(ix)].item(),
                                                                      (g[tuple(ix)] - w[tuple(ix)]).item()) for ix in where]
        raise AssertionError("%s: %d of %d elements differ from the exact result; the first:\n%s" % (what, n, g.numel(), "\n".join(lines)))
