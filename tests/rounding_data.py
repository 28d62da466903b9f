"""Integer-valued data on which the final rounding of a 16-bit output is what is tested (tests/test_round16_data_cpu.py proves that the
data discriminates, tests/test_gpu_round16_exact.py runs the kernels on it) — a helper module, not a conftest, the sibling of
tests/exact_data.py.

tests/exact_data.py keeps 16-bit sums inside the type's exact integer range, so that nothing rounds and any summation order gives the
same bits.  Here the fp32 accumulator is still exact (check_draw's bound, below 2^24, is asserted before a launch), but the sums are
large and odd: most of them are NOT values of the output type, and the one step that is left, rnd16(alpha * acc + beta * c), is compared
bit for bit.  Truncation, round-half-away, round-half-up and a second rounding all stay within 1 ulp: the tolerance tests cannot see them.

make_rounding(case, swap): magnitudes uniform in 1 .. V, V = floor(sqrt(4 * 2^14 / K)) capped at 255 (bf16) / 2047 (fp16); one operand
all positive; the other gets one sign per row (an index of its modes that are not contracted) and a per-row share, up to a half, of its
entries flipped: |sum| is about 2^14 (1 - 2 share), spread over several binades.  `swap` puts the signed operand on the other side.  C:
integers of the type's exact range.
make_beta(case, swap): the same A and B; C holds odd integers of [-15, 15] for beta = 2^-14 (below).

round16(x, dtype, rule): x (fp64, exact) rounded to the 16-bit type by one of four rules — "even" is the correct one; "trunc", "away"
(half away from zero) and "up" (half towards +inf) are the defects the data must expose.  Past the largest finite value: +-inf.
expected_rounded(): the exact reference rounded ONCE (exact_data.round_to: fp64 -> fp32 is exact here), with the counts of outputs that
round, overflow and are exact ties (by sign and direction); asserts ON THE REFERENCE that at least half of a case's outputs round (cases
of fewer than 1024 outputs are exempt) and at most 1 % overflow.

beta below fp32's last place: x = S + beta * c with S an integer, c odd, beta = 2^-14 is exact in fp64 but no value of fp32 once
|S| >= 2^10.  Where S is a tie of the 16-bit type and beta * c is lost in fp32, r1 = rnd16(x) follows the sign of c and
r2 = rnd16(rnd32(x)) goes to even.  expected_beta(): fp16 gives r1 (one rounding of the fused multiply-add, v_fma_mixlo_f16), bf16 gives
r2 (an fp32 fma, then one conversion); at least 64 outputs of every case tell the two apart."""
import numpy as np
import torch

import exact_data as xd

RANGE = {"bfloat16": 256, "float16": 2048}               # integers up to here are values of the type
FRACTION_BITS = {"bfloat16": 7, "float16": 10}
MIN_EXPONENT = {"bfloat16": -126, "float16": -14}
MAX_FINITE = {"bfloat16": float(torch.finfo(torch.bfloat16).max), "float16": 65504.0}
TARGET = 4 * 2 ** 14                                     # K * V^2: the mean |a| |b| is V^2 / 4, so sum |a| |b| is about 2^14
BETA = 2.0 ** -14
RULES = ("even", "trunc", "away", "up")
MIN_ROUNDING, MAX_OVERFLOW, MIN_TIES, SMALL, MIN_DIFFER = 0.5, 0.01, 1000, 1024, 64
MIN_TOLD_APART = 16                                      # outputs in which a wrong rounding must differ from the right one


def magnitude(dtype, terms):
    """V: the largest magnitude of an operand's entries for `terms` products per output"""
    return int(max(1, min(RANGE[dtype] - 1, np.floor(np.sqrt(TARGET / terms)))))


def _signed(rng, modes_x, ext, k_modes, V):
    """magnitudes 1 .. V; one sign per row (an index of the modes outside k_modes), a share of up to a half of the row's entries flipped"""
    shape = [ext[c] for c in modes_x]
    k_axes = [modes_x.index(c) for c in k_modes]
    r_axes = [i for i in range(len(shape)) if i not in k_axes]
    K = int(np.prod([shape[i] for i in k_axes])) if k_axes else 1
    R = int(np.prod([shape[i] for i in r_axes])) if r_axes else 1
    x = rng.integers(1, V + 1, size=(R, K)).astype(np.int16)
    x *= (rng.integers(0, 2, size=(R, 1)) * 2 - 1).astype(np.int16)
    x[rng.random((R, K), dtype=np.float32) < 0.5 * rng.random((R, 1), dtype=np.float32)] *= -1
    x = x.reshape([shape[i] for i in r_axes] + [shape[i] for i in k_axes])
    return np.ascontiguousarray(np.transpose(x, np.argsort(r_axes + k_axes)))


def _operands(case, swap):
    m = xd.Modes(*case.modes[:3])
    assert case.dtype in xd.H16 and not m.loneA and not m.loneB, case.id
    ext = case.ext
    V = magnitude(case.dtype, int(np.prod([ext[c] for c in m.K])) if m.K else 1)
    ra, rb = xd._rng(case, swap, 10), xd._rng(case, swap, 11)
    if not swap:
        A = _signed(ra, m.A, ext, m.K, V)
        B = rb.integers(1, V + 1, size=[ext[c] for c in m.B]).astype(np.int16)
    else:
        A = ra.integers(1, V + 1, size=[ext[c] for c in m.A]).astype(np.int16)
        B = _signed(rb, m.B, ext, m.K, V)
    return xd._to_torch(A, case.dtype), xd._to_torch(B, case.dtype), [ext[c] for c in m.C]


def make_rounding(case, swap=False):
    """(A, B, C) as exact_data.make_exact gives them, for the rounding regime"""
    A, B, sC = _operands(case, swap)
    R = RANGE[case.dtype]
    C = xd._rng(case, swap, 12).integers(-R, R + 1, size=sC).astype(np.int16)
    return A, B, xd._to_torch(C, case.dtype)


def make_beta(case, swap=False):
    A, B, sC = _operands(case, swap)
    C = (2 * xd._rng(case, swap, 12).integers(-8, 8, size=sC) + 1).astype(np.int16)          # odd, -15 .. 15
    return A, B, xd._to_torch(C, case.dtype)


# ---- rounding rules on exact fp64 values --------------------------------------------------------------------------------------------------
def _grid(x, dtype):
    """x = q * u with u the spacing of the 16-bit type at x (subnormals: the smallest normal binade's): q is exact"""
    x = np.asarray(x, dtype=np.float64)
    _, e = np.frexp(np.abs(x))                                        # |x| = m 2^e, m in [0.5, 1)
    u = np.ldexp(1.0, np.maximum(e - 1, MIN_EXPONENT[dtype]) - FRACTION_BITS[dtype])
    return x / u, u


def round16(x, dtype, rule="even"):
    q, u = _grid(x, dtype)
    lo = np.floor(q)
    frac = q - lo
    if rule == "even":
        r = lo + ((frac > 0.5) | ((frac == 0.5) & (np.mod(lo, 2) == 1)))
    elif rule == "trunc":
        r = np.trunc(q)
    elif rule == "away":
        r = np.sign(q) * np.floor(np.abs(q) + 0.5)
    else:
        assert rule == "up", rule
        r = np.floor(q + 0.5)
    out = r * u
    return np.where(np.abs(out) > MAX_FINITE[dtype], np.copysign(np.inf, out), out)


def through_fp32(x):
    """rnd32(x): what an fp32 fused multiply-add leaves of the exact value"""
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def counts(ref, want, dtype):
    """[outputs, outputs that round, outputs that overflow, ties: positive to-even-down, positive up, negative down, negative up]
    (down / up: towards / away from zero)"""
    ref, want = np.asarray(ref, dtype=np.float64), np.asarray(want, dtype=np.float64)
    q, _ = _grid(ref, dtype)
    over = np.isinf(want)
    tie = (q - np.floor(q) == 0.5) & ~over
    up = np.abs(want) > np.abs(ref)
    return [int(ref.size), int((want != ref).sum()), int(over.sum()), int((tie & (ref > 0) & ~up).sum()), int((tie & (ref > 0) & up).sum()),
            int((tie & (ref < 0) & ~up).sum()), int((tie & (ref < 0) & up).sum())]


def check_share(case_id, n, rounds, over, least):
    assert n < SMALL or rounds >= least * n, "%s: only %d of %d exact outputs round (at least %.0f %% must)" % (case_id, rounds, n, 100 * least)
    assert over <= MAX_OVERFLOW * n, "%s: %d of %d outputs overflow" % (case_id, over, n)


def expected_rounded(case, ref):
    """(the exact value rounded once to the output type; counts()) — the conditions are asserted on the reference, never on a result"""
    assert float(ref.abs().max()) < 2.0 ** 24 and bool((ref == ref.round()).all()), case.id      # fp64 -> fp32 is exact
    want = xd.round_to(ref, case.dtype)
    c = counts(ref.numpy(), want.numpy(), case.dtype)
    check_share(case.id, c[0], c[1], c[2], MIN_ROUNDING)
    return want, c


def beta_rules(case, ref):
    """r1 = rnd16(x), r2 = rnd16(rnd32(x)) of the exact x; which of them the type's contract names"""
    x = ref.numpy()
    r1, r2 = round16(x, case.dtype), round16(through_fp32(x), case.dtype)
    return (r2, r1) if case.dtype == "bfloat16" else (r1, r2)            # (the contract, the other rule)


def expected_beta(case, ref):
    want, other = beta_rules(case, ref)
    differ = int((want != other).sum())
    assert differ >= MIN_DIFFER, "%s: one and two roundings differ at %d outputs only" % (case.id, differ)
    return torch.from_numpy(want), counts(ref.numpy(), want, case.dtype) + [differ]


# ---- statistics of a session ---------------------------------------------------------------------------------------------------------------
def summary(stats):
    """stats: (part, data type, case id, counts) -> per part and data type: runs, the smallest share of rounding outputs among the cases of
    1024 outputs or more, the four tie counts"""
    out = {}
    for part, dt, _, c in stats:
        runs, share, ties = out.get((part, dt), (0, 1.0, [0, 0, 0, 0]))
        if c[0] >= SMALL:
            share = min(share, c[1] / c[0])
        out[(part, dt)] = (runs + 1, share, [a + b for a, b in zip(ties, c[3:7])])
    return out


def check_ties(stats, parts=None):
    """per part and data type over the whole session: at least 1000 exact ties of each kind — to-even-down and to-even-up, of both signs;
    prints the report"""
    rep = summary(stats)
    for (part, dt), (runs, share, ties) in sorted(rep.items()):
        print("round16 %-12s %-9s: %4d runs, smallest share of outputs that round %.3f, ties +down %d +up %d -down %d -up %d" % (
            part, dt, runs, share, *ties))
    for (part, dt), (runs, share, ties) in sorted(rep.items()):
        if parts is None or part in parts:
            assert min(ties) >= MIN_TIES, (part, dt, ties)
    return rep
