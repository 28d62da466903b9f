"""The rounding regime of tests/rounding_data.py for the element-wise and reduction entry points: which cases of
tests/ew_exact_cases.py and tests/many_mode_cases.py run in it, their data, scalars and comparator — a helper module, not a conftest
(tests/test_round16_data_cpu.py checks every draw, tests/test_gpu_round16_exact.py runs the cases through the tables' own run_case).

Every 16-bit case whose operators are ADD and MUL takes part, with its own plan, path predicate, pitches, offsets and C placement; MAX and
MIN cannot round.  The exact tables keep every result a value of the type; here most results are not, and the single rounding is compared:
  * cutensorPermute: integers of the upper half of the type's exact range, alpha = +-3.
  * binary / trinary ADD: integers of the exact range (A: of its upper half); the run's scalars keep their signs, the last becomes +-1
    and the others +-2 (2a + c needs 10 bits against bf16's 8); with a MUL among the operators only the first is +-2.  A run without a
    C term: alpha = +-3.  Powers of two keep the two-pass trinary form's 16-bit intermediate alpha * perm(A) exact, as in the exact table.
  * binary / trinary MUL: integers of the upper half of 1 .. MUL_RANGE, so that the product needs more than 8 / 11 bits and stays finite.
  * ADD reductions: magnitudes 1 .. V with V = 2 * 2^14 / (reduced length), capped as in rounding_data, one sign per reduced line and up
    to half of its entries flipped — no clamp into the exact range; ew_exact_cases.check_draw asserts sum |alpha a| + |beta c| < 2^24.
  * MUL reductions: +-1 and two odd factors of MUL_FACTORS per line: the product is odd and beyond the exact range, so it always rounds,
    and every odd product of [256, 512) (bf16) / [2048, 4096) (fp16) is an exact tie; any order of multiplication is exact in fp32.
C: integers of the exact range.  References are ew_exact_cases.reference (numpy int64 / float64) followed by one round_to.  Asserted on the
reference: at least 30 % of the outputs of a run round (runs of fewer than 1024 outputs are exempt, as in rounding_data)."""
import numpy as np
import torch

import ew_exact_cases as ew
import exact_data as xd
import many_mode_cases as mm
import rounding_data as rd

MIN_ROUNDING = 0.3
MUL_RANGE = {"bfloat16": 63, "float16": 127}             # |alpha a * gamma c| <= 2 * 127^2 < 65504
MUL_RANGE_SUM = {"bfloat16": 63, "float16": 100}         # (ADD, MUL) and (MUL, ADD): |(2a + b) c| <= 3 * 100 * 100 < 65504
MUL_FACTORS = {"bfloat16": (17, 63), "float16": (47, 127)}         # the two odd factors of a reduced line: 17^2 > 256, 47^2 > 2048
                                                                   # (17 * 17 = 289 and 47 * 47 = 2209 are tie_target(.., 0), 17 * 19 and 47 * 49 tie_target(.., 1))
STATS = []                                               # ("elementwise", data type, case id, rounding_data.counts()) of every run


def _ops(case):
    return (case.op,) if isinstance(case.op, str) else tuple(case.op)


def takes_part(case):
    """every 16-bit case of the two tables on ADD / MUL; cases with a switch run in process through the hooks, as in their own tables.
    (The one many-mode case with a switch, rev12_gather, is fp32, as are the cases with a unary operator.)"""
    return case.dtype in xd.H16 and all(o in ("ADD", "MUL") for o in _ops(case)) and getattr(case, "un", None) is None


EW = [c for c in ew.CASES if takes_part(c)]
MM = [c for c in mm.CASES if takes_part(c)]
BY_ID = {c.id: c for c in EW + MM}
assert len(BY_ID) == len(EW) + len(MM)


def runs(case):
    if case.kind == "permutation":
        return [((3.0,), "none"), ((-3.0,), "none")]
    if case.kind == "reduction":
        return list(case.runs)                            # exact_cases.SCALARS16: +-1, +-2 already
    out = []
    for scal, cmode in case.runs:
        live = [s for s in scal if s != 0.0]
        top = 3.0 if len(live) == 1 else 2.0
        at = [i for i, s in enumerate(scal) if s != 0.0]
        if all(o == "ADD" for o in _ops(case)):           # 2a + 2b + c: the last term decides the low bits
            big = at[:-1] if len(at) > 1 else at
        else:
            big = at[:1]
        out.append((tuple(0.0 if s == 0.0 else float(np.sign(s)) * (top if i in big else 1.0) for i, s in enumerate(scal)), cmode))
    return out


def _signed_ints(rng, shape, top):
    """magnitudes in the upper half of 1 .. top, random signs"""
    return rng.integers(top // 2, top + 1, size=shape) * (rng.integers(0, 2, size=shape) * 2 - 1)


def make_draw(case, draw, d):
    """ew_exact_cases.make_draw for the rounding regime: numpy int64 tensors by name"""
    R = rd.RANGE[case.dtype]
    ops = _ops(case)
    out = {}
    if case.kind != "reduction":
        top = R if "MUL" not in ops else (MUL_RANGE if case.kind == "binary" else MUL_RANGE_SUM)[case.dtype]
        for i, t in enumerate(ew.TENSORS[case.kind][:-1]):
            rng = ew._rng(case, draw, 10 + i)
            out[t] = rng.integers(-R, R + 1, size=case.extents(t)) if top == R and i else _signed_ints(rng, case.extents(t), top)
        return out
    kept, red, _ = ew._lines(case)
    rng = ew._rng(case, draw, 10)
    out["C"] = ew._rng(case, draw, 12).integers(-R, R + 1, size=case.extents("D"))
    if case.op == "ADD":
        V = int(max(1, min(R - 1, 2 * 2 ** 14 // red)))
        A2 = rng.integers(1, V + 1, size=(kept, red)) * (rng.integers(0, 2, size=(kept, 1)) * 2 - 1)
        A2[rng.random((kept, red)) < 0.5 * rng.random((kept, 1))] *= -1
    else:
        A2 = rng.integers(0, 2, size=(kept, red)) * 2 - 1
        lo, hi = MUL_FACTORS[case.dtype]
        for k in range(kept):
            at = rng.choice(red, size=min(red, 2), replace=False)
            A2[k, at] *= 2 * rng.integers(lo // 2, hi // 2 + 1, size=len(at)) + 1
    _place_tie(case, draw, A2, out["C"])
    out["A"] = ew._from_lines(case, A2)
    return out


def tie_target(dtype, draw):
    """an odd integer of [R, 2R), where the type keeps even integers: an exact tie.  Draw 0: = 1 mod 4, round-to-even goes towards zero
    (round-half-away and, the value being positive, round-half-up differ); draw 1: = 3 mod 4, it goes away from zero (truncation differs)"""
    return {"bfloat16": (289, 323), "float16": (2209, 2303)}[dtype][draw % 2]


def _place_tie(case, draw, A2, C):
    """Reduced line 0 is rebuilt so that one run of the case gives exactly tie_target() there: the smallest cases (a reduction to a
    scalar has ONE output) then hold a tie of each direction over their two draws, whatever the seeds give elsewhere.
    ADD: the run with beta != 0; the line alternates +1, -1, its first entry e and c (made odd) solve alpha * sum + beta * c = t.
    MUL: the run with beta = 0; all +1 and two odd factors with |alpha| f1 f2 = |alpha| t, the sign that of alpha."""
    kept, red = A2.shape
    t = tie_target(case.dtype, draw)
    R = rd.RANGE[case.dtype]
    if case.op == "MUL":
        (alpha, _), _ = next(r for r in case.runs if r[0][1] == 0.0)
        if red < 2:
            return
        f1 = MUL_FACTORS[case.dtype][0]
        f2 = t // f1
        assert f1 * f2 == t, (case.id, t)
        A2[0, :] = 1
        A2[0, 0], A2[0, 1] = f1 * int(np.sign(alpha)), f2
        return
    (alpha, beta), _ = next(r for r in case.runs if r[0][1] != 0.0)
    line = np.where(np.arange(red) % 2 == 0, 1, -1)
    rest = int(line[1:].sum())
    cflat = C.reshape(-1, order="F") if C.ndim else C.reshape(1)
    for c in [int(cflat[0]) | 1] + list(range(1, R, 2)):               # odd c: alpha e = t - beta c - alpha rest
        e = (t - beta * c) / alpha - rest
        if abs(c) <= R and e == round(e) and e != 0 and abs(e) <= R:
            line[0] = int(e)
            A2[0, :] = line
            C[(0,) * C.ndim] = c
            return
    raise AssertionError("%s: no tie placed" % case.id)


def check_draw(case, ins, run, d):
    """the data conditions of one run, asserted before anything is launched: integers, and an fp32 computation that stays exact"""
    assert all(np.issubdtype(x.dtype, np.integer) for x in ins.values()), case.id
    scal, _ = run
    assert all(float(s) == round(float(s)) for s in scal), (case.id, scal)
    if case.kind == "reduction" and case.op == "ADD":
        return ew.check_draw(case, ins, run, d)
    if case.kind == "reduction":
        _, red = ew._red_axes(case)
        a = np.abs(ins["A"])
        assert bool((a % 2 == 1).all()) and int((a > 1).sum(axis=tuple(red)).max()) <= 2 and int(a.max()) <= MUL_FACTORS[case.dtype][1], case.id
        bound = abs(scal[0]) * float(MUL_FACTORS[case.dtype][1]) ** 2 + abs(scal[1]) * float(np.abs(ins["C"]).max())
    else:                   # every intermediate of alpha a (op) beta b (op) gamma c is an integer no larger than this
        m = [abs(s) * float(np.abs(ins[t]).max()) for s, t in zip(scal, ew.TENSORS[case.kind][:-1])]
        bound = 0.0
        for o, v in zip(("ADD",) + _ops(case), m):
            bound = bound + v if o == "ADD" else bound * max(v, 1.0)
    assert bound < 2.0 ** 24, "%s: bound %g is not below 2^24" % (case.id, bound)
    return bound / 2.0 ** 24


def expected(case, ref):
    """the exact result rounded once to the data type; the share that rounds is asserted on the reference and the counts are kept"""
    r = torch.from_numpy(np.ascontiguousarray(ref).reshape(np.shape(ref)))
    assert bool((r == r.round()).all()) and float(r.abs().max()) < 2.0 ** 24, case.id
    want = xd.round_to(r, case.dtype)
    c = rd.counts(r.numpy(), want.numpy(), case.dtype)
    rd.check_share(case.id, c[0], c[1], c[2], MIN_ROUNDING)
    STATS.append(("elementwise", case.dtype, case.id, c))
    return want


def run_case(ct, ops, h, case):
    table = mm if case in MM else ew
    return table.run_case(ct, ops, h, case, make=make_draw, check=check_draw, expect=expected, runs=runs(case))
