"""The final rounding of every 16-bit output, bit for bit (data, rules and comparators: tests/rounding_data.py; the cases:
tests/rounding_cases.py and tests/rounding_ew.py; tests/test_round16_data_cpu.py proves on the CPU that the data tells a wrong rounding
from the right one).

Every kernel that writes bf16 or fp16 ends with rnd16(alpha * acc + beta * c).  The exact suites keep that step trivial on purpose (their
sums are values of the type) and the tolerance tests allow 2 ulp, so truncation, round-half-away, round-half-up or a second rounding —
1 ulp each — pass both.  Here the accumulator is still exact and most results are NOT values of the type: the comparison with the exact
reference rounded once has no tolerance.

  * test_round16_contraction / _under_a_switch / _cutensormg: every 16-bit case of tests/exact_cases.py below 1e9 multiply-adds on its own
    path (forced LDS-DMA variants, persistent kernel, forced and planned split-K, general family, gett_simple, repack, cuTENSORMg).
  * test_round16_beta_*: beta = 2^-14 below fp32's last place, where one rounding and two give different bits: fp16 rounds the fused
    multiply-add once, bf16 rounds an fp32 fused multiply-add — on every path that has beta arithmetic of its own.
  * test_round16_elementwise / _many_modes: cutensorPermute, the binary and trinary forms and cutensorReduce.
  * test_round16_statistics: runs, the smallest share of rounding outputs and the exact ties seen per data type (printed: pytest -s)."""
import pytest

import exact_cases as xc
import exact_data as xd
import rounding_cases as rc
import rounding_data as rd
import rounding_ew as rw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(built):
    import torch
    assert torch.cuda.is_available()
    from cudalibrarysamples_amd import cutensor as ct, ops
    return ct, ops, ops.Handle(), torch


@pytest.mark.parametrize("cid", rc.ROUNDING_IN_PROCESS)
def test_round16_contraction(env, cid):
    ct, ops, h, torch = env
    rc.run_rounding(ct, ops, h, xc.BY_ID[cid])


@pytest.mark.parametrize("group", rc.ROUNDING_GROUPS)
def test_round16_contraction_under_a_switch(env, group):
    """the 16-bit cases of one switch value in a fresh child, as tests/test_gpu_exact.py::test_exact_under_a_switch runs them"""
    xc._DATA.clear()
    cases = [c for c in rc.ROUNDING if c.group == group]
    rc.in_child([c.id for c in cases], cases[0].env, timeout=900, mode="run")


@pytest.mark.parametrize("group", rc.BETA_GROUPS)
def test_round16_beta_below_the_last_place_of_fp32(env, group):
    """the pipelined chunk path and the element-wise epilogue of the LDS-DMA kernels (h16_4x_one_slice), flush()'s chunk form
    (h16_4m_one_slice), the persistent kernel (h16p_grid8), both split-K folds (h16_splitk8), the general family's epilogue (gen_force),
    gett_simple (gen0) and the mode-table kernel (in this process); tests/rounding_cases.py derives each case's path"""
    ct, ops, h, torch = env
    xc._DATA.clear()
    cases = [c for c in rc.BETA if (c.group or "in_process") == group]
    if group == "in_process":
        for c in cases:
            rc.run_beta(ct, ops, h, c)
    else:
        rc.in_child([c.id for c in cases], cases[0].env, timeout=900, mode="beta")


@pytest.mark.parametrize("gather", [False, True])
def test_round16_cutensormg_on_one_device(env, monkeypatch, gather):
    """tests/test_gpu_exact.py::test_exact_cutensormg_on_one_device (bf16, 512^3, beta = 1) in the rounding regime"""
    ct, ops, h, torch = env
    from cudalibrarysamples_amd import cutensormg as cm
    import guarded as gd
    if gather:
        monkeypatch.setenv("CUTENSORMG_AMD_FORCE_GATHER", "1")
    case = xc.Case("mg_bfloat16", "bfloat16", dict(i=512, j=512, k=512), ("ik", "kj", "ij"), alpha=1.0, beta=1.0)
    for swap in (False, True):
        A, B, C = rd.make_rounding(case, swap)
        xd.check_draw(case, A, B, C, swap)
        want, counts = rd.expected_rounded(case, xd.exact_reference(case, A, B, C))
        with cm.Contraction([0], list(case.modes), case.ext, [dict(), dict(), dict()], [dict(), dict(), dict()], dtype=xc._dt(ct, case.dtype)) as con:
            d = con.describe()
            assert d.get("forceGather", 0) == int(gather), d
            dev = [gd.packed_device(x) for x in (A, B, C)]
            ws = [torch.full((max(int(con.ws_sizes[0]), 16),), 0xFF, dtype=torch.uint8, device="cuda")]
            stream = torch.cuda.Stream()
            torch.cuda.synchronize()
            cm.check(con.run(case.alpha, [dev[0].data_ptr()], [dev[1].data_ptr()], case.beta, [dev[2].data_ptr()], [dev[2].data_ptr()],
                             [ws[0].data_ptr()], [stream.cuda_stream]))
            stream.synchronize()
            xd.assert_exact(dev[2].cpu().t(), want, "%s gather=%d draw %d" % (case.id, gather, swap))
        rc.STATS.append(("contraction", case.dtype, case.id, counts))


@pytest.mark.parametrize("cid", [c.id for c in rw.EW])
def test_round16_elementwise(env, cid):
    ct, ops, h, torch = env
    rw.run_case(ct, ops, h, rw.BY_ID[cid])


@pytest.mark.parametrize("cid", [c.id for c in rw.MM])
def test_round16_many_modes(env, cid):
    ct, ops, h, torch = env
    rw.run_case(ct, ops, h, rw.BY_ID[cid])


def test_round16_statistics():
    """what the runs of this session saw, per part and data type (printed: pytest -s) — and over the whole module at least 1000 exact ties
    per data type of each kind (to-even-down and to-even-up, of both signs), among the contractions and among the element-wise
    results.  Counted on the references, never on a kernel's result."""
    stats = rc.STATS + rw.STATS
    ran = {p: {s[2] for s in stats if s[0] == p} for p in ("contraction", "elementwise")}
    whole = [p for p, cases in (("contraction", rc.ROUNDING), ("elementwise", rw.EW + rw.MM)) if {c.id for c in cases} <= ran[p]]
    rep = rd.check_ties(stats, parts=whole)            # (a part whose every case ran: the tie counts are its own)
    assert all((p, dt) in rep for p in whole for dt in xd.H16)
