"""Every contraction path bit for bit on integer-valued data (tests/exact_data.py; the case table is tests/exact_cases.py).

The other contraction tests draw U(0,1) or U(-1,1) data and compare with an fp64 reference under a tolerance that has to cover
legitimate round-off — and with it one contracted element dropped or taken twice (the headline test accepts about 26 missing products
per output).  On data whose products and partial sums are exactly representable in the accumulator every correct kernel returns exactly
the integer answer, whatever its tile order, split-K factor or fold: the comparison here has no tolerance, and a non-zero `got - expected`
is the sum of the products that were lost or doubled.

Every case names its path with a predicate on the plan's description, runs on two draws (the dense operand on either side), with D in a
NaN-filled buffer.  Switches that the library reads once per process are set in a child per switch value, one after the other, each with
its own time limit.

16-bit outputs: the exact value is rounded once to the data type (at most 1 % of a case's outputs leave the type's exact integer range;
those are compared with the single round-to-nearest-even of the exact value).  A result that differs there would be a second rounding:
the one place where the library rounds twice by design is the lone-mode reduction of 16-bit data into a 16-bit temporary (contraction_route.cpp,
split_lone_modes) — bf16_lone_small_sums keeps those sums in the exact range, bf16_lone_rounded_sums takes them to about
600 and asserts the result of rounding them first."""
import pytest

import exact_cases as xc
import exact_data as xd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(built):
    import torch
    assert torch.cuda.is_available()
    from cudalibrarysamples_amd import cutensor as ct, ops
    return ct, ops, ops.Handle(), torch


@pytest.mark.parametrize("cid", xc.IN_PROCESS)
def test_exact(env, cid):
    ct, ops, h, torch = env
    xc.run_case(ct, ops, h, xc.BY_ID[cid])


@pytest.mark.parametrize("cid", [c.id for c in xc.CASES if c.full_size and c.group is None])
def test_exact_full_size(env, cid):
    """the headline (split-K 256 + fold), contraction.cu's default extents and 8192^3 bf16 by the planner's choice: EVERY output against
    the device's fp64 einsum (exact on this data), 4096 sampled outputs of that against int64 dot products"""
    ct, ops, h, torch = env
    xc._DATA.clear()
    torch.cuda.empty_cache()
    xc.run_case(ct, ops, h, xc.BY_ID[cid])
    xc._DATA.clear()
    torch.cuda.empty_cache()


TIMEOUTS = {"fused_fold": 600, "korder": 600}


@pytest.mark.parametrize("group", xc.GROUPS)
def test_exact_under_a_switch(env, group):
    """the cases of one switch value in a fresh child (H16_WAVES = 4x .. 4q: every forced 16-bit kernel on four layouts x aligned, ragged K,
    sweep-ragged, no 16-byte lanes; the persistent kernel on a grid of 8; GEN = force / 0; PEEL = 0; REPACK = f; the in-launch fold)"""
    ct, ops, h, torch = env
    xc._DATA.clear()
    cases = [c for c in xc.CASES if c.group == group]
    xc.in_child([c.id for c in cases], cases[0].env, timeout=TIMEOUTS.get(group, 900))


def test_exact_every_candidate_kernel_and_split(env):
    """Every ranked (kernel, split-K) candidate of the ten problems of test_gpu_contraction.py::test_every_candidate_kernel_and_split,
    alpha = -2, beta = 1, and the nontemporal twins in a child with CUTENSOR_AMD_NT=1: no kernel index is left out."""
    ct, ops, h, torch = env
    seen, _, split = xc.sweep(ct, ops, h, xc.SWEEP_PROBLEMS, "sweep")
    assert split
    planned = {i for i in range(ct.lib.ctamdKernelCount()) if not ct.lib.ctamdKernelIsAblation(i)}
    missing = planned - seen
    out = xc.in_child([], {"CUTENSOR_AMD_NT": "1"}, timeout=600, mode="nt_sweep")
    nt_seen = set(eval(out.split("KERNELS", 1)[1].splitlines()[0].strip()))
    missing -= nt_seen
    assert not missing, "GETT kernels never exercised: %s" % sorted(missing)


def test_exact_f32_candidates_off_the_lanes_and_on_the_row_epilogue(env):
    """The planner's first ten candidates on operands without 16-byte lanes at a 12-byte-aligned base (the RAG twins of the ring kernel must
    be among them), and its first eight on a 16-byte-aligned base with flat outputs (the row epilogue, ring and register-staged kernels)."""
    ct, ops, h, torch = env
    _, names, _ = xc.sweep(ct, ops, h, xc.UNALIGNED_SWEEP, "unal_sweep", ranks=10, off=3, align=4)
    assert "gett_f32_stream_kernel" in names, names
    _, names, _ = xc.sweep(ct, ops, h, xc.ROWS_SWEEP, "rows_sweep", ranks=8, off=4, align=16)
    assert {"gett_f32_stream_kernel", "gett_f32_kernel"} <= names, names


def test_exact_on_the_production_libraries(env):
    """the cases that need no switch once more on lib/ (the suite loads lib_hooks/), as test_workspace_contract_on_the_production_libraries"""
    xc._DATA.clear()
    xc.in_child(xc.NO_SWITCH, {"CTAMD_LIB_FLAVOUR": "production"}, timeout=900, mode="production")


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("gather", [False, True])
def test_exact_cutensormg_on_one_device(env, monkeypatch, dtype, gather):
    """cuTENSORMg on one device, 512^3: plain, and with CUTENSORMG_AMD_FORCE_GATHER=1 (the staged operands are what is contracted)"""
    ct, ops, h, torch = env
    from cudalibrarysamples_amd import cutensormg as cm
    if gather:
        monkeypatch.setenv("CUTENSORMG_AMD_FORCE_GATHER", "1")
    E = 512
    case = xc.Case("mg_%s" % dtype, dtype, dict(i=E, j=E, k=E), ("ik", "kj", "ij"), alpha=1.0, beta=1.0)
    for swap in (False, True):
        A, B, C = xd.make_exact(case, swap)
        xd.check_draw(case, A, B, C, swap)
        want, _ = xd.expected(case, xd.exact_reference(case, A, B, C))
        with cm.Contraction([0], list(case.modes), case.ext, [dict(), dict(), dict()], [dict(), dict(), dict()], dtype=xc._dt(ct, dtype)) as con:
            d = con.describe()
            assert d.get("forceGather", 0) == int(gather), d
            import guarded as gd
            dev = [gd.packed_device(x) for x in (A, B, C)]
            ws = [torch.full((max(int(con.ws_sizes[0]), 16),), 0xFF, dtype=torch.uint8, device="cuda")]
            stream = torch.cuda.Stream()
            torch.cuda.synchronize()
            cm.check(con.run(case.alpha, [dev[0].data_ptr()], [dev[1].data_ptr()], case.beta, [dev[2].data_ptr()], [dev[2].data_ptr()],
                             [ws[0].data_ptr()], [stream.cuda_stream]))
            stream.synchronize()
            got = dev[2].cpu().t()                       # packed column-major [i, j] = the transpose of the row-major view
            xd.assert_exact(got, want, "%s gather=%d draw %d" % (case.id, gather, swap))


def test_every_family_of_the_table_has_a_case():
    """the rows of the issue's table -> at least one case each (the predicates themselves are asserted where the cases run)"""
    ids = " ".join(c.id for c in xc.CASES)
    for needle in ("f32_headline_full", "fused_fold", "korder", "f32_sample_full", "f32_unal_", "f32_4098_", "f32_rows_", "f32_short_k_batch", "mode_table",
                   "_peeled", "peel_off", "gen_off_simple", "h16_4x_", "h16_4p_", "h16_4m_", "h16_4m4_", "h16_8m_", "h16_4q_", "h16p_grid8", "h16_splitk1",
                   "h16_splitk3", "h16_splitk8", "bf16_4100_", "bf16_8192_full", "gen_forced", "gen_conjA", "gen_conjB", "gen_conjC", "gen_odd_splitk",
                   "f16_gen_reference_equation", "_repack", "lone_small_sums", "lone_rounded_sums", "f32_lone_AB", "f32_trinary_contraction", "f64_blocksparse"):
        assert needle in ids, needle
    assert len(xc.NO_SWITCH) > 50


def test_bounds_reached():
    """what the runs of this session reached, per data type (printed: pytest -s): the largest K, the largest accumulator bound as a fraction
    of its limit (2^24 / 2^53, halved where alpha or beta is a half) and the largest share of outputs outside the output type's exact range"""
    rep = xc.report(xc.STATS)
    for dt, (n, k, frac, share) in sorted(rep.items()):
        print("exact data, %-10s: %4d runs, largest K %7d, accumulator bound %.4f of its limit, outputs that round %.3f %%" % (dt, n, k, frac, 100 * share))
        assert frac < 1.0 and share <= (xd.MAX_UNREPRESENTABLE if dt in xd.H16 else 0.0), (dt, frac, share)
