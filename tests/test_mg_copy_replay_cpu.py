"""The launches of cutensorMgCopy EXECUTED on the CPU: ctamdMgCopyReplayOnHost (csrc/mg/mg_copy.cpp) walks a plan's launch tables over
host cell buffers and runs every kernel thread by thread through the bodies of csrc/mg/mg_redistribute_layout.h — the same cells,
forms, lane widths, runs and tiles the device executes — so a bug of the decomposition shows without a GPU.  Every case of
tests/mg_copy_cases.py on plan-only handles with 1, 2, 4 and 8 distinct device ids, and 50 seeded random layouts, against the
NumPy reference with the poison checks (bit for bit; nothing outside the valid elements written; no source padding read)."""
import pytest

from tests import mg_copy_cases as mc

HANDLES = [1, 2, 4, 8]


@pytest.fixture(scope="module")
def cm(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("plan-only handles for device ids 0..7 need a host without that many GPUs")
    from cudalibrarysamples_amd import cutensormg
    return cutensormg


@pytest.mark.parametrize("n", HANDLES)
@pytest.mark.parametrize("case,dtype", mc.RUNS, ids=mc.RUN_IDS)
def test_replay_of_every_case_is_exact(cm, case, dtype, n):
    d = mc.run_on_host(cm, list(range(n)), case, dtype, seed=n)
    assert case.expect(d, dtype), d


@pytest.mark.parametrize("first,second", mc.ROUND_TRIPS)
def test_scatter_then_gather_gives_back_the_input_bits(cm, first, second):
    a, b = mc.BY_ID[first], mc.BY_ID[second]
    S, D, W = mc.make_data(a.src, a.dst, "fp32", 7)
    with cm.CopyPlan([0, 1, 2, 3], a.dst.layout(), a.src.layout()) as p:
        assert p.replay_on_host([x.ctypes.data for x in D], [x.ctypes.data for x in S]) == 0
    mc.check(D, W, "fp32", first)
    back = mc.aligned_cells(b.dst.cells, b.dst.span, S[0].dtype, mc.DST_POISON)
    with cm.CopyPlan([0, 1, 2, 3], b.dst.layout(), b.src.layout()) as p:
        assert p.replay_on_host([x.ctypes.data for x in back], [x.ctypes.data for x in D]) == 0
    assert len(back) == 1 and (back[0] == S[0]).all()


def test_fuzz_draws_stay_within_the_refusal_cap(cm):
    """the NumPy side alone: none of the 50 draws breaks a descriptor rule (distinct labels, equal extents, at most 16 modes, default
    owners) — the refused share is 0 %, the cap is 20 %"""
    refused = 0
    for seed in range(mc.FUZZ_DRAWS):
        src, dst, dtype = mc.fuzz_draw(seed)
        ok = (sorted(src.modes) == sorted(dst.modes) and len(set(src.modes)) == len(src.modes) <= 16 and
              all(src.ext[src.modes.index(c)] == dst.ext[dst.modes.index(c)] for c in src.modes) and dtype in mc.DTYPES)
        refused += not ok
    assert refused == 0 and refused <= 0.2 * mc.FUZZ_DRAWS


@pytest.mark.parametrize("seed", range(mc.FUZZ_DRAWS))
def test_replay_of_random_layouts_is_exact(cm, seed):
    src, dst, dtype = mc.fuzz_draw(seed)
    d = mc.run_on_host(cm, list(range([1, 2, 4, 8][seed % 4])), None, dtype, seed=seed, src=src, dst=dst)
    assert mc.launches(d)
