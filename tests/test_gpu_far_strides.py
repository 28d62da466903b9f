"""Every kernel family's addressing on far-strided tensors (the arena, the placement and the case table are tests/far_cases.py; tests/
test_far_planner_cpu.py checks the table on the CPU planner, tests/test_far_arena_cpu.py the arena itself): small extents, one pitch
inflated until the tensor's byte span (or, for the 16-bit LDS-DMA family, the span of one tile) lies next to 2^31 or 2^32.

Per launch: the path from the plan's description, the result bit for bit on integer-valued data (two draws), every near tensor's
surroundings untouched (exact_cases.Placed.check_outside), the far tensor's elements re-poisoned and then the WHOLE 12.8-GiB arena still
0xFF, near and far inputs unchanged.  An offset truncated to 32 bits, sign-extended from them or off by 2^31 / 2^32 lands inside the arena
by its construction and fails one of these; it does not leave the allocation.

The module needs 20 GiB of free device memory and skips, loudly, without it: a run with that skip verifies nothing of this."""
import json

import pytest

import exact_cases as xc
import far_cases as fc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(built):
    import torch
    assert torch.cuda.is_available()
    if not fc.free_memory_ok():
        pytest.skip("FAR-STRIDE TESTS NOT RUN: less than 20 GiB of device memory free (%d MiB)" % (torch.cuda.mem_get_info()[0] >> 20))
    from cudalibrarysamples_amd import cutensor as ct, ops
    arena = fc.Arena()
    yield ct, ops, ops.Handle(), arena
    del arena
    torch.cuda.empty_cache()


@pytest.mark.parametrize("cid", fc.IN_PROCESS)
def test_far_contraction(env, cid):
    ct, ops, h, arena = env
    fc.run_case(ct, ops, h, fc.BY_ID[cid], arena)


@pytest.mark.parametrize("cid", [c.id for c in fc.EW_CASES])
def test_far_elementwise_and_reduction(env, cid):
    ct, ops, h, arena = env
    fc.run_ew_case(ct, ops, h, fc.EW_BY_ID[cid], arena)


@pytest.mark.parametrize("group", fc.GROUPS)
def test_far_contraction_in_a_child(env, group):
    """the cases whose switch the library reads once per process: one child at a time, each with an arena of its own"""
    cases = [c for c in fc.CASES if c.group == group]
    out = xc.in_child([c.id for c in cases], cases[0].env, 300, script="far_cases.py")
    fc.LAUNCHES.extend(tuple(x) for x in json.loads(out.split("LAUNCHES ", 1)[1].splitlines()[0]))


def test_every_section_launched_the_kernels_it_is_named_after(env):
    """the launches of this session per section of the table and kernel (printed: run with -s): every section of far_cases.SECTIONS saw
    every kernel, split-K fold and variant it names — a section that ran nothing fails here, so this test passes only in a run of the
    whole module"""
    print("\nfar-stride launches:", json.dumps(fc.summary(fc.LAUNCHES), sort_keys=True))
    missing = fc.missing_launches(fc.LAUNCHES)
    assert not missing, "no launch of these (section, kernel) pairs in this session — this test passes only in a run of the WHOLE module, not under -k " \
                        "or after a single-test rerun: %s" % missing
