"""The compiled mixed fp64 x complex128 GETT kernels (csrc/kernels/gett_gen_rc64.hip), read from the gfx950 code object inside
build/obj/gett_gen_rc64.o (no GPU needed): gett_gen_rc64_kernel is compiled with __launch_bounds__(256, 2) = 256 registers per lane — 64
accumulator registers (two fp64x4 per fragment, four fragments per wave), 24 of fragments, at most 12 of staging.  A spill would be a
scratch allocation at every dispatch: every instantiation must come out with no private segment, and two workgroups must fit a CU."""
import os
import re

from test_kernel_resources import _code_object, _kernel_notes

KDIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cudalibrarysamples_amd", "csrc", "kernels")


def test_rc64_kernels_use_no_scratch_and_fit_two_workgroups_per_cu(built, tmp_path):
    k = _kernel_notes(_code_object(tmp_path, "gett_gen_rc64"))
    gen = {n: v for n, v in k.items() if "gett_gen_rc64_kernel" in n}
    # the table: (real side, real width) row groups x four orientation pairs — every row its own instantiation, and nothing else in the file
    groups = re.findall(r"CTAMD_GEN_RC64_ORIENTS\((\d+), (\d+)\)", open(os.path.join(KDIR, "gett_gen_rc64.hip")).read())
    assert len(set(groups)) == len(groups) == 4 and len(gen) == 4 * len(groups) == len(k), sorted(k)
    bad = {n: v for n, v in gen.items() if v.get("private_segment_fixed_size", 0) or v.get("vgpr_spill_count", 0)}
    assert not bad, bad
    assert all(v.get("vgpr_count", 999) <= 256 for v in gen.values()), gen
    # static LDS, two stages of a 64 x 8 real (4 KiB) and a 64 x 8 complex (8 KiB) tile: two workgroups fit the CU's 160 KiB many times over
    assert all(v.get("group_segment_fixed_size", 1 << 30) == 2 * (64 * 8 * 8 + 64 * 8 * 16) for v in gen.values()), gen
    assert all(2 * v["group_segment_fixed_size"] <= 160 * 1024 for v in gen.values())


def test_the_table_size_is_the_kernel_count(built):
    """16 rows behind every earlier row of the general family's table: a mixed plan of each (side, width) names a kernel index in that range"""
    from cudalibrarysamples_amd import cutensor as ct, ops
    import rc64_cases as rc
    h = ops.Handle()
    idx = set()
    for c in rc.CASES:
        if c.id.startswith(("ragged_", "vec")):
            idx.add(rc.plan_path(ct, ops, h, c).get("kernel"))
    assert len(idx) == 16 and max(idx) - min(idx) == 15, sorted(idx)
