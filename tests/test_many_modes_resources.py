"""Resources of the mode-table kernels (kernels/elementwise_table.hip), read from the code object's metadata: the table travels by value
in the kernel arguments and is indexed at run time — read through the argument pointer, so that no kernel gets a private segment (a
scratch allocation is paid for at every dispatch) — the tile kernel's LDS is what the planner states in the plan's description, and
every kernel stays within 128 registers a lane (four workgroups of 256 threads on a CU).  No GPU."""
import re

import pytest

import many_mode_cases as mm
from test_kernel_resources import _code_object, _kernel_notes

SIZES = {"float32": 4, "float64": 8, "bfloat16": 2, "float16": 2, "complex64": 8, "complex128": 16}
TRAITS = {"float32": "WF32IfE", "float64": "WF64E", "bfloat16": "WH16ILb1E", "float16": "WH16ILb0E", "complex64": "WCplxIfE", "complex128": "WCplxIdE"}


@pytest.fixture(scope="module")
def notes(built, tmp_path_factory):
    return _kernel_notes(_code_object(tmp_path_factory.mktemp("ewt_obj"), "elementwise_table"))


def test_no_private_segment_no_spills_and_at_most_128_registers(notes):
    kinds = {}
    for name, v in notes.items():
        kind = re.search(r"(ew_table_tile_kernel|ew_table_gather_kernel|reduce_table_kernel|reduce_table_finalize_kernel)", name)
        assert kind, name
        kinds[kind.group(1)] = kinds.get(kind.group(1), 0) + 1
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (name, v)
        assert v["vgpr_count"] + v["agpr_count"] <= 128, (name, v)
    # six data types, the four real ones twice (the operator twins); reductions also fp32 data accumulated in fp64
    assert kinds == {"ew_table_tile_kernel": 10, "ew_table_gather_kernel": 10, "reduce_table_kernel": 12, "reduce_table_finalize_kernel": 12}, kinds


@pytest.mark.parametrize("dtype", sorted(SIZES))
def test_the_tile_kernel_declares_the_lds_the_planner_states(built, notes, dtype):
    from cudalibrarysamples_amd import cutensor as ct, ops
    case = next(c for c in mm.CASES if c.dtype == dtype and c.kind == "permutation" and c.id.endswith("perm_rev12"))
    d = mm.plan_path(ct, ops, ops.Handle(), case)
    assert d["kname"] == "ew_table_tile_kernel" and 0 < d["lds"] <= 16384 and d["tile"][0] * SIZES[dtype] <= d["lds"], d
    mine = {n: v for n, v in notes.items() if "ew_table_tile_kernel" in n and TRAITS[dtype] in n}
    assert len(mine) == (1 if dtype.startswith("complex") else 2), sorted(mine)
    for name, v in mine.items():
        assert v["group_segment_fixed_size"] == d["lds"], (name, v, d)
