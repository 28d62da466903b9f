"""The compiled gfx950 kernels of cutensorMgCopy (csrc/mg/mg_redistribute.hip), read from the code object inside
build/obj/mg_redistribute.o with the helpers of tests/test_kernel_resources.py (no GPU needed): no kernel has a private segment or a
spill — the argument block with its cell tables is indexed per lane and must stay in the kernel-argument segment, not be copied to
scratch — and the tile kernels' static LDS is the size the comment in mg_redistribute_layout.h states."""
from tests.test_kernel_resources import _code_object, _kernel_notes


def test_redistribution_kernels_have_no_private_segment_and_the_stated_lds(built, tmp_path):
    k = _kernel_notes(_code_object(tmp_path, "mg_redistribute"))
    rows = {n: v for n, v in k.items() if "mg_redistribute_rows_kernel" in n}
    tile = {n: v for n, v in k.items() if "mg_redistribute_tile_kernel" in n}
    gather = {n: v for n, v in k.items() if "mg_redistribute_gather_kernel" in n}
    table = {n: v for n, v in k.items() if "mg_redistribute_table_kernel" in n}
    assert (len(rows), len(tile), len(gather), len(table)) == (6, 3, 3, 1), sorted(k)     # rows: 3 element sizes x {16-byte, element} lanes
    bad = {n: v for n, v in k.items() if v.get("private_segment_fixed_size", 0) or v.get("vgpr_spill_count", 0) or v.get("sgpr_spill_count", 0)}
    assert not bad, bad
    # the tile [64][65] in 4-byte words (2- and 4-byte elements) or 8-byte words, plus the 2584 bytes of tile-edge address parts
    lds = sorted(v.get("group_segment_fixed_size") for v in tile.values())
    assert lds == [64 * 65 * 4 + 2584, 64 * 65 * 4 + 2584, 64 * 65 * 8 + 2584] == [19224, 19224, 35864], tile
    assert all(v.get("group_segment_fixed_size", 0) == 0 for n, v in k.items() if n not in tile), k
