"""The compiled complex trinary kernels (build/obj/elementwise_trinary_cplx.o, no GPU needed): the object holds the new kernels and nothing
else — per data type the transposing kernel with E and with E plus a second tile X, the row copy with E and the element-gather kernel.
None may use scratch memory or spill vector registers (the rows of C, E and X a lane requests before it uses the first one live in
registers), each stays within 128 VGPRs (four waves per SIMD), and the static LDS stays within the footprint of the real two-tile form,
2 x 64 x (128 + 4) x 4 = 67584 bytes: one tile of T1 x (T0 + NV) elements is 33280 bytes on both types without X; with X complex128 keeps
that tile twice (66560) and complex64 takes two 64 x 64 tiles of 64 x (64 + 2) x 8 bytes: 67584, the real form's footprint exactly."""
from test_kernel_resources import _code_object, _kernel_notes

REAL_TWO_TILES = 2 * 64 * (128 + 4) * 4


def test_complex_trinary_kernels_use_no_scratch_and_fit_registers_and_lds(built, tmp_path):
    k = _kernel_notes(_code_object(tmp_path, "elementwise_trinary_cplx"))
    mine = {n: v for n, v in k.items() if "ew3c_" in n and "Ew3CplxParams" in n}
    assert mine and len(mine) == len(k), sorted(set(k) - set(mine))             # the object holds nothing else
    by = {f: {n: v for n, v in mine.items() if f in n} for f in ("ew3c_transpose_kernel", "ew3c_rowcopy_kernel", "ew3c_generic_kernel")}
    # complex64 and complex128: the transposing kernel with and without X, one row copy, one gather kernel
    assert {f: len(v) for f, v in by.items()} == {"ew3c_transpose_kernel": 4, "ew3c_rowcopy_kernel": 2, "ew3c_generic_kernel": 2}, sorted(mine)
    bad = {n: v for n, v in mine.items() if v.get("private_segment_fixed_size", 0) or v.get("vgpr_spill_count", 0)}
    assert not bad, bad
    assert all(v.get("vgpr_count", 999) + v.get("agpr_count", 0) <= 128 for v in mine.values()), mine
    assert all(v.get("group_segment_fixed_size", 0) == 0 for f in ("ew3c_rowcopy_kernel", "ew3c_generic_kernel") for v in by[f].values())
    one_tile = 32 * (128 + 2) * 8                              # without X: 128 x 32 complex64, 64 x 32 complex128
    assert one_tile == 32 * (64 + 1) * 16
    two_c64, two_c128 = 2 * 64 * (64 + 2) * 8, 2 * one_tile    # with X: 64 x 64 complex64 (tile0 halved), 64 x 32 complex128
    assert two_c128 <= two_c64 == REAL_TWO_TILES
    sizes = sorted(v.get("group_segment_fixed_size") for v in by["ew3c_transpose_kernel"].values())
    # (the form without X may keep NV elements of the second tile's symbol: 16 bytes)
    assert sizes[:2] == [one_tile + 16] * 2 or sizes[:2] == [one_tile] * 2, sizes
    assert sizes[2:] == [two_c128, two_c64], sizes
