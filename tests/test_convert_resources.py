"""The compiled converting element-wise kernels (build/obj/elementwise_convert.o, no GPU needed): no kernel of elementwise_convert.hip
may use scratch memory (a private segment at every dispatch would put the 8 x 8 register transposes of the transposing kernels in memory),
and the transposing kernels' static LDS tile stays within 32 KiB, five workgroups per CU.  Per pair of data types the object holds the row
copy, the element-gather kernel and the transposing kernel at each tile width its parked type admits, each with and without the C term
and with and without the unary operators."""
from test_kernel_resources import _code_object, _kernel_notes


def test_converting_kernels_use_no_scratch_and_fit_the_lds(built, tmp_path):
    k = _kernel_notes(_code_object(tmp_path, "elementwise_convert"))
    mine = {n: v for n, v in k.items() if "convert_kernel" in n}
    assert mine and len(mine) == len(k), sorted(set(k) - set(mine))             # the object holds nothing else
    by = {f: {n: v for n, v in mine.items() if f in n} for f in ("ew_rowcopy_convert_kernel", "ew_transpose_convert_kernel", "ew_generic_convert_kernel")}
    # 6 pairs x {C, no C} x {identity, operators}; the transposing kernel at 3 + 3 + 3 + 3 + 2 + 2 tile widths without C (the narrower type
    # parked) and 3 + 3 + 2 + 2 + 2 + 1 with C (A's type parked), each twice
    assert len(by["ew_rowcopy_convert_kernel"]) == 24 and len(by["ew_generic_convert_kernel"]) == 24, {f: len(v) for f, v in by.items()}
    assert len(by["ew_transpose_convert_kernel"]) == 2 * (16 + 13), len(by["ew_transpose_convert_kernel"])
    bad = {n: v for n, v in mine.items() if v.get("private_segment_fixed_size", 0) or v.get("vgpr_spill_count", 0)}
    assert not bad, bad                                               # (scalar registers holding Ew2DParams may spill into vector lanes: no memory)
    assert all(v.get("group_segment_fixed_size", 0) == 0 for f in ("ew_rowcopy_convert_kernel", "ew_generic_convert_kernel") for v in by[f].values())
    sizes = {v.get("group_segment_fixed_size") for v in by["ew_transpose_convert_kernel"].values()}
    assert sizes <= {8192, 16384, 32768}, sizes
    assert all(v.get("vgpr_count", 999) + v.get("agpr_count", 0) <= 128 for v in mine.values()), mine      # at least four waves per SIMD
