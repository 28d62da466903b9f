"""The compiled single-precision-compute fp64 / complex128 GETT kernels (csrc/kernels/gett_gen_f64x.hip), read from the gfx950 code object
inside build/obj/gett_gen_f64x.o (no GPU needed): gett_gen_f64x_kernel is compiled with __launch_bounds__(256, 2) = 256 registers per
lane.  The tight instantiations are the 128 x 128 x 32 tile on 8-byte gathers (sixteen staged doubles per operand beside the 64
accumulator registers: it keeps 32-bit row indices where the others keep 64-bit row offsets) and the three-accumulator complex tile.  A
spill would be a scratch allocation at every dispatch: every instantiation must come out with no private segment."""
from test_kernel_resources import _code_object, _kernel_notes


def test_f64x_kernels_use_no_scratch_and_fit_two_workgroups_per_cu(built, tmp_path):
    k = _kernel_notes(_code_object(tmp_path, "gett_gen_f64x"))
    gen = {n: v for n, v in k.items() if "gett_gen_f64x_kernel" in n}
    # (4 real + 2 complex table rows) x 4 orientation pairs
    assert len(gen) == 24, sorted(k)
    # (scalar registers do overflow into lanes of a vector register, here as in every kernel of the family: GettParams is 1.5 KiB of
    # scalars; that costs no memory traffic and is inside the vector register count below)
    bad = {n: v for n, v in gen.items() if v.get("private_segment_fixed_size", 0) or v.get("vgpr_spill_count", 0)}
    assert not bad, bad
    assert all(v.get("vgpr_count", 999) <= 256 for v in gen.values()), gen
    # static LDS, two stages: 64 KiB for the real 128 x 128 x 32 tile at most — two workgroups fit the CU's 160 KiB
    assert all(v.get("group_segment_fixed_size", 1 << 30) <= 65536 for v in gen.values()), gen
    fold = {n: v for n, v in k.items() if "gen_f64x_splitk_reduce_kernel" in n}
    assert len(fold) == 2 and not any(v.get("private_segment_fixed_size", 0) for v in fold.values()), fold
