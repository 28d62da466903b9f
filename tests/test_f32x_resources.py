"""The compiled reduced-precision fp32 kernels (build/obj/gett_gen_f32x.o, no GPU needed): gett_gen_f32x_kernel is compiled with
__launch_bounds__(256, 2) — 256 registers per lane, two workgroups per CU.  The TF32 128 x 128 x 32 tile (64 accumulator + 64
fragment + 32 staging registers + the conversion's temporaries) is the tight one.  No instantiation may spill (a private segment at every
dispatch), and the static LDS must stay within what two workgroups per CU can share (160 KiB): 64 KiB for the 128 x 128 tiles — one
16-bit image per operand at BK = 64, two (hi, lo) at BK = 32 — and less for the 64 x 64 ones."""
import re

from test_kernel_resources import _code_object, _kernel_notes


def _cfg(name):
    """(elem, bm, bn, bk, oa, ob, v) from the mangled F32xCfg<...> template arguments: Li<n>E"""
    m = re.search(r"F32xCfg((?:ILi\d+E|Li\d+E)+)", name)
    return tuple(int(x) for x in re.findall(r"Li(\d+)E", m.group(1))) if m else None


def test_reduced_precision_fp32_kernels_use_no_scratch_and_fit_the_lds(built, tmp_path):
    k = _kernel_notes(_code_object(tmp_path, "gett_gen_f32x"))
    hot = {n: v for n, v in k.items() if "gett_gen_f32x_kernel" in n}
    assert len(hot) == 48, sorted(k)                                  # 3 modes x (2 tiles x 2 widths) x 4 orientation pairs
    bad = {n: v for n, v in hot.items() if v.get("private_segment_fixed_size", 0) or v.get("vgpr_spill_count", 0)}
    assert not bad, bad                                               # (scalar registers holding GettParams spill into vector lanes, as in gett_gen_kernel: no memory)
    assert all(v.get("vgpr_count", 999) + v.get("agpr_count", 0) <= 256 for v in hot.values()), hot      # two workgroups per CU
    for n, v in hot.items():
        cfg = _cfg(n)
        assert cfg is not None and len(cfg) == 7, n
        elem, bm, bn, bk, _, _, vec = cfg
        planes = 2 if elem == 7 else 1
        want = 2 * planes * (bm + bn) * bk * 2                        # two stages x planes x (A rows + B rows) x BK x 2 bytes
        assert v.get("group_segment_fixed_size") == want and want <= 65536, (n, v, want)
        assert 2 * want <= 160 * 1024
