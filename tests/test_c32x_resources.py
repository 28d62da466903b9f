"""The compiled reduced-precision complex64 kernels (build/obj/gett_gen_c32x.o, no GPU needed).  gett_gen_c32x_kernel is compiled with
__launch_bounds__(256, 1) for the 128 x 128 tiles (128 accumulator registers: 16 fragments x (re, im); 512 registers per lane, one
workgroup per CU) and with __launch_bounds__(256, 2) for the 64 x 64 ones (256 registers, two workgroups per CU).  No instantiation may
spill (a private segment at every dispatch), the static LDS is two stages of (re, im) x planes 16-bit images per operand — 64 KiB for the
128 x 128 x 32 tile under 16BF / 16F, 128 KiB under TF32 — and the workgroups that share a CU must fit its 160 KiB."""
import re

from test_kernel_resources import _code_object, _kernel_notes


def _cfg(name):
    """(elem, bm, bn, bk, oa, ob, v) from the mangled C32xCfg<...> template arguments: Li<n>E"""
    m = re.search(r"C32xCfg((?:ILi\d+E|Li\d+E)+)", name)
    return tuple(int(x) for x in re.findall(r"Li(\d+)E", m.group(1))) if m else None


def test_reduced_precision_complex64_kernels_use_no_scratch_and_fit_the_lds(built, tmp_path):
    k = _kernel_notes(_code_object(tmp_path, "gett_gen_c32x"))
    hot = {n: v for n, v in k.items() if "gett_gen_c32x_kernel" in n}
    assert len(hot) == 48, sorted(k)                                  # 3 modes x (2 tiles x 2 widths) x 4 orientation pairs
    bad = {n: v for n, v in hot.items() if v.get("private_segment_fixed_size", 0) or v.get("vgpr_spill_count", 0)}
    assert not bad, bad                                               # (scalar registers holding GettParams spill into vector lanes, as in gett_gen_kernel: no memory)
    seen = set()
    for n, v in hot.items():
        cfg = _cfg(n)
        assert cfg is not None and len(cfg) == 7, n
        elem, bm, bn, bk, _, _, vec = cfg
        assert elem in (10, 11, 12) and (bm, bn) in ((128, 128), (64, 64)) and vec in (1, 2), n
        seen.add((elem, bm, vec))
        wgs = 2 if bm * bn <= 64 * 64 else 1                          # workgroups per CU of the launch bound
        assert v.get("vgpr_count", 999) + v.get("agpr_count", 0) <= 512 // wgs, (n, v)
        images = 4 if elem == 12 else 2                               # (re, im) x planes
        want = 2 * images * (bm + bn) * bk * 2                        # two stages x images x (A rows + B rows) x BK x 2 bytes
        assert v.get("group_segment_fixed_size") == want, (n, v, want)
        assert wgs * want <= 160 * 1024, (n, want)
    assert len(seen) == 12, sorted(seen)
