"""The flat entries of the streaming fp32 GETT and of its fold on scalar kernel parameters, read from the code object in
build/obj/gett_f32_stream.o (no GPU needed): their kernel descriptors ask for preloaded arguments (csrc/Makefile passes
-amdgpu-kernarg-preload-count to this one translation unit; a struct passed by value gets none, so every other kernel of the unit
must show length 0), and they keep the resource limits of the flat entries — no private segment, no spills, at most 256 vector
registers per lane (two waves per SIMD) and the 72-KiB ring."""
import os
import re
import subprocess

from test_kernel_resources import LLVM, _code_object, _kernel_notes


def _preload_lengths(co):
    """{kernel symbol: .amdhsa_user_sgpr_kernarg_preload_length} from the kernel descriptors (<symbol>.kd in .rodata)"""
    out = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-D", "-j", ".rodata", co], check=True, capture_output=True, text=True).stdout
    lengths, name = {}, None
    for line in out.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)\.kd>:", line)
        if m:
            name = m.group(1)
            lengths[name] = 0          # the directive is printed only when it is not 0
            continue
        m = re.match(r"\s*\.amdhsa_user_sgpr_kernarg_preload_length\s+(\d+)", line)
        if m and name is not None:
            lengths[name] = int(m.group(1))
    return lengths


def test_scalar_parameter_entries_are_preloaded_and_stay_within_the_flat_entries_limits(built, tmp_path):
    co = _code_object(tmp_path, "gett_f32_stream")
    k = _kernel_notes(co)
    pre = _preload_lengths(co)
    assert set(pre) == set(k), sorted(set(pre) ^ set(k))
    gett = {n: v for n, v in k.items() if "gett_f32_stream_kernel" in n and n.endswith("NS_14StreamFlatTailE")}
    assert len(gett) == 8, sorted(k)          # four layouts x default / nontemporal stream
    fold = {n: v for n, v in k.items() if "splitk_fold_frag_args_kernel" in n}
    assert len(fold) == 4, sorted(k)          # 2 x 2, 3 x 3, 4 x 4 fragments per wave, and the run-time decode
    for name, v in {**gett, **fold}.items():
        assert pre[name] == 14, (name, pre[name])      # what gfx950 grants: 16 user SGPRs less the argument pointer
        assert not v.get("private_segment_fixed_size", 0) and not v.get("vgpr_spill_count", 0) and not v.get("sgpr_spill_count", 0), (name, v)
        assert v["vgpr_count"] <= 256, (name, v)
    for name, v in gett.items():
        assert "Li3ELi8E" in name or "Li3ELi9E" in name, name
        assert not name.endswith("StreamFlatParamsE") and "Li3ELi0" not in name, name
        struct = re.sub(r"EvPKfS\d+_Pyj+NS_14StreamFlatTailE$", "EvNS_16StreamFlatParamsE", name.replace("Li3ELi8E", "Li3ELi6E").replace("Li3ELi9E", "Li3ELi7E"))
        assert struct in k, (name, struct)
        assert v["group_segment_fixed_size"] == k[struct]["group_segment_fixed_size"] == 3 * 24 * 1024, (name, v)
    # the flag reaches nothing else: every kernel that takes its arguments as a struct compiles without preload
    others = {n: l for n, l in pre.items() if n not in gett and n not in fold}
    assert len(others) >= 19 + 8 + 4 and not any(others.values()), {n: l for n, l in others.items() if l}


def test_changed_flat_entries_stay_within_their_limits(built, tmp_path):
    """The struct entries run the same body (straight-line last K-tiles): the same limits, read again here for every flat entry."""
    k = _kernel_notes(_code_object(tmp_path, "gett_f32_stream"))
    flat = {n: v for n, v in k.items() if "gett_f32_stream_kernel" in n and re.search(r"Li3ELi[6-9]ELb0E", n)}
    assert len(flat) == 16, sorted(k)
    for name, v in flat.items():
        assert not v.get("private_segment_fixed_size", 0) and not v.get("vgpr_spill_count", 0) and not v.get("sgpr_spill_count", 0), (name, v)
        assert v["vgpr_count"] <= 256 and v["group_segment_fixed_size"] == 3 * 24 * 1024, (name, v)
