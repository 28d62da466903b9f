"""Host replay of the reduced-precision fp32 kernel's tile staging (csrc/kernels/gett_gen_f32x.inc on the index arithmetic of
gett_gen_layout.h): tests/harness/gen_f32x_layout_harness.cpp stages a tile of fp32 units into the 16-bit image(s) with all 256 threads —
units of V fp32 elements, written as 8-byte groups of four (K-contiguous), as 2-byte transposing writes (free-contiguous) or as single
2-byte gathers — and reads every MFMA fragment back, for every (rows, BK, V, orientation) the kernel table instantiates.  No GPU."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KDIR = os.path.join(ROOT, "cudalibrarysamples_amd", "csrc", "kernels")
HARNESS = os.path.join(ROOT, "tests", "harness", "gen_f32x_layout_harness.cpp")


def test_fp32_units_land_where_the_16_bit_fragment_reads_expect_them(tmp_path):
    exe = str(tmp_path / "gen_f32x_layout_harness")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", KDIR, HARNESS, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "gen f32x layout ok" in r.stdout, r.stdout + r.stderr


def test_the_harness_covers_every_instantiated_shape():
    """Every (planes, rows, BK, V) of gett_gen_f32x.hip's table appears in the harness's REPLAY list (both orientations each)."""
    planes = {"GEN_F32_BF16": 1, "GEN_F32_F16": 1, "GEN_F32_BF16X3": 2}
    want = set()
    for m in re.finditer(r"CTAMD_F32X_ORIENTS\((\w+), (\d+), (\d+), (\d+), (\d+)\)", open(os.path.join(KDIR, "gett_gen_f32x.hip")).read()):
        ge, bm, bn, bk, v = m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4)), int(m.group(5))
        want.add((planes[ge], bm, bk, v))
        want.add((planes[ge], bn, bk, v))
    have = {tuple(int(x) for x in m.groups()) for m in re.finditer(r"REPLAY\((\d+), (\d+), (\d+), (\d+)\)", open(HARNESS).read())}
    assert len(want) >= 8 and want <= have, sorted(want - have)
