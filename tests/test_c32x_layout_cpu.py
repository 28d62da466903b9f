"""Host replay of the reduced-precision complex64 kernel's tile staging (csrc/kernels/gett_gen_c32x.inc on the index arithmetic of
gett_gen_layout.h): tests/harness/gen_c32x_layout_harness.cpp stages a tile of complex64 units into the real and imaginary 16-bit images
(one plane each for 16BF / 16F, hi and lo for TF32) with all 256 threads — units of V complex64 elements, written per image as 4-byte
pairs (K-contiguous), as 2-byte transposing writes (free-contiguous) or as single 2-byte gathers — and reads every MFMA fragment back,
for every (rows, BK, V, orientation) the kernel table instantiates.  No GPU."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KDIR = os.path.join(ROOT, "cudalibrarysamples_amd", "csrc", "kernels")
HARNESS = os.path.join(ROOT, "tests", "harness", "gen_c32x_layout_harness.cpp")


def test_complex64_units_land_where_the_16_bit_fragment_reads_expect_them(tmp_path):
    exe = str(tmp_path / "gen_c32x_layout_harness")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", KDIR, HARNESS, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "gen c32x layout ok" in r.stdout, r.stdout + r.stderr


def test_the_harness_covers_every_instantiated_shape():
    """Every (planes, rows, BK, V) of gett_gen_c32x.hip's table appears in the harness's REPLAY list (both orientations each)."""
    planes = {"GEN_C32_BF16": 1, "GEN_C32_F16": 1, "GEN_C32_BF16X3": 2}
    src = open(os.path.join(KDIR, "gett_gen_c32x.hip")).read()
    modes = re.findall(r"CTAMD_C32X_MODE\((GEN_\w+)\)", src)
    tiles = [tuple(int(x) for x in m.groups()) for m in re.finditer(r"CTAMD_C32X_ORIENTS\(GE, (\d+), (\d+), (\d+), (\d+)\)", src)]
    assert sorted(modes) == sorted(planes) and len(tiles) == 4, (modes, tiles)
    assert not re.search(r"CTAMD_C32X_ORIENTS\(GEN_", src)          # every instantiation goes through CTAMD_C32X_MODE
    want = set()
    for ge in modes:
        for bm, bn, bk, v in tiles:
            want.add((planes[ge], bm, bk, v))
            want.add((planes[ge], bn, bk, v))
    have = {tuple(int(x) for x in m.groups()) for m in re.finditer(r"REPLAY\((\d+), (\d+), (\d+), (\d+)\)", open(HARNESS).read())}
    assert len(want) >= 8 and want <= have, sorted(want - have)
