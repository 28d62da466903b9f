"""Host replay of the tile staging of the single-precision-compute fp64 / complex128 GETT kernel (csrc/kernels/gett_gen_f64x.inc)
through csrc/kernels/gett_gen_layout.h — the 4-byte image GenImage<4, 32> / GenFrag<4> of fp64 data rounded to fp32, the 8-byte image of
complex128 rounded to complex64: tests/harness/f64x_layout_harness.cpp stages the A and the B tile with all 256 threads and reads every
MFMA fragment back, for every (element, tile, orientation pair, vector width) of the kernel table.  No GPU."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KDIR = os.path.join(ROOT, "cudalibrarysamples_amd", "csrc", "kernels")
HARNESS = os.path.join(ROOT, "tests", "harness", "f64x_layout_harness.cpp")


def test_tile_staging_and_fragment_reads_agree(tmp_path):
    exe = str(tmp_path / "f64x_layout_harness")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", KDIR, HARNESS, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "f64x layout ok" in r.stdout, r.stdout + r.stderr


def test_the_harness_covers_every_instantiated_shape():
    """Every (staged element bytes, BM, BN, BK, V) of gett_gen_f64x.hip's table is a PAIR of the harness (a PAIR replays the four
    orientation pairs the table's CTAMD_F64X_ORIENTS instantiates)."""
    es = {"GEN_F64_F32": 4, "GEN_C64_C32": 8}
    want = {(es[m.group(1)],) + tuple(int(x) for x in m.groups()[1:])
            for m in re.finditer(r"CTAMD_F64X_ORIENTS\((\w+), (\d+), (\d+), (\d+), (\d+)\)", open(os.path.join(KDIR, "gett_gen_f64x.hip")).read())}
    have = {tuple(int(x) for x in m.groups()) for m in re.finditer(r"PAIR\((\d+), (\d+), (\d+), (\d+), (\d+)\)", open(HARNESS).read())}
    assert len(want) == 6 and want <= have, sorted(want - have)
    # the kernel takes its image and fragment types from the staged element size alone
    inc = open(os.path.join(KDIR, "gett_gen_f64x.inc")).read()
    assert "GenImage<Cfg::ES, BK>" in inc and "GenFrag<Cfg::ES>" in inc and "ES = CPLX ? 8 : 4" in inc
