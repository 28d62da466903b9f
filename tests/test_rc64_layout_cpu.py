"""Host replay of the mixed fp64 x complex128 GETT kernel's tile staging (csrc/kernels/gett_gen_rc64.inc on the index arithmetic of
gett_gen_layout.h): tests/harness/gen_rc64_layout_harness.cpp stages a tile of each operand with all 256 threads — the real one as
8-byte elements, the complex one as 16-byte elements — and reads every fragment of the two-MFMA step back, for every (real side,
orientation pair, real vector width) the kernel table instantiates.  No GPU."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KDIR = os.path.join(ROOT, "cudalibrarysamples_amd", "csrc", "kernels")


def test_both_operands_stage_and_the_two_mfma_step_reads_agree(tmp_path):
    exe = str(tmp_path / "gen_rc64_layout_harness")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", KDIR, os.path.join(ROOT, "tests", "harness", "gen_rc64_layout_harness.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "rc64 layout ok" in r.stdout, r.stdout + r.stderr


def test_the_harness_covers_every_instantiated_row():
    """Every (real side, real width) row group of gett_gen_rc64.hip appears in the harness, the four orientation pairs of a group are
    the same four in both, and the kernel's tile is the one the harness replays."""
    hip = open(os.path.join(KDIR, "gett_gen_rc64.hip")).read()
    inc = open(os.path.join(KDIR, "gett_gen_rc64.inc")).read()
    src = open(os.path.join(ROOT, "tests", "harness", "gen_rc64_layout_harness.cpp")).read()
    want = {tuple(int(x) for x in m.groups()) for m in re.finditer(r"CTAMD_GEN_RC64_ORIENTS\((\d+), (\d+)\)", hip)}
    have = {tuple(int(x) for x in m.groups()) for m in re.finditer(r"REPLAY_ORIENTS\((\d+), (\d+)\)", src.split("int main")[1])}
    assert len(want) == 4 and want == have, (sorted(want), sorted(have))
    pairs = lambda text, name: sorted(m.groups() for m in re.finditer(name + r"\(SIDE, (\d), (\d), VR\)", text))
    assert pairs(inc, "CTAMD_GEN_RC64_ENTRY") == pairs(src, "REPLAY_ENTRY") == [("0", "0"), ("0", "1"), ("1", "0"), ("1", "1")]
    assert "BM = 64, BN = 64, BK = 8" in inc and "ROWS = 64, BK = 8" in src
