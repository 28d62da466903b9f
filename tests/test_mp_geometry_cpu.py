"""The box arithmetic of libcutensorMp.so (csrc/mp/mp_geometry.h: cells, intersections, needed boxes, offsets, the modes and launch
offsets of a copy) on its own, on the CPU: tests/harness/mp_geometry_harness.cpp — a stand-alone program over the header that checks
every function against brute-force enumeration on extents <= 7 — built plain and with AddressSanitizer + UBSan, and run.  Exit status 0
and no sanitizer report."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan-ubsan"])
def test_boxes_offsets_and_copy_launches_against_enumeration(tmp_path, flags):
    exe = str(tmp_path / "mp_geometry_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include"] + flags +
                          [os.path.join(ROOT, "tests", "harness", "mp_geometry_harness.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "mp geometry ok" in r.stdout
    assert r.stderr == "", r.stderr       # a sanitizer report goes to stderr
