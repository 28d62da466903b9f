"""The worker hand-off of libcutensorMg.so (csrc/mg/mg_workers.h: one thread per handle device, phases handed out with run() and
collected with wait()) on its own, on the CPU: tests/harness/mg_workers_harness.cpp — a stand-alone program over the header — built plain
and with ThreadSanitizer, and run.  Exit status 0 and no sanitizer report."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [[], ["-fsanitize=thread"]], ids=["plain", "tsan"])
def test_run_wait_rounds_sleep_wake_failure_and_shutdown(tmp_path, flags):
    exe = str(tmp_path / "mg_workers_harness")
    subprocess.check_call(["g++", "-O1", "-pthread", "-std=c++17"] + flags +
                          [os.path.join(ROOT, "tests", "harness", "mg_workers_harness.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "mg workers ok" in r.stdout
    assert r.stderr == "", r.stderr       # a ThreadSanitizer report goes to stderr
