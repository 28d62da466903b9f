"""tools/bench_convert.py --plans-only (no GPU): the tool makes, for both workloads and all six pairs, the converting plan and its two
same-type brackets, on the kernels it says it measures."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_convert_plans_only(built):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_convert.py"), "--plans-only", "--n", "2048"], capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 2 * 6 * 3 and all(x["supported"] for x in lines), r.stdout[-2000:]
    size = {"bf16": 2, "f16": 2, "f32": 4, "f64": 8}
    for x in lines:
        a, d = x["pair"].split("->")
        want_variant = 0 if x["workload"].endswith("cab") else 1               # EW_TRANSPOSE / EW_ROWCOPY
        assert x["plan"]["variant"] == want_variant, x
        assert ("convert" in x["plan"]) == (x["variant"] == "convert"), x
        if x["variant"] == "convert":
            assert x["bytes"] == 2048.0 ** 3 * (size[a] + size[d]), x
