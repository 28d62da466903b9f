"""tools/bench_cplx_trinary.py --plans-only (no GPU): the tool makes, for both shapes, both types and the three forms, the trinary plan
on the form it says it measures and the two binary plans it compares with."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_cplx_trinary_plans_only(built):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_cplx_trinary.py"), "--plans-only"], capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 2 * 2 * 3 * 2 and all(x["supported"] for x in lines), r.stdout[-2000:]
    size = {"c64": 8, "c128": 16}
    form = {"E": dict(passes=1, bothPermuted=0, swapAB=0), "two_tiles": dict(passes=1, bothPermuted=1), "two_pass": dict(passes=2, bothPermuted=0)}
    for x in lines:
        a, b, c = (int(v) for v in x["shape"].split("x"))
        assert x["bytes"] == 4.0 * a * b * c * size[x["type"]], x
        if x["variant"] == "trinary":
            p = x["plan"]
            assert p["form"] == "trinary" and p["conj"] == [1, 0, 0] and all(p[k] == v for k, v in form[x["form"]].items()), x
            # the transposing tiles of 16-byte lanes: 128 x 32 complex64 (64 x 64 with a second tile), 64 x 32 complex128
            assert p["variant"] == 0 and p["tile0"] == (128 if x["type"] == "c64" and x["form"] != "two_tiles" else 64), x
        else:
            assert len(x["plan"]) == 2 and all("form" not in p for p in x["plan"]), x
