"""bench.py as it is run for every change: a plain run times the headline alone (nothing else measured on the line), and
--dump-outputs writes the result of the last timed step, which is the einsum of the seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_plain_run_dumps_the_headline_result(built, tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 7 and line["warmup"] == 2 and line["ms_per_step"] > 0 and line["value"] > 0, line
    assert line["metric"] == "contraction GFLOP/s, fp32 einsum abcd,dcbe->ae" and line["unit"] == "GFLOP/s" and line["dtype"] == "f32"
    assert line["higher_is_better"] is True and line["value_is"] == "einsum_value"
    # what --full adds is not measured
    assert line["secondary"] == [] and line["roofline"] is None and line["cpu_baseline"] is None and line["cold_operands"] is None
    assert line["sample_protocol"] is None
    assert sorted(os.listdir(str(tmp_path))) == ["C.npy"]
    got = np.load(str(tmp_path / "C.npy"))
    assert got.dtype == np.float32 and got.shape == (96, 96)
    # the inputs bench.py draws: U(0,1) fp32 from a device generator seeded 1234, A (96, 64, 64, 64) then B (64, 64, 64, 96)
    import torch

    import oracle
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)
    a = torch.rand((96, 64, 64, 64), generator=g, device="cuda", dtype=torch.float32).cpu().numpy()
    b = torch.rand((64, 64, 64, 96), generator=g, device="cuda", dtype=torch.float32).cpu().numpy()
    rows = [0, 1, 47, 95]
    ref = oracle.einsum("abcd,dcbe->ae", np.ascontiguousarray(a[rows]), b)
    np.testing.assert_allclose(got[rows], ref, rtol=1e-4)
