#!/usr/bin/env python3
"""fp32 contractions under every compute descriptor: what a caller who asks for less precision gets in time and in digits.

For each shape: plans with COMPUTE_DESC_32F, _TF32, _16BF, _16F (and a second, identical 32F plan: the spread of the measurement itself)
— by the default planner and with CUTENSOR_AMD_F32X=force (the reduced-precision kernels of csrc/kernels/gett_gen_f32x.inc whenever
the descriptor permits them).  The switch is a test hook read when a plan is made, so each value runs in a child process of its own
(test-hooks library flavour), one after the other, each under a time limit; a child that fails ends the run.

Timing: every plan warmed up, then ROUNDS rounds in which the variants ALTERNATE inside the same process; per round and variant one
device-event window of enough back-to-back calls for at least WINDOW_MS; the median over the rounds is reported (the minimum too).
TFLOP/s = 2 L M N K / time.  Error: against the fp64 contraction of the same fp32 operands on the device, over the whole output —
max |d - ref| and max |d - ref| / sum |a||b|.

One JSON line per (shape, planner, compute).   python tools/bench_f32_compute.py [--shapes 'a;b;...'] [--out FILE]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPUTES = ("32F", "TF32", "16BF", "16F", "32F")          # the second 32F: an identical plan, the measurement's own spread
ROUNDS = 5
WINDOW_MS = 60.0
CHILD_TIMEOUT = 540

HEADLINE = dict(a=96, b=64, c=64, d=64, e=96)
# name, extents, (modes of A, B, C — fastest mode first, the ABI's order)
SHAPES = [
    ("4096^3 mk,kn", dict(m=4096, n=4096, k=4096), ("mk", "kn", "mn")),
    ("4096^3 km,kn", dict(m=4096, n=4096, k=4096), ("km", "kn", "mn")),
    ("4096^3 mk,nk", dict(m=4096, n=4096, k=4096), ("mk", "nk", "mn")),
    ("4096^3 km,nk", dict(m=4096, n=4096, k=4096), ("km", "nk", "mn")),
    ("8192^3 km,kn", dict(m=8192, n=8192, k=8192), ("km", "kn", "mn")),
    ("4098^3 km,kn", dict(m=4098, n=4098, k=4098), ("km", "kn", "mn")),
    ("bhqd,bhkd->bhqk 8x8x2048x2048x128", dict(b=8, h=8, q=2048, k=2048, d=128), ("dqhb", "dkhb", "kqhb")),
    ("bik,bjk->bij 32x2048x2048x256", dict(b=32, i=2048, j=2048, k=256), ("kib", "kjb", "jib")),
    ("contraction.cu default", dict(m=96, n=96, u=96, v=64, h=64, k=64), ("mhkn", "ukvh", "munv")),
    ("abcd,dcbe->ae headline", HEADLINE, ("dcba", "ebcd", "ea")),
    ("mlik,lkjm->lij 64,64,512,64,512", dict(m=64, l=64, i=512, k=64, j=512), ("kilm", "mjkl", "jil")),
]


def child(names):
    import torch
    sys.path.insert(0, ROOT)
    from cudalibrarysamples_amd import cutensor as ct, ops
    h = ops.Handle()
    planner = "forced" if os.environ.get("CUTENSOR_AMD_F32X", "").startswith("f") else "default"

    def logical(buf):
        return buf.permute(*reversed(range(buf.dim())))

    for name, ext, (mA, mB, mC) in SHAPES:
        if names and name not in names:
            continue
        e = lambda m: [ext[c] for c in m]   # noqa: E731
        gen = torch.Generator(device="cuda").manual_seed(1)
        A = torch.rand(e(mA)[::-1], generator=gen, device="cuda") * 2 - 1
        B = torch.rand(e(mB)[::-1], generator=gen, device="cuda") * 2 - 1
        D = torch.empty(e(mC)[::-1], device="cuda")
        eq = "%s,%s->%s" % (mA, mB, mC)
        a64, b64 = logical(A).double(), logical(B).double()
        ref = torch.einsum(eq, a64, b64)
        mag = torch.einsum(eq, a64.abs_(), b64.abs_())
        del a64, b64
        flops = 2.0
        for c in set(mA + mB):
            flops *= ext[c]
        plans, info = [], []
        for comp in COMPUTES:
            p = ops.contraction_plan(h, e(mA), mA, e(mB), mB, e(mC), mC, dtype=ct.R_32F, compute=comp, workspace_limit=None)
            plans.append(p)
            ws = torch.empty(max(p.required_workspace, 256), dtype=torch.uint8, device="cuda")

            def run(p=p, ws=ws):
                p.contract(1.0, A.data_ptr(), B.data_ptr(), 0.0, 0, D.data_ptr(), ws.data_ptr(), p.required_workspace)
            D.fill_(float("nan"))
            run()
            torch.cuda.synchronize()
            err = (logical(D).double() - ref).abs_()
            max_err, rel = float(err.max()), float((err / mag).max())
            del err
            for _ in range(2):
                run()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize()
            iters = max(1, int(WINDOW_MS / max(e0.elapsed_time(e1), 1e-3) + 0.999))
            info.append(dict(run=run, iters=iters, times=[], max_err=max_err, rel=rel, d=p.describe()))
        del ref, mag
        for _ in range(ROUNDS):
            for it in info:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(it["iters"]):
                    it["run"]()
                e1.record()
                torch.cuda.synchronize()
                it["times"].append(e0.elapsed_time(e1) / it["iters"])
        for i, (comp, it) in enumerate(zip(COMPUTES, info)):
            d = it["d"]
            ms = statistics.median(it["times"])
            print(json.dumps({"shape": name, "planner": planner, "compute": comp + ("#2" if i == 4 else ""), "ms": round(ms, 5), "ms_min": round(min(it["times"]), 5),
                              "tflops": round(flops / (ms * 1e-3) / 1e12, 2), "kname": d.get("kname"), "family": d.get("family"), "elem": d.get("elem"),
                              "vec": d.get("vec"), "tile": [d.get("bm"), d.get("bn"), d.get("bk")], "splitK": d.get("splitK"), "max_err": it["max_err"],
                              "max_err_over_mag": it["rel"], "iters": it["iters"], "rounds": ROUNDS}), flush=True)
        for p in plans:
            p.destroy()
        del A, B, D, plans, info
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--shapes", default="", help="shape names separated by ';' (default: all)")
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    a = ap.parse_args()
    names = [s for s in a.shapes.split(";") if s]
    if a.child:
        child(names)
        return 0
    for switch in ("", "force"):
        env = dict(os.environ, CTAMD_LIB_FLAVOUR="hooks")
        env.pop("CUTENSOR_AMD_F32X", None)
        if switch:
            env["CUTENSOR_AMD_F32X"] = switch
        cmd = [sys.executable, os.path.abspath(__file__), "--child"] + (["--shapes", a.shapes] if a.shapes else [])
        # (lines are passed on as they come: a long run stays visibly alive)
        proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True)
        timer = threading.Timer(CHILD_TIMEOUT, proc.kill)
        timer.start()
        try:
            for line in proc.stdout:
                sys.stdout.write(line)
                sys.stdout.flush()
                if a.out:
                    with open(a.out, "a") as f:
                        f.write(line)
            rc = proc.wait()
        finally:
            timer.cancel()
        if rc != 0:
            return rc                 # nothing more is started on the GPU after a failure
    return 0


if __name__ == "__main__":
    sys.exit(main())
