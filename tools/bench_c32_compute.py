#!/usr/bin/env python3
"""complex64 contractions under every compute descriptor: what a caller who asks for less precision gets in time and in digits.

For each shape, eight plans in ONE process (test-hooks library flavour; CUTENSOR_AMD_F32X is read when a plan is made, so the tool sets it
around the plans it forces): COMPUTE_DESC_32F twice (two identical plans: their difference is the run-to-run spread of the measurement),
_TF32 / _16BF / _16F by the default planner, and the same three with CUTENSOR_AMD_F32X=force (the reduced-precision kernels of
csrc/kernels/gett_gen_c32x.inc whenever the descriptor permits them).

Timing: every plan warmed up, then ROUNDS rounds in which the variants ALTERNATE; per round and variant one device-event window of enough
back-to-back calls for at least WINDOW_MS; the median over the rounds is reported (the minimum too).  TFLOP/s = 8 L M N K / time (8 real
flops per complex multiply-add).  Error: against the complex128 contraction of the same operands on the device, over the whole output —
the larger component's |d - ref| over mag = sum (|a_r| + |a_i|)(|b_r| + |b_i|).

One JSON line per (shape, variant), then one per shape that compares each default-planner time with the 32F time + spread.
    python tools/bench_c32_compute.py [--shapes 'a;b;...'] [--out FILE]
    python tools/bench_c32_compute.py --plans-only        (no GPU: the plans and the model's two estimates)"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("CTAMD_LIB_FLAVOUR", "hooks")
# (variant name, compute descriptor, CUTENSOR_AMD_F32X while the plan is made)
VARIANTS = [("32F", "32F", None), ("32F#2", "32F", None),
            ("default TF32", "TF32", None), ("default 16BF", "16BF", None), ("default 16F", "16F", None),
            ("forced TF32", "TF32", "force"), ("forced 16BF", "16BF", "force"), ("forced 16F", "16F", "force")]
ROUNDS = 5
WINDOW_MS = 60.0

HEADLINE = dict(a=96, b=64, c=64, d=64, e=96)
LAYOUTS = (("mk", "kn"), ("km", "kn"), ("mk", "nk"), ("km", "nk"))
# name, extents, (modes of A, B, C — fastest mode first, the ABI's order)
SHAPES = [("%d^3 %s,%s" % (e, mA, mB), dict(m=e, n=e, k=e), (mA, mB, "mn")) for e in (2048, 4096) for (mA, mB) in LAYOUTS] + [
    ("4098^3 km,kn", dict(m=4098, n=4098, k=4098), ("km", "kn", "mn")),
    ("bik,bjk->bij 32x2048x2048x256", dict(b=32, i=2048, j=2048, k=256), ("kib", "kjb", "jib")),
    ("bhqd,bhkd->bhqk 8x8x2048x2048x128", dict(b=8, h=8, q=2048, k=2048, d=128), ("dqhb", "dkhb", "kqhb")),
    ("abcd,dcbe->ae headline", HEADLINE, ("dcba", "ebcd", "ea")),
    ("mlik,lkjm->lij 64,64,512,64,512", dict(m=64, l=64, i=512, k=64, j=512), ("kilm", "mjkl", "jil")),
]


def make_plans(ct, ops, h, ext, modes):
    mA, mB, mC = modes
    e = lambda m: [ext[c] for c in m]   # noqa: E731
    plans = []
    for _, comp, switch in VARIANTS:
        os.environ.pop("CUTENSOR_AMD_F32X", None)
        if switch:
            os.environ["CUTENSOR_AMD_F32X"] = switch
        plans.append(ops.contraction_plan(h, e(mA), mA, e(mB), mB, e(mC), mC, dtype=ct.C_32F, compute=comp, workspace_limit=None))
    os.environ.pop("CUTENSOR_AMD_F32X", None)
    return plans


def brief(d):
    return {"kname": d.get("kname"), "family": d.get("family"), "elem": d.get("elem"), "vec": d.get("vec"), "tile": [d.get("bm"), d.get("bn"), d.get("bk")],
            "splitK": d.get("splitK"), "model_us": d.get("estimate_us", d.get("estimateUs"))}


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def plans_only(names, out):
    sys.path.insert(0, ROOT)
    from cudalibrarysamples_amd import cutensor as ct, ops
    h = ops.Handle()
    for name, ext, modes in SHAPES:
        if names and name not in names:
            continue
        plans = make_plans(ct, ops, h, ext, modes)
        for (vname, _, _), p in zip(VARIANTS, plans):
            emit(dict({"shape": name, "variant": vname, "plans_only": True, "workspace": p.required_workspace}, **brief(p.describe())), out)
            p.destroy()


def measure(names, out):
    import torch
    sys.path.insert(0, ROOT)
    from cudalibrarysamples_amd import cutensor as ct, ops
    h = ops.Handle()

    def logical(buf):
        return buf.permute(*reversed(range(buf.dim())))

    def l1(z):
        return z.real.abs() + z.imag.abs()

    for name, ext, (mA, mB, mC) in SHAPES:
        if names and name not in names:
            continue
        e = lambda m: [ext[c] for c in m]   # noqa: E731
        gen = torch.Generator(device="cuda").manual_seed(1)
        draw = lambda sh: torch.complex(torch.rand(sh, generator=gen, device="cuda") * 2 - 1, torch.rand(sh, generator=gen, device="cuda") * 2 - 1)   # noqa: E731
        A, B = draw(e(mA)[::-1]), draw(e(mB)[::-1])
        D = torch.empty(e(mC)[::-1], dtype=torch.complex64, device="cuda")
        eq = "%s,%s->%s" % (mA, mB, mC)
        a128, b128 = logical(A).to(torch.complex128), logical(B).to(torch.complex128)
        ref = torch.einsum(eq, a128, b128)
        mag = torch.einsum(eq, l1(a128), l1(b128))
        del a128, b128
        flops = 8.0
        for c in set(mA + mB):
            flops *= ext[c]
        plans, info = make_plans(ct, ops, h, ext, (mA, mB, mC)), []
        for p in plans:
            ws = torch.empty(max(p.required_workspace, 256), dtype=torch.uint8, device="cuda")

            def run(p=p, ws=ws):
                p.contract(1.0, A.data_ptr(), B.data_ptr(), 0.0, 0, D.data_ptr(), ws.data_ptr(), p.required_workspace)
            D.fill_(float("nan"))
            run()
            torch.cuda.synchronize()
            got = logical(D)
            err = torch.maximum((got.real.double() - ref.real).abs_(), (got.imag.double() - ref.imag).abs_())
            max_err, rel = float(err.max()), float((err / mag).max())
            del err, got
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
        ms = [statistics.median(it["times"]) for it in info]
        for (vname, _, _), it, t in zip(VARIANTS, info, ms):
            emit(dict({"shape": name, "variant": vname, "ms": round(t, 5), "ms_min": round(min(it["times"]), 5), "tflops": round(flops / (t * 1e-3) / 1e12, 2),
                       "ms_over_32F": round(t / ms[0], 4), "max_err": it["max_err"], "max_err_over_mag": it["rel"], "iters": it["iters"], "rounds": ROUNDS},
                      **brief(it["d"])), out)
        # asking for less precision never costs time: each default-planner time against the 32F time + the spread of the two identical 32F plans
        spread = abs(ms[0] - ms[1])
        emit({"shape": name, "summary": True, "ms_32F": round(ms[0], 5), "spread_ms": round(spread, 5),
              "default_within_32F_plus_spread": {VARIANTS[i][0]: bool(ms[i] <= ms[0] + spread) for i in (2, 3, 4)},
              "default_on_reduced_kernels": {VARIANTS[i][0]: info[i]["d"].get("kname") == "gett_gen_c32x_kernel" for i in (2, 3, 4)},
              "forced_over_32F": {VARIANTS[i][0]: round(ms[i] / ms[0], 4) for i in (5, 6, 7)}}, out)
        for p in plans:
            p.destroy()
        del A, B, D, plans, info
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plans-only", action="store_true", help="no GPU: print every variant's plan")
    ap.add_argument("--shapes", default="", help="shape names separated by ';' (default: all)")
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    a = ap.parse_args()
    names = [s for s in a.shapes.split(";") if s]
    (plans_only if a.plans_only else measure)(names, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
