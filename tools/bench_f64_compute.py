#!/usr/bin/env python3
"""fp64 / complex128 contractions under COMPUTE_DESC_64F and COMPUTE_DESC_32F: what a caller who permits single-precision products gets
in time and in digits.

For each shape four plans: 64F; 32F by the default planner; 32F with CUTENSOR_AMD_F64X=force (the kernels of
csrc/kernels/gett_gen_f64x.inc whenever the descriptor permits them); and a second, identical 64F plan — the spread of the measurement
itself.  The switch is a test hook read when a plan is made (test-hooks library flavour), so all four plans live in ONE process.

Timing: every plan warmed up, then ROUNDS rounds in which the variants ALTERNATE; per round and variant one device-event window of enough
back-to-back calls for at least WINDOW_MS; the median over the rounds is reported (the minimum too).  TFLOP/s = 2 L M N K / time (complex
data: 8).  Error: against the fp64 contraction of the same operands by torch on the device, over the whole output — max |d - ref| and
max |d - ref| / mag (complex: per component, mag = sum (|a_r| + |a_i|)(|b_r| + |b_i|)).

Output, one JSON line each: {"record": "run"} per (shape, variant); {"record": "decision"} per shape — the three times, the kernel the
default planner took under 32F, default-32F / 64F ("never costs time": at most 1 + the spread) and 64F#2 / 64F (the spread);
{"record": "subnormal"} — what becomes of operands and products whose fp32 image is subnormal; {"record": "summary"} — the worst ratio
beside the largest spread, and the forced kernels' rates over 157.3 TFLOP/s at 4096^3 'mk,kn' (complex: 2048^3): the efficiency
constants of pick_gen_choice (kF64xEffReal / kF64xEffCplx, host/plan_contraction.cpp).

    python tools/bench_f64_compute.py [--shapes 'a;b;...'] [--out FILE]      python tools/bench_f64_compute.py --plans-only   (no GPU)"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("CTAMD_LIB_FLAVOUR", "hooks")
SWITCH = "CUTENSOR_AMD_F64X"
# variant name, compute descriptor, value of the switch while the plan is made
VARIANTS = (("64F", "64F", None), ("32F", "32F", None), ("32F forced", "32F", "force"), ("64F#2", "64F", None))
ROUNDS = 5
WINDOW_MS = 60.0
PEAK_F32_MFMA = 157.3      # TFLOP/s, v_mfma_f32_16x16x4_f32 nominal

# kind, M, N, K, modes of A, B (fastest mode first, the ABI's order); C is 'mn'
SHAPES = [
    ("f64", 4096, 4096, 4096, "mk", "kn"), ("f64", 4096, 4096, 4096, "km", "kn"), ("f64", 4096, 4096, 4096, "mk", "nk"),
    ("f64", 2048, 2048, 2048, "mk", "kn"), ("f64", 4096, 4096, 512, "mk", "kn"), ("f64", 1024, 1024, 1024, "mk", "kn"),
    ("f64", 8192, 8192, 256, "mk", "kn"), ("c128", 2048, 2048, 2048, "mk", "kn"), ("c128", 1024, 1024, 1024, "mk", "kn"),
]
EFF_SHAPE = {"f64": ("f64", 4096, 4096, 4096, "mk", "kn"), "c128": ("c128", 2048, 2048, 2048, "mk", "kn")}


def shape_name(s):
    return "%s %dx%dx%d %s,%s" % s


def make_plans(ct, ops, h, shape):
    kind, M, N, K, mA, mB = shape
    ext = dict(m=M, n=N, k=K)
    e = lambda m: [ext[c] for c in m]   # noqa: E731
    plans = []
    for name, comp, sw in VARIANTS:
        os.environ.pop(SWITCH, None)
        if sw:
            os.environ[SWITCH] = sw
        try:
            plans.append(ops.contraction_plan(h, e(mA), mA, e(mB), mB, e("mn"), "mn", dtype=ct.R_64F if kind == "f64" else ct.C_64F, compute=comp,
                                              workspace_limit=None))
        finally:
            os.environ.pop(SWITCH, None)
    return plans


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
    for shape in SHAPES:
        if names and shape_name(shape) not in names:
            continue
        plans = make_plans(ct, ops, h, shape)
        for (name, comp, sw), p in zip(VARIANTS, plans):
            d = p.describe()
            emit({"record": "plan", "shape": shape_name(shape), "variant": name, "kname": d.get("kname"), "elem": d.get("elem"), "vec": d.get("vec"),
                  "tile": [d.get("bm"), d.get("bn"), d.get("bk")], "splitK": d.get("splitK"), "workspace": d.get("workspace")}, out)
            p.destroy()


def subnormal_probe(torch, ct, ops, h, out):
    """64 x 64 x 32, forced kernel, every operand element the same power of two: D = 32 a b when nothing is flushed.
    inputs: a = 2^-130 (fp32 image subnormal), b = 2^20 — the product 2^-110 is a normal fp32 number; products: a = b = 2^-70 — each
    product, and their sum 2^-135, is subnormal in fp32."""
    os.environ[SWITCH] = "force"
    try:
        p = ops.contraction_plan(h, [64, 32], "mk", [32, 64], "kn", [64, 64], "mn", dtype=ct.R_64F, compute="32F", workspace_limit=0)
    finally:
        os.environ.pop(SWITCH, None)
    d = p.describe()
    rec = {"record": "subnormal", "kname": d.get("kname"), "elem": d.get("elem")}
    for what, a, b in (("inputs", 2.0 ** -130, 2.0 ** 20), ("products", 2.0 ** -70, 2.0 ** -70)):
        A = torch.full((32, 64), a, dtype=torch.float64, device="cuda")
        B = torch.full((64, 32), b, dtype=torch.float64, device="cuda")
        D = torch.full((64, 64), float("nan"), dtype=torch.float64, device="cuda")
        ws = torch.empty(256, dtype=torch.uint8, device="cuda")
        p.contract(1.0, A.data_ptr(), B.data_ptr(), 0.0, 0, D.data_ptr(), ws.data_ptr(), 0)
        torch.cuda.synchronize()
        got, want = float(D[0, 0]), 32.0 * a * b
        uniform = bool((D == D[0, 0]).all())
        rec[what] = {"a": a, "b": b, "expected_if_kept": want, "got": got, "all_outputs_equal": uniform,
                     "verdict": "kept" if got == want else "flushed to zero" if got == 0.0 else "other"}
    p.destroy()
    emit(rec, out)


def bench(names, out):
    import torch
    sys.path.insert(0, ROOT)
    from cudalibrarysamples_amd import cutensor as ct, ops
    h = ops.Handle()
    worst_ratio, worst_spread, rates = 0.0, 0.0, {}

    def logical(buf):
        return buf.permute(*reversed(range(buf.dim())))

    def mag_of(x):
        return (x.real.abs() + x.imag.abs()) if x.is_complex() else x.abs()

    for shape in SHAPES:
        name = shape_name(shape)
        if names and name not in names:
            continue
        kind, M, N, K, mA, mB = shape
        ext = dict(m=M, n=N, k=K)
        e = lambda m: [ext[c] for c in m]   # noqa: E731
        gen = torch.Generator(device="cuda").manual_seed(1)

        def draw(sh):
            u = lambda: torch.rand(sh, generator=gen, device="cuda", dtype=torch.float64) * 2 - 1   # noqa: E731
            return u() if kind == "f64" else torch.complex(u(), u())
        A, B = draw(e(mA)[::-1]), draw(e(mB)[::-1])
        D = torch.empty(e("mn")[::-1], device="cuda", dtype=A.dtype)
        eq = "%s,%s->mn" % (mA, mB)
        ref = torch.einsum(eq, logical(A), logical(B))
        mag = torch.einsum(eq, mag_of(logical(A)), mag_of(logical(B)))
        flops = (8.0 if kind == "c128" else 2.0) * M * N * K
        plans, info = make_plans(ct, ops, h, shape), []
        for p in plans:
            ws = torch.empty(max(p.required_workspace, 256), dtype=torch.uint8, device="cuda")

            def run(p=p, ws=ws):
                p.contract(1.0, A.data_ptr(), B.data_ptr(), 0.0, 0, D.data_ptr(), ws.data_ptr(), p.required_workspace)
            D.fill_(float("nan"))
            run()
            torch.cuda.synchronize()
            diff = logical(D) - ref
            err = torch.maximum(diff.real.abs(), diff.imag.abs()) if diff.is_complex() else diff.abs()
            max_err, rel = float(err.max()), float((err / mag).max())
            del diff, err
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
        us = {}
        for (vname, comp, sw), it in zip(VARIANTS, info):
            d = it["d"]
            ms = statistics.median(it["times"])
            us[vname] = ms * 1e3
            emit({"record": "run", "shape": name, "variant": vname, "ms": round(ms, 5), "ms_min": round(min(it["times"]), 5),
                  "tflops": round(flops / (ms * 1e-3) / 1e12, 2), "kname": d.get("kname"), "elem": d.get("elem"), "vec": d.get("vec"),
                  "tile": [d.get("bm"), d.get("bn"), d.get("bk")], "splitK": d.get("splitK"), "max_err": it["max_err"], "max_err_over_mag": it["rel"],
                  "iters": it["iters"], "rounds": ROUNDS}, out)
        ratio, spread = us["32F"] / us["64F"], abs(us["64F#2"] / us["64F"] - 1.0)
        worst_ratio, worst_spread = max(worst_ratio, ratio), max(worst_spread, spread)
        emit({"record": "decision", "kind": kind, "M": M, "N": N, "K": K, "mA": mA, "mB": mB, "64F_us": round(us["64F"], 2), "forced_32F_us": round(us["32F forced"], 2),
              "default_32F_us": round(us["32F"], 2), "default_32F_kernel": info[1]["d"].get("kname"), "forced_over_64F": round(us["32F forced"] / us["64F"], 4),
              "default_32F_over_64F": round(ratio, 4), "spread_64F": round(spread, 4)}, out)
        if shape == EFF_SHAPE[kind]:
            rates[kind] = flops / (us["32F forced"] * 1e-6) / 1e12
        for p in plans:
            p.destroy()
        del A, B, D, plans, info
        torch.cuda.empty_cache()
    subnormal_probe(torch, ct, ops, h, out)
    emit({"record": "summary", "worst_default_32F_over_64F": round(worst_ratio, 4), "largest_spread_64F": round(worst_spread, 4),
          "forced_tflops_at_eff_shape": {k: round(v, 2) for k, v in rates.items()},
          "efficiency_over_157.3": {k: round(v / PEAK_F32_MFMA, 3) for k, v in rates.items()}}, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plans-only", action="store_true", help="print the four plans of every shape; needs no GPU")
    ap.add_argument("--shapes", default="", help="shape names separated by ';' (default: all), e.g. 'f64 4096x4096x4096 mk,kn'")
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    a = ap.parse_args()
    names = [s for s in a.shapes.split(";") if s]
    if a.plans_only:
        plans_only(names, a.out)
    else:
        bench(names, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
