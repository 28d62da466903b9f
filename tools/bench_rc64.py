#!/usr/bin/env python3
"""A real fp64 tensor contracted with a complex128 one: the mixed plan (csrc/kernels/gett_gen_rc64.inc: the real operand staged as it is,
two fp64 MFMAs per product) against what a caller did before it existed — widen the real tensor to complex128, then the complex128 plan.

For each shape four variants, ALTERNATED in one process:
  (a) "mixed"        the mixed plan on the real tensor
  (b) "c128"         the complex128 plan on a pre-widened copy (the widening copy is NOT timed)
  (c) "widen+c128"   torch's .to(complex128) of the real tensor, then (b): what the caller paid in all
  (d) "c128#2"       a second, identical complex128 plan: the run-to-run spread of the measurement itself
The real tensor is the caller's A (`--real B`: the caller's B).

Timing: every variant warmed up, then ROUNDS rounds in which the variants alternate; per round and variant one device-event window of
enough back-to-back calls for at least WINDOW_MS; the median over the rounds is reported (the minimum too).  TFLOP/s counts the real
operations of the algorithm: 4 L M N K for the mixed plan (two real multiply-adds per product), 8 L M N K for complex128.  Error: max
per-component |d - ref| over the whole output against a complex128 einsum of the widened operands on the CPU (shapes up to CPU_REF_WORK
multiply-adds; beyond that the same einsum by torch on the device, and the record says so).

Output, one JSON line each: {"record": "run"} per (shape, variant); {"record": "ratio"} per shape — mixed / c128 (must not exceed 1 + the
spread), mixed / (widen + c128), the spread c128#2 / c128, and the mixed rate as a fraction of the 78.6 TFLOP/s fp64 MFMA peak;
{"record": "summary"} — the worst ratio beside the largest spread, and the rate at 2048^3 'mk,kn' over 78.6: the efficiency constant of
the planner's estimate (kRc64GenEff, host/plan_contraction.cpp).

    python tools/bench_rc64.py [--shapes 'a;b;...'] [--real A|B] [--out profiles/rc64_compute.jsonl]
    python tools/bench_rc64.py --plans-only        (no GPU)
Bank conflicts: a counter pass of its own around a short run, e.g.
    rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE -d DIR -o r -- python tools/bench_rc64.py --rounds 1 --window-ms 1 --shapes '1024x1024x1024 mk,kn;...'
and tools/rocprof_summary.py on its database: conflict cycles over LDS-active cycles per kernel."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("CTAMD_LIB_FLAVOUR", "hooks")
VARIANTS = ("mixed", "c128", "widen+c128", "c128#2")
ROUNDS = 5
WINDOW_MS = 60.0
PEAK_F64_MFMA = 78.6        # TFLOP/s, v_mfma_f64_16x16x4_f64
CPU_REF_WORK = 1e10          # multiply-adds up to which the reference is computed on the CPU (every default shape)

# name, extents, modes of A, B, D (fastest mode first, the ABI's order)
SHAPES = []
for _n in (2048, 1024):
    for _mA, _mB in (("mk", "kn"), ("km", "kn"), ("mk", "nk"), ("km", "nk")):
        SHAPES.append(("%dx%dx%d %s,%s" % (_n, _n, _n, _mA, _mB), dict(m=_n, n=_n, k=_n), (_mA, _mB, "mn")))
SHAPES.append(("batch bik,bjk->bij 16x1024x1024x256", dict(b=16, i=1024, j=1024, k=256), ("kib", "kjb", "jib")))      # row-major 'bik,bjk->bij' reversed
SHAPES.append(("splitk 128x128x65536 km,kn", dict(m=128, n=128, k=65536), ("km", "kn", "mn")))
EFF_SHAPE = "2048x2048x2048 mk,kn"


def make_plans(ct, ops, h, shape, real):
    _, ext, (mA, mB, mC) = shape
    e = lambda m: [ext[c] for c in m]   # noqa: E731
    kw = dict(dtype=ct.C_64F, workspace_limit=None)
    mixed = ops.contraction_plan(h, e(mA), mA, e(mB), mB, e(mC), mC, **dict(kw, **{"dtypeA" if real == 0 else "dtypeB": ct.R_64F}))
    c128 = ops.contraction_plan(h, e(mA), mA, e(mB), mB, e(mC), mC, **kw)
    c128b = ops.contraction_plan(h, e(mA), mA, e(mB), mB, e(mC), mC, **kw)
    return mixed, c128, c128b


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def plan_record(d):
    return {"kname": d.get("kname"), "elem": d.get("elem"), "vec": d.get("vec"), "real": d.get("real"), "tile": [d.get("bm"), d.get("bn"), d.get("bk")],
            "splitK": d.get("splitK"), "workspace": d.get("workspace"), "model_us": d.get("model_us")}


def plans_only(names, real, out):
    sys.path.insert(0, ROOT)
    from cudalibrarysamples_amd import cutensor as ct, ops
    h = ops.Handle()
    for shape in SHAPES:
        if names and shape[0] not in names:
            continue
        plans = make_plans(ct, ops, h, shape, real)
        for vname, p in zip(("mixed", "c128", "c128#2"), plans):
            emit(dict({"record": "plan", "shape": shape[0], "variant": vname}, **plan_record(p.describe())), out)
            p.destroy()


def bench(names, real, out):
    import torch
    sys.path.insert(0, ROOT)
    from cudalibrarysamples_amd import cutensor as ct, ops
    h = ops.Handle()
    worst_ratio, worst_spread, eff = 0.0, 0.0, None

    def logical(buf):
        return buf.permute(*reversed(range(buf.dim())))

    for shape in SHAPES:
        name, ext, (mA, mB, mC) = shape
        if names and name not in names:
            continue
        e = lambda m: [ext[c] for c in m]   # noqa: E731
        gen = torch.Generator(device="cuda").manual_seed(1)
        u = lambda sh: torch.rand(sh, generator=gen, device="cuda", dtype=torch.float64) * 2 - 1   # noqa: E731
        X = [None, None]
        for i, m in enumerate((mA, mB)):
            X[i] = u(e(m)[::-1]) if i == real else torch.complex(u(e(m)[::-1]), u(e(m)[::-1]))
        W = X[real].to(torch.complex128)                    # the pre-widened copy of (b)
        D = torch.empty(e(mC)[::-1], device="cuda", dtype=torch.complex128)
        work = 1.0
        for v in ext.values():
            work *= v
        eq = "%s,%s->%s" % (mA, mB, mC)
        wide = [logical(W if i == real else X[i]) for i in (0, 1)]
        on_cpu = work <= CPU_REF_WORK
        ref = torch.einsum(eq, *[w.cpu() for w in wide]) if on_cpu else torch.einsum(eq, *wide).cpu()
        mixed, c128, c128b = make_plans(ct, ops, h, shape, real)
        ws = torch.empty(max(256, mixed.required_workspace, c128.required_workspace), dtype=torch.uint8, device="cuda")

        def run_mixed():
            mixed.contract(1.0, X[0].data_ptr(), X[1].data_ptr(), 0.0, 0, D.data_ptr(), ws.data_ptr(), mixed.required_workspace)

        def run_c128(p=c128, w=W):
            ab = [w.data_ptr() if i == real else X[i].data_ptr() for i in (0, 1)]
            p.contract(1.0, ab[0], ab[1], 0.0, 0, D.data_ptr(), ws.data_ptr(), p.required_workspace)

        def run_widen():
            run_c128(c128, X[real].to(torch.complex128))

        runs = {"mixed": run_mixed, "c128": run_c128, "widen+c128": run_widen, "c128#2": lambda: run_c128(c128b)}
        descs = {"mixed": mixed.describe(), "c128": c128.describe(), "widen+c128": c128.describe(), "c128#2": c128b.describe()}
        info = []
        for vname in VARIANTS:
            run = runs[vname]
            D.fill_(float("nan"))
            run()
            torch.cuda.synchronize()
            diff = logical(D).cpu() - ref
            max_err = float(torch.maximum(diff.real.abs(), diff.imag.abs()).max())
            del diff
            for _ in range(2):
                run()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize()
            iters = max(1, int(WINDOW_MS / max(e0.elapsed_time(e1), 1e-3) + 0.999))
            info.append(dict(name=vname, run=run, iters=iters, times=[], max_err=max_err))
        del ref
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
        for it in info:
            ms = statistics.median(it["times"])
            us[it["name"]] = ms * 1e3
            flops = (4.0 if it["name"] == "mixed" else 8.0) * work
            emit(dict({"record": "run", "shape": name, "variant": it["name"], "real_operand": "AB"[real], "ms": round(ms, 5), "ms_min": round(min(it["times"]), 5),
                       "tflops": round(flops / (ms * 1e-3) / 1e12, 2), "flops_per_multiply_add": 4 if it["name"] == "mixed" else 8,
                       "max_err": it["max_err"], "reference": "cpu complex128" if on_cpu else "device complex128", "iters": it["iters"], "rounds": ROUNDS},
                      **plan_record(descs[it["name"]])), out)
        ratio, spread = us["mixed"] / us["c128"], abs(us["c128#2"] / us["c128"] - 1.0)
        rate = 4.0 * work / (us["mixed"] * 1e-6) / 1e12
        worst_ratio, worst_spread = max(worst_ratio, ratio), max(worst_spread, spread)
        emit({"record": "ratio", "shape": name, "real_operand": "AB"[real], "mixed_us": round(us["mixed"], 2), "c128_us": round(us["c128"], 2),
              "widen_c128_us": round(us["widen+c128"], 2), "mixed_over_c128": round(ratio, 4), "mixed_over_widen_c128": round(us["mixed"] / us["widen+c128"], 4),
              "spread_c128": round(spread, 4), "not_slower_beyond_spread": bool(ratio <= 1.0 + spread), "mixed_tflops": round(rate, 2),
              "mixed_fraction_of_78.6": round(rate / PEAK_F64_MFMA, 3)}, out)
        if name == EFF_SHAPE:
            eff = rate
        for p in (mixed, c128, c128b):
            p.destroy()
        del X, W, D, wide, info, runs
        torch.cuda.empty_cache()
    emit({"record": "summary", "real_operand": "AB"[real], "worst_mixed_over_c128": round(worst_ratio, 4), "largest_spread_c128": round(worst_spread, 4),
          "mixed_tflops_at_eff_shape": None if eff is None else round(eff, 2), "efficiency_over_78.6": None if eff is None else round(eff / PEAK_F64_MFMA, 3)}, out)


def main():
    global ROUNDS, WINDOW_MS
    ap = argparse.ArgumentParser()
    ap.add_argument("--plans-only", action="store_true", help="print the plans of every shape; needs no GPU")
    ap.add_argument("--shapes", default="", help="shape names separated by ';' (default: all), e.g. '2048x2048x2048 mk,kn'")
    ap.add_argument("--real", default="A", choices=("A", "B"), help="which of the caller's inputs is the real tensor")
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    ap.add_argument("--rounds", type=int, default=ROUNDS, help="alternating rounds per shape")
    ap.add_argument("--window-ms", type=float, default=WINDOW_MS, help="least length of one timed window (a counter pass wants it short)")
    a = ap.parse_args()
    ROUNDS, WINDOW_MS = a.rounds, a.window_ms
    names = [s for s in a.shapes.split(";") if s]
    real = "AB".index(a.real)
    if a.plans_only:
        plans_only(names, real, a.out)
    else:
        bench(names, real, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
