#!/usr/bin/env python3
"""What one complex element-wise trinary call costs against the two binary calls a caller needed before it existed:

    D = alpha * conj(perm A) + beta * perm B + gamma * C        on complex64 / complex128 tensors

at 512 x 256 x 256 and at the trinary sample's 400 x 200 x 300, for each form of the trinary planner: E ('abc, cab -> abc': A has D's
layout), two tiles ('cba, cab -> abc': both permuted, shared tile modes) and two passes ('cba, bac -> abc').

Per shape, type and form, three variants alternate inside one process (`--rounds` rounds, each timing every variant in turn: `--reps`
launches between two events on the launch stream, after one untimed launch; every plan runs once before the first timed window), so that
drift of the machine lands on all of them alike:

    trinary        the one trinary call
    two_binary     cutensorElementwiseBinaryExecute twice: D = alpha conj(perm A) + gamma C, then D = beta perm B + 1 D in place (6 |D| bytes)
    trinary_again  a second, identical trinary plan (trinary against trinary_again is the run-to-run spread)

One JSON line per (shape, type, form, variant): median, minimum and maximum over the rounds of TB/s by ALGORITHMIC bytes — 4 |D| sizeof T
for every variant: what the task needs, not what two calls move — and the median milliseconds per call.  A library that refuses the
trinary plan (one built before the complex kernels) gets "supported": false on the trinary lines; its two_binary lines are what a later
library's are compared with.

    python tools/bench_cplx_trinary.py --out profiles/cplx_trinary_bandwidth.jsonl
    python tools/bench_cplx_trinary.py --plans-only      # no GPU: the plans and their descriptions"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ("512x256x256", "400x200x300")
TYPES = ("c64", "c128")
FORMS = {"E": ("abc", "cab"), "two_tiles": ("cba", "cab"), "two_pass": ("cba", "bac")}      # modes of A and B; C and D are 'abc'
VARIANTS = ("trinary", "two_binary", "trinary_again")
ALPHA, BETA, GAMMA = 0.75 - 0.5j, -0.5 + 1.25j, 1.5 + 0.25j


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--types", default=",".join(TYPES))
    ap.add_argument("--forms", default=",".join(FORMS))
    ap.add_argument("--reps", type=int, default=3, help="launches per timed window")
    ap.add_argument("--rounds", type=int, default=5, help="times every variant is visited")
    ap.add_argument("--out", default="", help="append the JSON lines to this file as well")
    ap.add_argument("--label", default="", help="free text copied into every line (which library was measured)")
    ap.add_argument("--plans-only", action="store_true", help="make the plans and print their descriptions; needs no GPU")
    args = ap.parse_args()
    from cudalibrarysamples_amd import ops, cutensor as ct
    h = ops.Handle()
    lines = []
    types = {"c64": (ct.C_32F, 8), "c128": (ct.C_64F, 16)}

    def emit(line):
        line = dict(line, label=args.label)
        lines.append(line)
        print(json.dumps(line), flush=True)

    if not args.plans_only:
        import torch
        tdt = {"c64": torch.complex64, "c128": torch.complex128}
        stream = torch.cuda.current_stream().cuda_stream
        g = torch.Generator(device="cuda")
        g.manual_seed(1234)

    for shape in args.shapes.split(","):
        a, b, c = (int(x) for x in shape.split("x"))
        ext = dict(a=a, b=b, c=c)
        numel = a * b * c
        e = lambda m: [ext[x] for x in m]   # noqa: E731
        for t in args.types.split(","):
            dt, size = types[t]
            nbytes = 4.0 * numel * size
            if not args.plans_only:
                bufs = []
                for _ in range(4):                                 # A, B, C, D: N(0, 1) parts (D is overwritten)
                    x = torch.empty(numel, dtype=tdt[t], device="cuda")
                    torch.view_as_real(x).normal_(generator=g)
                    bufs.append(x)
                A, B, C, D = (x.data_ptr() for x in bufs)
            for form in args.forms.split(","):
                mA, mB = FORMS[form]
                what = "%s, %s -> abc" % (mA, mB)

                def trinary():
                    return ops.trinary_plan(h, e(mA), mA, e(mB), mB, e("abc"), "abc", e("abc"), "abc", dtype=dt, opA="CONJ")
                ps = {"bin1": ops.binary_plan(h, e(mA), mA, e("abc"), "abc", dtype=dt, opA="CONJ"), "bin2": ops.binary_plan(h, e(mB), mB, e("abc"), "abc", dtype=dt)}
                try:
                    ps["trinary"], ps["trinary_again"] = trinary(), trinary()
                except Exception as err:                           # a library without the complex trinary kernels: NOT_SUPPORTED
                    ps["trinary"] = ps["trinary_again"] = None
                    print("# %s %s %s refused: %s" % (shape, t, form, str(err).splitlines()[0]), file=sys.stderr)
                key = {"shape": shape, "type": t, "form": form, "workload": what, "bytes": nbytes}
                if args.plans_only:
                    emit(dict(key, variant="trinary", supported=ps["trinary"] is not None, plan=ps["trinary"].describe() if ps["trinary"] else None))
                    emit(dict(key, variant="two_binary", supported=True, plan=[ps["bin1"].describe(), ps["bin2"].describe()]))
                    for p in ps.values():
                        if p is not None:
                            p.destroy()
                    continue

                def two_binary():
                    ps["bin1"].binary(ALPHA, A, GAMMA, C, D, stream)
                    ps["bin2"].binary(BETA, B, 1.0, D, D, stream)
                run = {"trinary": (lambda: ps["trinary"].trinary(ALPHA, A, BETA, B, GAMMA, C, D, stream)) if ps["trinary"] else None,
                       "two_binary": two_binary,
                       "trinary_again": (lambda: ps["trinary_again"].trinary(ALPHA, A, BETA, B, GAMMA, C, D, stream)) if ps["trinary_again"] else None}
                ms = {name: [] for name in VARIANTS}
                for name in VARIANTS:                              # every code object loaded, every variant run once, before the first timed window
                    if run[name] is not None:
                        run[name]()
                torch.cuda.synchronize()
                for _ in range(args.rounds):
                    for name in VARIANTS:
                        if run[name] is None:
                            continue
                        run[name]()
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(args.reps):
                            run[name]()
                        e1.record()
                        torch.cuda.synchronize()
                        ms[name].append(e0.elapsed_time(e1) / args.reps)
                for name in VARIANTS:
                    if run[name] is None:
                        emit(dict(key, variant=name, supported=False))
                        continue
                    v = sorted(ms[name])
                    tb = lambda x: nbytes / (x * 1e-3) / 1e12   # noqa: E731
                    plan = [ps["bin1"].describe(), ps["bin2"].describe()] if name == "two_binary" else ps[name].describe()
                    emit(dict(key, variant=name, supported=True, TBps_median=tb(v[len(v) // 2]), TBps_min=tb(v[-1]), TBps_max=tb(v[0]),
                              ms_median=v[len(v) // 2], ms_min=v[0], ms_max=v[-1], rounds=args.rounds, reps=args.reps, plan=plan))
                for p in ps.values():
                    if p is not None:
                        p.destroy()
            if not args.plans_only:
                del bufs
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
