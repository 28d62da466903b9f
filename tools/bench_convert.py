#!/usr/bin/env python3
"""What a type conversion inside cutensorPermute costs and saves: the transposition 'abc->cab' and the row copy 'abc->acb' on a cubic
tensor (default 2048^3) for the six converting pairs (bf16 / fp16 <-> fp32, fp32 <-> fp64).

Per workload and pair, five variants alternate inside one process (`--rounds` rounds, each timing every variant in turn: `--reps`
launches between two events on the launch stream, after one untimed launch; every plan runs once before the first timed window), so
that drift of the machine lands on all of them alike:

    convert       the converting plan, A's type -> D's type, one pass
    same_A        the same-type plan in A's type          (the brackets: the converting plan should reach the slower of the two,
    same_D        the same-type plan in D's type           minus the spread)
    same_A_again  a second, identical plan in A's type    (same_A against same_A_again is the run-to-run spread)
    two_pass      what a user did before: the same-type plan in A's type into a temporary, then torch's copy_ into D's type

One JSON line per (workload, pair, variant): median, minimum and maximum over the rounds of TB/s by ALGORITHMIC bytes — |D| (sizeof A +
sizeof D) for convert and two_pass (what the task needs, not what the two passes move), 2 |D| sizeof T for the same-type plans — and the
median milliseconds per launch.  A library that refuses the pair (one built before the conversion existed) gets "supported": false on
the convert line; its same-type lines are what a later library's are compared with.

    python tools/bench_convert.py --out profiles/convert_bandwidth.jsonl
    python tools/bench_convert.py --plans-only      # no GPU: the plans and their descriptions"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PAIRS = ("bf16:f32", "f16:f32", "f32:bf16", "f32:f16", "f32:f64", "f64:f32")
WORKLOADS = {"transpose": ("permute abc->cab", "cab"), "rowcopy": ("permute abc->acb", "acb")}
VARIANTS = ("convert", "same_A", "same_D", "same_A_again", "two_pass")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=3, help="launches per timed window")
    ap.add_argument("--rounds", type=int, default=5, help="times every variant is visited")
    ap.add_argument("--pairs", default=",".join(PAIRS))
    ap.add_argument("--workloads", default="transpose,rowcopy")
    ap.add_argument("--out", default="", help="append the JSON lines to this file as well")
    ap.add_argument("--label", default="", help="free text copied into every line (which library was measured)")
    ap.add_argument("--plans-only", action="store_true", help="make the plans and print their descriptions; needs no GPU")
    args = ap.parse_args()
    from cudalibrarysamples_amd import ops, cutensor as ct
    n = args.n
    numel = n * n * n
    h = ops.Handle()
    lines = []
    types = {"f32": (ct.R_32F, 4), "bf16": (ct.R_16BF, 2), "f16": (ct.R_16F, 2), "f64": (ct.R_64F, 8)}
    pairs = [tuple(p.split(":")) for p in args.pairs.split(",")]

    def emit(line):
        line = dict(line, n=n, label=args.label)
        lines.append(line)
        print(json.dumps(line), flush=True)

    def plan(a, d, modes):
        return ops.permutation_plan(h, [n, n, n], "abc", [n, n, n], modes, dtype=types[a][0], dtypeB=types[d][0])

    if not args.plans_only:
        import torch
        tdt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "f64": torch.float64}
        stream = torch.cuda.current_stream().cuda_stream
        widest = max(types[t][1] for p in pairs for t in p)
        bufA, bufD, bufT = (torch.empty(numel * widest, dtype=torch.uint8, device="cuda") for _ in range(3))
        g = torch.Generator(device="cuda")
        g.manual_seed(1234)

    for a, d in pairs:
        sa, sd = types[a][1], types[d][1]
        if not args.plans_only:
            A, T = bufA[:numel * sa].view(tdt[a]), bufT[:numel * sa].view(tdt[a])
            D, DA = bufD[:numel * sd].view(tdt[d]), bufD[:numel * sa].view(tdt[a])
            AD = bufA[:numel * sd].view(tdt[d])            # the same-type plan of D's type reads its input from A's buffer
            chunk = 1 << 28
            for s in range(0, numel, chunk):               # uniform in [0.5, 2): ordinary values of every type
                e = min(numel, s + chunk)
                A[s:e] = (torch.rand(e - s, generator=g, device="cuda", dtype=torch.float32) * 1.5 + 0.5).to(tdt[a])
        for w in args.workloads.split(","):
            what, modes = WORKLOADS[w]
            ps = {"same_A": plan(a, a, modes), "same_D": plan(d, d, modes), "same_A_again": plan(a, a, modes)}
            try:
                ps["convert"] = plan(a, d, modes)
            except Exception as e:                         # a library without the conversion: NOT_SUPPORTED
                ps["convert"] = None
                print("# %s -> %s refused: %s" % (a, d, str(e).splitlines()[0]), file=sys.stderr)
            conv_bytes = float(numel) * (sa + sd)
            nbytes = {"convert": conv_bytes, "two_pass": conv_bytes, "same_A": 2.0 * numel * sa, "same_A_again": 2.0 * numel * sa, "same_D": 2.0 * numel * sd}
            if args.plans_only:
                for name in ("convert", "same_A", "same_D"):
                    emit({"workload": what, "pair": "%s->%s" % (a, d), "variant": name, "supported": ps[name] is not None, "bytes": nbytes[name],
                          "plan": ps[name].describe() if ps[name] else None})
                for p in ps.values():
                    if p is not None:
                        p.destroy()
                continue

            def two_pass():
                ps["same_A"].permute(1.0, A.data_ptr(), T.data_ptr(), stream)
                D.copy_(T)
            run = {"convert": (lambda: ps["convert"].permute(1.0, A.data_ptr(), D.data_ptr(), stream)) if ps["convert"] else None,
                   "same_A": lambda: ps["same_A"].permute(1.0, A.data_ptr(), DA.data_ptr(), stream),
                   "same_D": lambda: ps["same_D"].permute(1.0, AD.data_ptr(), D.data_ptr(), stream),
                   "same_A_again": lambda: ps["same_A_again"].permute(1.0, A.data_ptr(), DA.data_ptr(), stream),
                   "two_pass": two_pass}
            ms = {name: [] for name in VARIANTS}
            for name in VARIANTS:                          # every code object loaded, every variant run once, before the first timed window
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
                    emit({"workload": what, "pair": "%s->%s" % (a, d), "variant": name, "supported": False})
                    continue
                v = sorted(ms[name])
                tb = lambda t: nbytes[name] / (t * 1e-3) / 1e12   # noqa: E731
                p = ps.get(name if name != "two_pass" else "same_A")
                emit({"workload": what, "pair": "%s->%s" % (a, d), "variant": name, "supported": True, "TBps_median": tb(v[len(v) // 2]),
                      "TBps_min": tb(v[-1]), "TBps_max": tb(v[0]), "ms_median": v[len(v) // 2], "rounds": args.rounds, "reps": args.reps,
                      "bytes": nbytes[name], "plan": p.describe()})
            for p in ps.values():
                if p is not None:
                    p.destroy()
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
