#!/usr/bin/env python3
"""What a unary operator costs the bandwidth-bound kernels: cutensorPermute 'abc->cab' and cutensorReduce 'abc->ac' on a cubic tensor
(default 2048^3), fp32 and bf16, under IDENTITY and under each of SQRT, RELU, RCP, SIGMOID, TANH, EXP, LOG, ABS, NEG on operand A.

All plans of one workload are made first; then `--rounds` rounds, each timing every operator in turn (`--reps` launches between two
events on the launch stream, after one untimed launch) — IDENTITY and the operators alternate inside one process, so that drift of the
machine lands on all of them alike.  One JSON line per (workload, data type, operator): the median, minimum and maximum over the rounds
of TB/s by the samples' byte counts (permutation: 2 |A| bytes, elementwise_permute.cu:208; reduction: |A| + |D| bytes, reduction.cu:229-231).
A library that refuses an operator (one built before the operators existed) gets a line with "supported": false; its IDENTITY lines are
what a later library's IDENTITY lines are compared with.  A is positive (uniform in [0.5, 2)), so every operator is in its domain.

    python tools/bench_unary.py --out profiles/unary_bandwidth.jsonl
    python tools/bench_unary.py --plans-only      # no GPU: the plans and their descriptions"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

OPERATORS = ("IDENTITY", "SQRT", "RELU", "RCP", "SIGMOID", "TANH", "EXP", "LOG", "ABS", "NEG")
CODES = dict(IDENTITY=1, SQRT=2, RELU=8, RCP=10, SIGMOID=11, TANH=12, EXP=22, LOG=23, ABS=24, NEG=25)      # cutensorOperator_t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5, help="launches per timed window")
    ap.add_argument("--rounds", type=int, default=5, help="times every operator is visited")
    ap.add_argument("--dtypes", default="f32,bf16")
    ap.add_argument("--out", default="", help="append the JSON lines to this file as well")
    ap.add_argument("--label", default="", help="free text copied into every line (which library was measured)")
    ap.add_argument("--plans-only", action="store_true", help="make the plans and print their descriptions; needs no GPU")
    args = ap.parse_args()
    from cudalibrarysamples_amd import ops, cutensor as ct
    n = args.n
    numel = n * n * n
    h = ops.Handle()
    lines = []

    def emit(line):
        line = dict(line, n=n, label=args.label)
        lines.append(line)
        print(json.dumps(line), flush=True)

    def plans(make):
        out = {}
        for name in OPERATORS:
            try:
                out[name] = make(CODES[name])
            except Exception as e:           # a library without the operators: NOT_SUPPORTED
                out[name] = None
                if name == "IDENTITY":
                    raise
                print("# %s refused: %s" % (name, str(e).splitlines()[0]), file=sys.stderr)
        return out

    for dname in args.dtypes.split(","):
        cdt, es = {"f32": (ct.R_32F, 4), "bf16": (ct.R_16BF, 2)}[dname]
        perm = plans(lambda code: ops.permutation_plan(h, [n, n, n], "abc", [n, n, n], "cab", dtype=cdt, opA=code))
        red = plans(lambda code: ops.reduction_plan(h, [n, n, n], "abc", [n, n], "ac", dtype=cdt, opA=code, workspace_limit=1 << 30))
        if args.plans_only:
            for what, ps in (("permute abc->cab", perm), ("reduce abc->ac", red)):
                for name, p in ps.items():
                    emit({"workload": what, "dtype": dname, "operator": name, "supported": p is not None, "plan": p.describe() if p else None})
            continue
        import torch
        tdt = {"f32": torch.float32, "bf16": torch.bfloat16}[dname]
        stream = torch.cuda.current_stream().cuda_stream
        A = torch.empty(numel, dtype=tdt, device="cuda")
        chunk = 1 << 28
        g = torch.Generator(device="cuda")
        g.manual_seed(1234)
        for s in range(0, numel, chunk):
            e = min(numel, s + chunk)
            A[s:e] = (torch.rand(e - s, generator=g, device="cuda", dtype=torch.float32) * 1.5 + 0.5).to(tdt)
        D = torch.empty(numel, dtype=tdt, device="cuda")
        ws = torch.empty(max([p.required_workspace for p in red.values() if p] + [256]), dtype=torch.uint8, device="cuda")
        workloads = (
            ("permute abc->cab", perm, 2.0 * numel * es, lambda p: p.permute(1.0, A.data_ptr(), D.data_ptr(), stream)),
            ("reduce abc->ac", red, (numel + n * n) * float(es),
             lambda p: p.reduce(1.0, A.data_ptr(), 0.0, D.data_ptr(), D.data_ptr(), ws.data_ptr(), p.required_workspace, stream)),
        )
        for what, ps, nbytes, run in workloads:
            tbps = {name: [] for name in ps}
            for name, p in ps.items():          # every code object loaded, every plan run once, before the first timed window
                if p is not None:
                    run(p)
            torch.cuda.synchronize()
            for _ in range(args.rounds):
                for name, p in ps.items():
                    if p is None:
                        continue
                    run(p)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.reps):
                        run(p)
                    e1.record()
                    torch.cuda.synchronize()
                    tbps[name].append(nbytes * args.reps / (e0.elapsed_time(e1) * 1e-3) / 1e12)
            for name, p in ps.items():
                if p is None:
                    emit({"workload": what, "dtype": dname, "operator": name, "supported": False})
                    continue
                v = sorted(tbps[name])
                emit({"workload": what, "dtype": dname, "operator": name, "supported": True, "TBps_median": v[len(v) // 2], "TBps_min": v[0],
                      "TBps_max": v[-1], "rounds": args.rounds, "reps": args.reps, "bytes": nbytes, "plan": p.describe()})
        del A, D, ws
        for p in list(perm.values()) + list(red.values()):
            if p is not None:
                p.destroy()
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
