#!/usr/bin/env python3
"""Bandwidth and host cost of cutensorMgCopy on ONE GPU (logical devices: a handle that lists device 0 several times; every
"remote" read is a local one — no number here says anything about reads over xGMI).

Workloads (default n = 8192, fp32 and bf16, handles [0] and [0, 0, 0, 0]):

    rows   n x n from one cell to a 2 x 2 grid of (n / 8)-blocks               'ab -> ab'
    tile   'ab -> ba' between two such grids
    flat   the identical-layout copy between two such grids

Variants, alternated inside one process (`--rounds` rounds, each timing every variant in turn: `--reps` calls after one untimed
call, from an event on the first stream of an idle device to the last of the end events of all streams):

    copy        the cutensorMgCopy plan
    copy_again  a second, identical plan                       (copy against copy_again is the run-to-run spread)
    permute     cutensorPermute of the same logical permutation between two packed one-cell tensors (the single-GPU library's kernels)
    flat_copy   the flat form of cutensorMgCopy over the same bytes (two identical 2 x 2 layouts): the ceiling

One JSON line per (workload, type, handle, variant): median / minimum / maximum TB/s on 2 x the valid bytes, median ms.  Then the
host time of one call from entry to return (rows form, 512 x 512 into a 4 x 2 grid) at 1 / 2 / 4 / 8 logical devices.

    python tools/bench_mg_copy.py --out profiles/mg_copy_bandwidth.jsonl
    python tools/bench_mg_copy.py --plans-only      # no GPU: the plans and their descriptions"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VARIANTS = ("copy", "copy_again", "permute", "flat_copy")
TYPES = {"fp32": (0, 4), "bf16": (14, 2)}


def layouts(n, workload):
    b = n // 8
    grid = lambda m: dict(modes=m, extent=[n, n], block=[b, b], grid=[2, 2])   # noqa: E731
    if workload == "rows":
        return grid("ab"), dict(modes="ab", extent=[n, n])
    if workload == "tile":
        return grid("ba"), grid("ab")
    return grid("ab"), grid("ab")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--types", default="fp32,bf16")
    ap.add_argument("--workloads", default="rows,tile,flat")
    ap.add_argument("--out", default="")
    ap.add_argument("--label", default="")
    ap.add_argument("--plans-only", action="store_true", help="make the plans and print their descriptions; needs no GPU")
    args = ap.parse_args()
    from cudalibrarysamples_amd import cutensormg as cm, ops
    n = args.n
    lines = []

    def emit(line):
        line = dict(line, n=n, label=args.label)
        lines.append(line)
        print(json.dumps(line), flush=True)

    if not args.plans_only:
        import torch
        streams = [torch.cuda.Stream() for _ in range(4)]
        bufS, bufD = (torch.zeros(n * n * 4 + 4096, dtype=torch.uint8, device="cuda") for _ in range(2))
        bufS.random_(0, 256)
        h1 = ops.Handle()

    def cells_of(buf, layout, es):
        """cell pointers inside one buffer: every cell of a 2 x 2 grid of packed blocks holds a quarter of the tensor"""
        ncell = 1
        for g in layout.get("grid") or [1]:
            ncell *= g
        return [buf.data_ptr() + c * (n * n * es // ncell) for c in range(ncell)]

    for w in args.workloads.split(","):
        for t in args.types.split(","):
            dt, es = TYPES[t]
            nbytes = 2.0 * n * n * es
            for devices in ([0], [0, 0, 0, 0]):
                dst, src = layouts(n, w)
                fdst, fsrc = layouts(n, "flat")
                plans = {"copy": cm.CopyPlan(devices, dst, src, dtype=dt), "copy_again": cm.CopyPlan(devices, dst, src, dtype=dt),
                         "flat_copy": cm.CopyPlan(devices, fdst, fsrc, dtype=dt)}
                if args.plans_only:
                    emit({"workload": w, "type": t, "handle": devices, "variant": "copy", "bytes": nbytes, "plan": plans["copy"].describe()})
                    for p in plans.values():
                        p.close()
                    continue
                modes_d = "ba" if w == "tile" else "ab"
                perm = ops.permutation_plan(h1, [n, n], "ab", [n, n], modes_d, dtype=dt)
                ss = [s.cuda_stream for s in streams[:len(devices)]]
                run = {k: (lambda p=p, a=(cells_of(bufD, dst if k != "flat_copy" else fdst, es), cells_of(bufS, src if k != "flat_copy" else fsrc, es)):
                           cm.check(p.run(a[0], a[1], None, ss))) for k, p in plans.items()}
                run["permute"] = lambda: perm.permute(1.0, bufS.data_ptr(), bufD.data_ptr(), ss[0])
                ms = {k: [] for k in VARIANTS}
                for k in VARIANTS:
                    run[k]()
                torch.cuda.synchronize()
                for _ in range(args.rounds):
                    for k in VARIANTS:
                        run[k]()
                        torch.cuda.synchronize()
                        e0 = torch.cuda.Event(enable_timing=True)
                        e0.record(streams[0])
                        for _ in range(args.reps):
                            run[k]()
                        ends = []
                        for s in streams[:len(devices)]:
                            e = torch.cuda.Event(enable_timing=True)
                            e.record(s)
                            ends.append(e)
                        torch.cuda.synchronize()
                        ms[k].append(max(e0.elapsed_time(e) for e in ends) / args.reps)
                for k in VARIANTS:
                    v = sorted(ms[k])
                    tb = lambda x: nbytes / (x * 1e-3) / 1e12   # noqa: E731
                    emit({"workload": w, "type": t, "handle": devices, "variant": k, "TBps_median": tb(v[len(v) // 2]), "TBps_min": tb(v[-1]),
                          "TBps_max": tb(v[0]), "ms_median": v[len(v) // 2], "rounds": args.rounds, "reps": args.reps, "bytes": nbytes,
                          "plan": plans[k].describe() if k in plans else perm.describe()})
                for p in plans.values():
                    p.close()
                perm.destroy()

    # host time of one call, entry to return
    for k in (1, 2, 4, 8):
        dst = dict(modes="ab", extent=[512, 512], block=[64, 64], grid=[4, 2])
        src = dict(modes="ab", extent=[512, 512])
        p = cm.CopyPlan([0] * k, dst, src, dtype=0)
        if args.plans_only:
            emit({"workload": "host_time", "handle": [0] * k, "plan": p.describe()})
            p.close()
            continue
        hs = [torch.cuda.Stream() for _ in range(max(0, k - len(streams)))]
        ss = [s.cuda_stream for s in (streams + hs)[:k]]
        cells = [bufD.data_ptr() + c * 512 * 512 * 4 // 8 for c in range(8)]
        us = []
        for i in range(60):
            t0 = time.perf_counter()
            st = p.run(cells, [bufS.data_ptr()], None, ss)
            us.append((time.perf_counter() - t0) * 1e6)
            assert st == 0
            if i % 10 == 9:
                torch.cuda.synchronize()
        v = sorted(us[10:])
        emit({"workload": "host_time", "handle": [0] * k, "us_median": v[len(v) // 2], "us_min": v[0], "us_max": v[-1], "calls": len(v),
              "launches": sum(len(d["launches"]) for d in p.describe()["devices"])})
        p.close()
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
