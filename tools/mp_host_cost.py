#!/usr/bin/env python3
"""Host side of ONE cutensorMpContract call, rank threads of one process on one GPU (the library's in-process exchange layer): the
per-call wall clock of 200 back-to-back calls per rank on three small layouts of tests/mp_plan_cases.py — "sub-box transfers" on 4 ranks
(pack + exchange + unpack), "k distributed, C sharded, beta" on 2 ranks (reduce-scatter) and "row-sharded, B replicated" on 2 ranks (no
exchange).  The problems are small, so the figure is the cost of the machinery: copies enqueued, transfers posted and matched, the local
contraction launched, the rank threads meeting in the exchange.  One JSON line per layout: the median and the maximum over ranks of the
per-call time, and what a call does according to ctamdMpDescribePlan (transfers, copy launches, contractions), summed over ranks.

    python tools/mp_host_cost.py [tree-label [run-number]]     # the labels are copied into every line
"""
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAYOUTS = ["sub-box transfers", "k distributed, C sharded, beta", "row-sharded, B replicated: no exchange"]
REPS = 200


def copy_launches(d):
    """launches of every copy of a call (older descriptions list the transfers' launches only)"""
    n = sum(t["launches"] for t in d["sends"] + d["recvs"])
    n += sum(len(c["launches"]) for o in d.get("operands") or [] for c in o["localCopies"])
    r = d.get("reduce")
    if r:
        n += sum(len(c["launches"]) for c in [r["cIn"], r["out"], r["unpack"]] + r["pack"] if c)
    return n


def measure(cmp, ct, torch, pc, case):
    name, eq, ext, dist, nranks, _, alpha, beta = case[:8]
    world = cmp.LocalWorld(nranks)
    per_call, described = [None] * nranks, [None] * nranks

    def body(r):
        torch.cuda.set_device(0)
        stream = torch.cuda.Stream()
        rp = pc.RankPlan((cmp, ct), world, r, eq, ext, dist, nranks, device=0, stream=ctypes.c_void_p(stream.cuda_stream))
        cmp.check(rp.status)
        described[r] = cmp.describe_plan(rp.plan)
        modes, P = pc.split_modes(eq), pc.grid(eq, dist)
        bufs = []
        for k in range(3):
            n = 1
            for b in pc.block_sizes(ext, modes[k], P[k]):
                n *= b
            bufs.append(torch.rand(n, device="cuda"))
        ws = torch.empty(max(rp.required_device(), 256), dtype=torch.uint8, device="cuda")
        a, b = ctypes.c_float(alpha), ctypes.c_float(beta)
        call = lambda: cmp.check(cmp.cutensorMpContract(rp.h, rp.plan, ctypes.byref(a), bufs[0].data_ptr(), bufs[1].data_ptr(), ctypes.byref(b),  # noqa: E731
                                                        bufs[2].data_ptr(), bufs[2].data_ptr(), ws.data_ptr(), None))
        torch.cuda.synchronize()
        for _ in range(10):
            call()
        stream.synchronize()
        t0 = time.perf_counter()
        for _ in range(REPS):
            call()
        per_call[r] = (time.perf_counter() - t0) / REPS * 1e6
        stream.synchronize()
        rp.close()

    try:
        cmp.run_ranks(nranks, body)
    finally:
        world.close()
    return {"layout": name, "nranks": nranks, "algorithm": described[0]["algorithm"], "host_us_per_call_median": round(statistics.median(per_call), 1),
            "host_us_per_call_max": round(max(per_call), 1), "transfers": sum(len(d["sends"]) + len(d["recvs"]) for d in described),
            "copy_launches": sum(copy_launches(d) for d in described), "contractions": sum(1 for d in described if d["compute"])}


def main():
    import torch
    from cudalibrarysamples_amd import cutensor as ct
    from cudalibrarysamples_amd import cutensormp as cmp
    from tests import mp_plan_cases as pc
    label = {"tree": sys.argv[1]} if len(sys.argv) > 1 else {}
    if len(sys.argv) > 2:
        label["run"] = int(sys.argv[2])
    for case in pc.GPU_CASES:
        if case[0] in LAYOUTS:
            print(json.dumps(dict(measure(cmp, ct, torch, pc, case), **label)), flush=True)


if __name__ == "__main__":
    main()
