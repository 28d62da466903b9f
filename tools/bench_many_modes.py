#!/usr/bin/env python3
"""What the mode-table kernels (kernels/elementwise_table.hip) move: permutations and a reduction of 2 x 2 x ... x 2 tensors, the shape of
a quantum-circuit state, on fp32 and complex64 data.

    reversal       26 modes, 'ab...z -> z...ba' (a bit reversal of the flat index)
    front3         26 modes, modes f, m and t moved to the front of the others
    shared_lead    26 modes, 'a b ... z -> a z y ... b' (the leading mode shared, the others reversed)
    alt_reduction  24 modes, every other mode summed away

Per workload and data type these variants alternate inside one process (`--rounds` rounds, each timing every variant in turn: `--reps`
launches between two events on the launch stream, after one untimed launch; every plan runs once before the first timed window), so that
drift of the machine lands on all of them alike:

    tiled        the plan as the library makes it (the tile kernel; the reduction: reduce_table_kernel)
    tiled_again  a second, identical plan (tiled against tiled_again is the run-to-run spread)
    gather       the same problem under CUTENSOR_AMD_EW_TABLE=gather (permutations only)
    torch        torch.permute(...) copied into the output / torch.sum on the same buffers ("supported": false where torch refuses the
                 call: its device kernels take a limited number of dimensions that do not coalesce)
    flat_copy    an identity cutensorPermute of a one-mode tensor of the same bytes: code that existed before these kernels, the ceiling

One JSON line per (workload, type, variant): median, minimum and maximum over the rounds of TB/s by ALGORITHMIC bytes (|A| + |D| elements
times the element size), the median milliseconds per call, and `of_flat_copy`: the median rate as a fraction of flat_copy's.

    python tools/bench_many_modes.py --out profiles/many_modes_bandwidth.jsonl
    python tools/bench_many_modes.py --plans-only      # no GPU: the plans and their descriptions"""
import argparse
import json
import os
import string
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("CTAMD_LIB_FLAVOUR", "hooks")       # the gather variant is planned under a switch only the test-hooks libraries read

SWITCH = "CUTENSOR_AMD_EW_TABLE"
VARIANTS = ("tiled", "tiled_again", "gather", "torch", "flat_copy")
M26 = string.ascii_lowercase
M24 = M26[:24]
WORKLOADS = {          # name -> (modes of A, modes of D), fastest first
    "reversal": (M26, M26[::-1]),
    "front3": (M26, "fmt" + "".join(c for c in M26 if c not in "fmt")),
    "shared_lead": (M26, "a" + M26[:0:-1]),
    "alt_reduction": (M24, M24[::2]),
}


def torch_call(torch, x, mA, mD, out):
    """the same movement on the same buffers: x is A's flat buffer (first mode fastest), out D's"""
    dims = [2] * len(mA)
    v = x.view(dims)                                           # dim i holds mode mA[n - 1 - i]
    n = len(mA)
    if len(mD) == n:
        perm = [n - 1 - mA.index(c) for c in reversed(mD)]
        return lambda: out.view(dims).copy_(v.permute(perm))
    red = [n - 1 - mA.index(c) for c in mA if c not in mD]
    kept = [c for c in mA if c in mD]                         # (the workload keeps D's modes in A's order)
    assert "".join(kept) == mD
    return lambda: torch.sum(v, dim=red, out=out.view([2] * len(mD)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--types", default="f32,c64")
    ap.add_argument("--reps", type=int, default=3, help="launches per timed window")
    ap.add_argument("--rounds", type=int, default=5, help="times every variant is visited")
    ap.add_argument("--out", default="", help="append the JSON lines to this file as well")
    ap.add_argument("--label", default="", help="free text copied into every line (which library was measured)")
    ap.add_argument("--plans-only", action="store_true", help="make the plans and print their descriptions; needs no GPU")
    args = ap.parse_args()
    from cudalibrarysamples_amd import ops, cutensor as ct
    h = ops.Handle()
    lines = []
    types = {"f32": (ct.R_32F, 4), "c64": (ct.C_32F, 8)}

    def emit(line):
        line = dict(line, label=args.label)
        lines.append(line)
        print(json.dumps(line), flush=True)

    if not args.plans_only:
        import torch
        tdt = {"f32": torch.float32, "c64": torch.complex64}
        stream = torch.cuda.current_stream().cuda_stream

    def make(mA, mD, dt, gather=False):
        old = os.environ.pop(SWITCH, None)
        if gather:
            os.environ[SWITCH] = "gather"
        try:
            if len(mD) == len(mA):
                return ops.permutation_plan(h, [2] * len(mA), mA, [2] * len(mD), mD, dtype=dt)
            return ops.reduction_plan(h, [2] * len(mA), mA, [2] * len(mD), mD, dtype=dt, workspace_limit=1 << 28)
        finally:
            os.environ.pop(SWITCH, None)
            if old is not None:
                os.environ[SWITCH] = old

    for name in args.workloads.split(","):
        mA, mD = WORKLOADS[name]
        reduction = len(mD) != len(mA)
        nA, nD = 1 << len(mA), 1 << len(mD)
        for t in args.types.split(","):
            dt, size = types[t]
            nbytes = float(nA + nD) * size
            ps = {"tiled": make(mA, mD, dt), "tiled_again": make(mA, mD, dt), "gather": None if reduction else make(mA, mD, dt, gather=True),
                  "flat_copy": ops.permutation_plan(h, [(nA + nD) // 2], "a", [(nA + nD) // 2], "a", dtype=dt)}
            key = {"workload": name, "type": t, "modesA": mA, "modesD": mD, "bytes": nbytes}
            if args.plans_only:
                for v, p in ps.items():
                    if p is not None:
                        emit(dict(key, variant=v, plan=p.describe()))
                        p.destroy()
                continue
            x = torch.randn(nA, device="cuda", dtype=torch.float32).to(tdt[t]) if t == "f32" else torch.view_as_complex(torch.randn(nA, 2, device="cuda"))
            out = torch.empty(nD, device="cuda", dtype=tdt[t])
            flat_in = torch.randn((nA + nD) // 2 * (2 if t == "c64" else 1), device="cuda")
            flat_out = torch.empty_like(flat_in)
            ws = torch.empty(max(ps["tiled"].required_workspace, 256), dtype=torch.uint8, device="cuda")

            def lib(p):
                if reduction:
                    return lambda: p.reduce(1.0, x.data_ptr(), 0.0, out.data_ptr(), out.data_ptr(), ws.data_ptr(), p.required_workspace, stream)
                return lambda: p.permute(1.0, x.data_ptr(), out.data_ptr(), stream)
            run = {"tiled": lib(ps["tiled"]), "tiled_again": lib(ps["tiled_again"]), "gather": lib(ps["gather"]) if ps["gather"] else None,
                   "torch": torch_call(torch, x, mA, mD, out),
                   "flat_copy": lambda: ps["flat_copy"].permute(1.0, flat_in.data_ptr(), flat_out.data_ptr(), stream)}
            # the library's result against torch's, once, on the buffers that are timed (a reduction: fp32 sums in another order).  torch's
            # device copy and reduction kernels take a limited number of dimensions after coalescing: where it refuses the call, say so
            ok, torch_error = None, None
            try:
                run["torch"]()
                torch.cuda.synchronize()
                want = out.clone()
                out.zero_()
                run["tiled"]()
                torch.cuda.synchronize()
                ok = bool(torch.allclose(torch.view_as_real(out) if t == "c64" else out, torch.view_as_real(want) if t == "c64" else want,
                                         rtol=1e-4 if reduction else 0.0, atol=1e-2 if reduction else 0.0))
            except RuntimeError as err:
                torch_error = str(err).splitlines()[0][:200]
                run["torch"] = None
                emit(dict(key, variant="torch", supported=False, error=torch_error))
            ms = {v: [] for v in VARIANTS}
            for v in VARIANTS:                                 # every code object loaded, every variant run once, before the first timed window
                if run[v] is not None:
                    run[v]()
            torch.cuda.synchronize()
            for _ in range(args.rounds):
                for v in VARIANTS:
                    if run[v] is None:
                        continue
                    run[v]()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.reps):
                        run[v]()
                    e1.record()
                    torch.cuda.synchronize()
                    ms[v].append(e0.elapsed_time(e1) / args.reps)
            tb = lambda m: nbytes / (m * 1e-3) / 1e12   # noqa: E731
            med = {v: sorted(ms[v])[len(ms[v]) // 2] for v in VARIANTS if ms[v]}
            for v in VARIANTS:
                if run[v] is None:
                    continue
                s = sorted(ms[v])
                emit(dict(key, variant=v, matches_torch=ok, TBps_median=tb(med[v]), TBps_min=tb(s[-1]), TBps_max=tb(s[0]), ms_median=med[v],
                          ms_min=s[0], ms_max=s[-1], of_flat_copy=med["flat_copy"] / med[v], rounds=args.rounds, reps=args.reps,
                          plan=ps[v].describe() if v in ps and ps[v] is not None else None))
            for p in ps.values():
                if p is not None:
                    p.destroy()
            del x, out, flat_in, flat_out, ws
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
