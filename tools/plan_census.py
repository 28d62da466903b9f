#!/usr/bin/env python3
"""Plan census: what the planner answers, one line per problem, for comparing two builds of the library byte for byte.

    python tools/plan_census.py > census.txt        # needs no GPU: plan-only handles, the test-hooks flavour of the library

Per problem: the three workspace estimates (MIN / DEFAULT / MAX, each with the plan made AT the estimate) and, for each workspace limit
in {0, 1 000 003}, the status of cutensorCreatePlan, the plan's required workspace and the raw ctamdDescribePlan string; the GEMM grid
of the 16-bit and fp32 types repeats that for algo = 0 .. 11.  Problems: every case of tests/workspace_cases.py and of
tests/exact_cases.py (planned through those modules' own helpers) and a grid of GEMM-like shapes.  Cases whose switch the library reads
once per process are planned in child processes started with the switch set, and the whole census is repeated under each value of
CUTENSOR_AMD_H16_WAVES that tests/test_h16_planner_cpu.py drives.  Nothing printed depends on time, addresses or the order in which
the children finish.  A planner change that is meant to change nothing leaves the output — `sha256sum` of it — as it was."""
import argparse
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
os.environ["CTAMD_LIB_FLAVOUR"] = "hooks"
for p in (TESTS, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

WAVES = ("8", "4", "4v", "4x", "s", "4m", "4m4", "8m", "4q", "4p")      # tests/test_h16_planner_cpu.py
GRID_DTYPES = ("bfloat16", "float16", "float32", "float64", "complex64")
GRID_LAYOUTS = (("km", "kn"), ("mk", "kn"), ("mk", "nk"), ("km", "nk"))
GRID_SIZES = (50, 96, 1000, 2048, 4100, 8192)
GRID_K = (64, 200, 4096, 65536)
GRID_ALGOS = range(12)
BIG_LIMIT = 1000003


def modules():
    import exact_cases as xc
    import guarded as gd
    import workspace_cases as wc
    from cudalibrarysamples_amd import cutensor as ct, ops
    return ct, ops, wc, xc, gd


def exact_contraction_plan(ct, ops, gd, xc, h, case, **kw):
    """tests/exact_cases.py _plan with the census' own plan keywords"""
    e, m = case.extents, case.modes
    if case.algo is not None:
        kw.setdefault("algo", case.algo)
    st = [gd.packed_strides(e(m[i]), case.pad[i]) for i in range(3)]
    conj = [ct.OP_CONJ if c else ct.OP_IDENTITY for c in (case.conjA, case.conjB, case.conjC)]
    return ops.contraction_plan(h, e(m[0]), m[0], e(m[1]), m[1], e(m[2]), m[2], dtype=xc._dt(ct, case.dtype), strideA=st[0], strideB=st[1],
                                strideC=st[2], alignment=case.align or 128, opA=conj[0], opB=conj[1], opC=conj[2], **kw)


def answers(ct, wc, make, **kw):
    """'est ...' and 'limit ...' fields of one problem; make(**plan keywords) -> ops.Plan or raises ct.CuTensorError"""
    def one(tag, **plan_kw):
        try:
            p = make(**dict(kw, **plan_kw))
        except ct.CuTensorError as err:
            return "%s:status=%d" % (tag, err.status)
        try:
            return "%s:est=%d:status=0:req=%d:%s" % (tag, p.workspace_estimate, p.required_workspace, wc.describe(ct, p).raw)
        finally:
            p.destroy()
    out = [one(name, workspace_pref=pref, workspace_limit=None)
           for name, pref in (("MIN", ct.WORKSPACE_MIN), ("DEFAULT", ct.WORKSPACE_DEFAULT), ("MAX", ct.WORKSPACE_MAX))]
    out += [one("L%d" % limit, workspace_limit=limit) for limit in (0, BIG_LIMIT)]
    return out


def census_cases(table, ids):
    ct, ops, wc, xc, gd = modules()
    cases = {c.id: c for c in (wc.CASES if table == "workspace" else xc.CASES)}
    for cid in ids:
        case = cases[cid]
        h = ops.Handle()
        if table == "exact" and case.kind == "contraction":
            def make(**kw):
                with wc.hook_env(case):
                    return exact_contraction_plan(ct, ops, gd, xc, h, case, **kw)
        else:
            def make(**kw):
                return wc.make_plan(ct, ops, h, case, **kw)
        print("\t".join(["%s/%s" % (table, cid)] + answers(ct, wc, make)), flush=True)
        h.close()


def census_grid(dtype):
    ct, ops, wc, xc, gd = modules()
    for mA, mB in GRID_LAYOUTS:
        for size in GRID_SIZES:
            for k in GRID_K:
                case = wc.Case("grid", "contraction", dtype, dict(m=size, n=size, k=k), (mA, mB, "mn"), None, pad=0)
                h = ops.Handle()
                make = lambda **kw: wc.make_plan(ct, ops, h, case, **kw)
                name = "grid/%s/%s,%s/%d/%d" % (dtype, mA, mB, size, k)
                print("\t".join([name] + answers(ct, wc, make)), flush=True)
                if dtype in ("bfloat16", "float16", "float32"):
                    for algo in GRID_ALGOS:
                        print("\t".join(["%s/algo%d" % (name, algo)] + answers(ct, wc, make, algo=algo)), flush=True)
                h.close()


def jobs():
    """(arguments of a child, its environment switches), in the order of the output"""
    ct, ops, wc, xc, gd = modules()
    out = []
    for table, cases in (("workspace", wc.CASES), ("exact", xc.CASES)):
        groups = []
        for c in cases:     # consecutive cases with the same switches share a child
            env = tuple(sorted(c.env.items()))
            if not groups or groups[-1][0] != env or len(groups[-1][1]) >= 40:
                groups.append((env, []))
            groups[-1][1].append(c.id)
        out += [(["cases", table] + ids, dict(env)) for env, ids in groups]
    out += [(["grid", dt], {}) for dt in GRID_DTYPES]
    return out


def run_child(args, env):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, env=dict(os.environ, **env), cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit("plan_census child %s failed (%d):\n%s" % (args[:3], r.returncode, r.stderr[-4000:]))
    return r.stdout


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("child", nargs="*", help=argparse.SUPPRESS)
    ap.add_argument("--jobs", type=int, default=8, help="child processes at a time")
    ap.add_argument("--no-waves", action="store_true", help="skip the repetitions under CUTENSOR_AMD_H16_WAVES")
    a = ap.parse_args()
    if a.child and a.child[0] == "cases":
        return census_cases(a.child[1], a.child[2:])
    if a.child and a.child[0] == "grid":
        return census_grid(a.child[1])
    todo = [("", args, env) for args, env in jobs()]
    if not a.no_waves:
        todo += [(w, args, dict(env, CUTENSOR_AMD_H16_WAVES=w)) for w in WAVES for args, env in jobs()]
    with ThreadPoolExecutor(max_workers=a.jobs) as pool:
        results = list(pool.map(lambda t: run_child(t[1], t[2]), todo))
    for (waves, args, env), text in zip(todo, results):
        print("# H16_WAVES=%s %s %s" % (waves or "-", " ".join(args[:2]), json.dumps(env, sort_keys=True)))
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
