"""One table of plan-only cuTENSORMp contraction cases: the layouts the tests of the multi-rank path plan or run (tests/test_mp_plan_cpu.py,
tests/test_gpu_mp.py), each with its world size, rank permutations, the algorithm it is forced to, its data type, element strides,
block sizes and device-workspace limit.  The layout builders live here and the tests import them; tools/gen_mp_plan_descriptions.py
describes every case of CASES, for every rank, into tests/golden/mp_plan_descriptions.json.gz and
tests/test_mp_plan_descriptions_cpu.py compares every later library with that file.

A case is planned on plan-only handles (no GPU visible) of a local world, one rank after the other.  `describe_raw` returns
ctamdMpDescribePlan's text per rank as the library wrote it, or, for a plan the library refuses, the JSON object {"status": <cutensorStatus_t>}."""
import collections
import contextlib
import ctypes
import os

import numpy as np

# eq 'ab,bc->ac' (first listed mode is the fastest); ext {label: extent}; dist = three dicts {label: ranks along that mode} for A, B, C;
# ranks = optional cell -> rank permutations per tensor; algo = CUTENSORMP_AMD_ALGO or None; pad = elements added to the first mode's block
# in the element strides of A, B and C (0: packed, passed as NULL); block = {label: block size} where it is not ceil(extent / ranks)
Case = collections.namedtuple("Case", "id eq ext dist nranks ranks algo dtype pad block dev_limit")

DEFAULT_LIMIT = 1 << 30

# name -> (cutensorDataType_t, compute descriptor)
DTYPES = {"f32": (0, "32F"), "f64": (1, "64F"), "c64": (4, "32F"), "c128": (5, "64F"), "bf16": (14, "32F")}

MANY_MODES = "abcdefEFGH,abcdefABCD->EFGHABCD"

# the layouts of tests/test_mp_plan_cpu.py: eq, extents, (distA, distB, distC), nranks, rank permutations
PLAN_CASES = [
    ("mk,kn->mn", dict(m=96, k=80, n=64), ({"m": 2}, {}, {"m": 2}), 2, None),
    ("mk,kn->mn", dict(m=100, k=72, n=52), ({"m": 2, "k": 2}, {"k": 2, "n": 2}, {"m": 2, "n": 2}), 4, None),
    ("mk,kn->mn", dict(m=64, k=64, n=64), ({"k": 4}, {"n": 4}, {"m": 2, "n": 2}), 4, None),
    ("akcl,lbk->abc", dict(a=30, b=21, c=9, k=16, l=12), ({"c": 3}, {"b": 3}, {"a": 3}), 3, None),
    ("mk,kn->mn", dict(m=5, k=16, n=8), ({"m": 8}, {}, {"m": 8}), 8, None),
    ("mkl,lkn->mn", dict(m=50, k=12, l=10, n=27), ({"k": 2, "l": 2}, {"l": 2, "k": 2}, {"m": 2, "n": 2}), 4, [None, [0, 2, 1, 3], None]),
    (MANY_MODES, {l: 2 for l in "abcdefEFGHABCD"}, ({"E": 2, "F": 2, "G": 2}, {"a": 2, "b": 2, "c": 2}, {"A": 2, "B": 2, "C": 2}), 8, None),
]

HEADLINE_EXT = dict(a=96, b=64, c=64, d=64, e=96)
HEADLINE_8 = ("dcba,ebcd->ea", HEADLINE_EXT, ({"b": 8}, {"b": 8}, {}), 8, None)

# the cases of tests/test_gpu_mp.py: name, eq, extents, (distA, distB, distC), nranks, dtype, alpha, beta[, rank permutations]
GPU_CASES = [
    ("row-sharded, B replicated: no exchange", "mk,kn->mn", dict(m=96, k=80, n=64), ({"m": 2}, {}, {"m": 2}), 2, "f32", 1.0, 0.0),
    ("2x2 grids, ragged blocks", "mk,kn->mn", dict(m=100, k=72, n=52), ({"m": 2, "k": 2}, {"k": 2, "n": 2}, {"m": 2, "n": 2}), 4, "f32", 1.1, 0.0),
    ("k distributed, C replicated", "mk,kn->mn", dict(m=48, k=128, n=40), ({"k": 4}, {"k": 4}, {}), 4, "f32", 1.0, 0.0),
    ("k distributed, C sharded, beta", "mk,kn->mn", dict(m=64, k=96, n=48), ({"k": 2}, {"k": 2}, {"n": 2}), 2, "f32", 0.7, 0.5),
    ("three ranks, multi-mode", "akcl,lbk->abc", dict(a=30, b=21, c=9, k=16, l=12), ({"c": 3}, {"b": 3}, {"a": 3}), 3, "f32", 1.0, 0.5),
    ("sub-box transfers", "mk,kn->mn", dict(m=64, k=64, n=64), ({"k": 4}, {"n": 4}, {"m": 2, "n": 2}), 4, "f32", 1.0, 0.0),
    ("fp64", "mk,kn->mn", dict(m=40, k=56, n=24), ({"m": 2}, {"n": 2}, {"m": 2}), 2, "f64", 1.0, 0.25),
    ("bf16", "mk,kn->mn", dict(m=128, k=256, n=128), ({"k": 2}, {"n": 2}, {"m": 2}), 2, "bf16", 1.0, 0.0),
    ("more ranks than blocks along a mode", "mk,kn->mn", dict(m=5, k=16, n=8), ({"m": 4}, {}, {"m": 4}), 4, "f32", 1.0, 0.0),
]

GPU_REDUCE_CASES = [
    ("C replicated: all-reduce in the user's D", "mk,kn->mn", dict(m=48, k=128, n=40), ({"k": 4}, {"k": 4}, {}), 4, "f32", 1.0, 0.5),
    ("C cut along its last mode: slots are slabs", "mk,kn->mn", dict(m=64, k=96, n=48), ({"k": 2}, {"k": 2}, {"n": 2}), 2, "f32", 0.7, 0.5),
    ("C cut along its first mode: packed slots", "mk,kn->mn", dict(m=64, k=96, n=48), ({"k": 2}, {"k": 2}, {"m": 2}), 2, "f32", 1.0, 0.0),
    ("ragged 2x2 grid of C, two contracted modes cut", "mkl,lkn->mn", dict(m=50, k=12, l=10, n=27), ({"k": 2, "l": 2}, {"l": 2, "k": 2}, {"m": 2, "n": 2}), 4, "f32", 1.0, 0.25,
     [None, [0, 2, 1, 3], None]),   # B's grid is (l, k): this rank order gives every rank the same (k, l) block of A and B
    ("the headline einsum, shrunk, K cut over four ranks", "dcba,ebcd->ea", dict(a=24, b=16, c=8, d=16, e=24), ({"b": 4}, {"b": 4}, {}), 4, "f32", 1.0, 0.0),
    ("complex", "mk,kn->mn", dict(m=20, k=64, n=12), ({"k": 2}, {"k": 2}, {"n": 2}), 2, "c64", 1.0, 0.5),
    ("bf16", "mk,kn->mn", dict(m=128, k=512, n=64), ({"k": 2}, {"k": 2}, {}), 2, "bf16", 1.0, 0.0),
    ("fp64, three ranks, one with an empty block of C", "mk,kn->mn", dict(m=4, k=90, n=16), ({"k": 3}, {"k": 3}, {"m": 3}), 3, "f64", 1.0, 0.5),
]

# Element strides that are not the packed layout of the block (the first mode's block padded by PAD elements): the `packed == false`
# branches of the planner — no whole-block sends, no reduce-scatter straight into D, no all-reduce in the user's D.
PAD = 3
PADDED_EXT = dict(m=24, k=32, n=16)
PADDED_GATHER = ("mk,kn->mn", PADDED_EXT, ({"k": 2}, {"n": 2}, {"m": 2}), 2)
PADDED_REDUCE_REPLICATED = ("mk,kn->mn", PADDED_EXT, ({"k": 2}, {"k": 2}, {}), 2)
PADDED_REDUCE_CUT_N = ("mk,kn->mn", PADDED_EXT, ({"k": 2}, {"k": 2}, {"n": 2}), 2)

# A copy of more than one launch.  The element-wise planner takes a view of two tiled modes and kMaxGroupModes = 4 others after fusion;
# a mode fuses with its neighbour unless the box is narrower than the block there.  Packed blocks narrower than their box in seven modes
# need either 2^7 ranks or, as here, blocks declared one element larger than the extent (blockSize 5 over extent 4 on one rank per mode):
# the valid part [0, 4) of every such mode is strided 5 in the user's block and 4 in the send region and the staging tensor.  A is cut
# along k and every rank needs all of it: the pack of the half it sends and the local copy of the half it keeps peel.
PEELED_EQ = "abcdefgk,kn->abcdefgn"
PEELED_EXT = dict(a=4, b=4, c=4, d=4, e=4, f=4, g=4, k=4, n=4)
PEELED_BLOCK = {l: 5 for l in "abcdefg"}
PEELED = (PEELED_EQ, PEELED_EXT, ({"k": 2}, {}, {"n": 2}), 2)


def _case(id, layout, algo=None, dtype="f32", pad=0, block=None, dev_limit=DEFAULT_LIMIT):
    eq, ext, dist, nranks = layout[:4]
    ranks = layout[4] if len(layout) > 4 else None
    return Case(id, eq, dict(ext), tuple(dict(d) for d in dist), nranks, ranks, algo, dtype, pad, dict(block or {}), dev_limit)


def _gpu_layout(c):
    return (c[1], c[2], c[3], c[4], c[8] if len(c) > 8 else None)


def _cases():
    for i, c in enumerate(PLAN_CASES):
        for algo in (None, "gather", "reduce"):
            yield _case("plan%d-%s" % (i, algo or "auto"), c, algo=algo)
    for i, c in enumerate(GPU_CASES):
        yield _case("gpu%d-%s" % (i, c[5]), _gpu_layout(c), dtype=c[5])
    for i, c in enumerate(GPU_REDUCE_CASES):
        for algo in ("reduce", "gather"):
            yield _case("gpu_reduce%d-%s-%s" % (i, c[5], algo), _gpu_layout(c), algo=algo, dtype=c[5])
    yield _case("headline-k8", HEADLINE_8)
    yield _case("many_modes-c64-n2", (MANY_MODES, {l: 2 for l in "abcdefEFGHABCD"}, ({"E": 2}, {"a": 2}, {"A": 2}), 2, [None, None, [1, 0]]), dtype="c64")
    # data types: two gather and two reduce shapes each
    for dt in DTYPES:
        yield _case("dtype-%s-gather-subbox" % dt, _gpu_layout(GPU_CASES[5]), algo="gather", dtype=dt)
        yield _case("dtype-%s-gather-kn" % dt, _gpu_layout(GPU_CASES[6]), algo="gather", dtype=dt)
        yield _case("dtype-%s-reduce-replicated" % dt, _gpu_layout(GPU_REDUCE_CASES[0]), algo="reduce", dtype=dt)
        yield _case("dtype-%s-reduce-cut_n" % dt, _gpu_layout(GPU_REDUCE_CASES[1]), algo="reduce", dtype=dt)
    # element strides that are not packed
    yield _case("padded-gather", PADDED_GATHER, pad=PAD)
    for algo in ("reduce", "gather"):
        yield _case("padded-replicated-%s" % algo, PADDED_REDUCE_REPLICATED, algo=algo, pad=PAD)
        yield _case("padded-cut_n-%s" % algo, PADDED_REDUCE_CUT_N, algo=algo, pad=PAD)
    yield _case("padded-ragged-2x2-reduce", _gpu_layout(GPU_REDUCE_CASES[3]), algo="reduce", pad=PAD)
    yield _case("padded-subbox-gather", _gpu_layout(GPU_CASES[5]), pad=PAD)
    # copies of more than one launch
    yield _case("peeled-gather", PEELED, block=PEELED_BLOCK)
    yield _case("peeled-gather-c64", PEELED, block=PEELED_BLOCK, dtype="c64")
    # device limits: refusals, and limits under which the contraction's workspace is what the fixed regions leave
    yield _case("limit-subbox-1k", _gpu_layout(GPU_CASES[5]), dev_limit=1024)
    yield _case("limit-subbox-fixed-only", _gpu_layout(GPU_CASES[5]), dev_limit=32768)       # send + recv + stage exactly
    yield _case("limit-cut_n-reduce-1k", _gpu_layout(GPU_REDUCE_CASES[1]), algo="reduce", dev_limit=1024)
    # the headline einsum asks for split-K workspace: K cut over two ranks (reduce; the local world's all-reduce scratch is the fixed
    # part) and a free mode cut over two ranks (gather, nothing fixed)
    for extra in (0, 1 << 20, DEFAULT_LIMIT):
        yield _case("limit-headline-k2-reduce-scratch+%d" % extra, ("dcba,ebcd->ea", HEADLINE_EXT, ({"b": 2}, {"b": 2}, {}), 2), dev_limit=96 * 96 * 4 + extra)
    for limit in (0, 1 << 16, 1 << 20):
        yield _case("limit-headline-a2-gather-%d" % limit, ("dcba,ebcd->ea", HEADLINE_EXT, ({"a": 2}, {}, {"a": 2}), 2), dev_limit=limit)


CASES = list(_cases())
assert len({c.id for c in CASES}) == len(CASES)


def split_modes(eq):
    lhs, mc = eq.split("->")
    ma, mb = lhs.split(",")
    return [ma, mb, mc]


def grid(eq, dist):
    """ranks along every mode of A, B, C"""
    modes = split_modes(eq)
    return [[dist[k].get(l, 1) for l in modes[k]] for k in range(3)]


def block_sizes(ext, modes, p, block=None):
    return [(block or {}).get(l, -(-ext[l] // n)) for l, n in zip(modes, p)]


def element_strides(bs, pad):
    """the block's layout, first mode fastest, the first mode's block padded by `pad` elements"""
    out, run = [], 1
    for i, b in enumerate(bs):
        out.append(run)
        run *= b + (pad if i == 0 else 0)
    return out


@contextlib.contextmanager
def algo_environment(algo):
    """The process environment with CUTENSORMP_AMD_ALGO set to `algo`, or unset (plans read it at plan creation)."""
    saved = os.environ.pop("CUTENSORMP_AMD_ALGO", None)
    if algo:
        os.environ["CUTENSORMP_AMD_ALGO"] = algo
    try:
        yield
    finally:
        os.environ.pop("CUTENSORMP_AMD_ALGO", None)
        if saved is not None:
            os.environ["CUTENSORMP_AMD_ALGO"] = saved


class RankPlan:
    """Handle, descriptors, contraction, preference and plan of one rank of a local world; `status` is cutensorMpCreatePlan's."""

    def __init__(self, cmp_ct, world, r, eq, ext, dist, nranks, dtype=None, compute=None, ranks=None, pad=0, block=None, dev_limit=DEFAULT_LIMIT,
                 device=0, stream=None):
        cmp, ct = cmp_ct
        self.cmp = cmp
        modes = split_modes(eq)
        P = grid(eq, dist)
        perm = ranks or [None, None, None]
        self.h = ctypes.c_void_p()
        cmp.check(cmp.ctamdMpCreateOnLocalWorld(ctypes.byref(self.h), world.ptr, r, device, stream))
        self.descs = []
        for k in range(3):
            d = ctypes.c_void_p()
            pr = None if perm[k] is None or int(np.prod(P[k])) == 1 else ct.i32(perm[k])
            bs = block_sizes(ext, modes[k], P[k], block)
            cmp.check(cmp.cutensorMpCreateTensorDescriptor(self.h, ctypes.byref(d), len(modes[k]), ct.i64([ext[l] for l in modes[k]]),
                                                           ct.i64(element_strides(bs, pad)) if pad else None, ct.i64(bs) if block else None, None,
                                                           ct.i64(P[k]), nranks, pr, ct.R_32F if dtype is None else dtype))
            self.descs.append(d)
        lab = [ct.i32([ord(c) for c in m]) for m in modes]
        self.op, self.pref, self.plan = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        cmp.check(cmp.cutensorMpCreateContraction(self.h, ctypes.byref(self.op), self.descs[0], lab[0], ct.OP_IDENTITY, self.descs[1], lab[1], ct.OP_IDENTITY,
                                                  self.descs[2], lab[2], ct.OP_IDENTITY, self.descs[2], lab[2], compute or ct.compute_desc("32F")))
        cmp.check(cmp.cutensorMpCreatePlanPreference(self.h, ctypes.byref(self.pref), cmp.ALGO_DEFAULT, dev_limit, 0))
        self.status = cmp.cutensorMpCreatePlan(self.h, ctypes.byref(self.plan), self.op, self.pref)

    def required_device(self):
        need = ctypes.c_uint64(0)
        self.cmp.check(self.cmp.cutensorMpPlanGetAttribute(self.h, self.plan, self.cmp.PLAN_REQUIRED_WORKSPACE_DEVICE, ctypes.byref(need), 8))
        return need.value

    def close(self):
        cmp = self.cmp
        cmp.check(cmp.cutensorMpDestroyPlan(self.plan))
        cmp.check(cmp.cutensorMpDestroyPlanPreference(self.pref))
        cmp.check(cmp.cutensorMpDestroyOperationDescriptor(self.op))
        for x in self.descs:
            cmp.check(cmp.cutensorMpDestroyTensorDescriptor(x))
        cmp.check(cmp.cutensorMpDestroy(self.h))


def plans_of_all_ranks(cmp_ct, eq, ext, dist, nranks, dtype=None, ranks=None, algo=None, monkeypatch=None):
    """ctamdMpDescribePlan (parsed) of every rank's plan, built one after the other on plan-only handles"""
    cmp, ct = cmp_ct
    if monkeypatch is not None:
        if algo:
            monkeypatch.setenv("CUTENSORMP_AMD_ALGO", algo)
        else:
            monkeypatch.delenv("CUTENSORMP_AMD_ALGO", raising=False)
    world = cmp.LocalWorld(nranks)
    out = []
    try:
        for r in range(nranks):
            rp = RankPlan(cmp_ct, world, r, eq, ext, dist, nranks, dtype=dtype, ranks=ranks)
            cmp.check(rp.status)
            d = cmp.describe_plan(rp.plan)
            assert d["requiredDevice"] == rp.required_device() and d["rank"] == r and d["nranks"] == nranks
            # executing on a plan-only handle is refused, not crashed
            one = ctypes.c_float(1.0)
            buf = (ctypes.c_char * 64)()
            st = cmp.cutensorMpContract(rp.h, rp.plan, ctypes.byref(one), buf, buf, ctypes.byref(one), buf, buf, buf, None)
            assert st != 0
            out.append(d)
            rp.close()
    finally:
        world.close()
    return out


def check_lists_fit(plans):
    n = len(plans)
    assert len({p["algorithm"] for p in plans}) == 1
    assert len({(p["gatherTotal"], p["reduceTotal"]) for p in plans}) == 1
    for s in range(n):
        for q in range(n):
            sent = [(t["tensor"], t["bytes"]) for t in plans[s]["sends"] if t["dst"] == q]
            expected = [(t["tensor"], t["bytes"]) for t in plans[q]["recvs"] if t["src"] == s]
            assert sent == expected, (s, q, sent, expected)
            assert all(t["src"] == s for t in plans[s]["sends"]) and all(t["dst"] == q for t in plans[q]["recvs"])
    if plans[0]["algorithm"] == "gather":
        assert sum(t["bytes"] for p in plans for t in p["recvs"]) == plans[0]["gatherTotal"]
    else:
        assert all(p["sends"] == [] and p["recvs"] == [] for p in plans)


def describe_raw(cmp_ct, case):
    """{"<case id>/r<rank>": ctamdMpDescribePlan's text of that rank's plan, or {"status":N} for a plan the library refuses}"""
    cmp, ct = cmp_ct
    dtype, compute = DTYPES[case.dtype]
    out = {}
    with algo_environment(case.algo):
        world = cmp.LocalWorld(case.nranks)
        try:
            for r in range(case.nranks):
                rp = RankPlan(cmp_ct, world, r, case.eq, case.ext, case.dist, case.nranks, dtype=dtype, compute=ct.compute_desc(compute),
                              ranks=case.ranks, pad=case.pad, block=case.block, dev_limit=case.dev_limit)
                out["%s/r%d" % (case.id, r)] = cmp.describe_plan_raw(rp.plan) if rp.status == 0 else '{"status":%d}' % rp.status
                rp.close()
        finally:
            world.close()
    return out
