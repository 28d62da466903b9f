"""The case table of the workspace contract (tests/test_workspace_contract_cpu.py plans every case, tests/test_gpu_workspace_contract.py
runs every case) — a helper module, not a conftest.

One case per path that takes scratch memory from the caller's workspace (split-K partials of every contraction family, the temporaries
of the two-step plans: copied operands, lone-mode reductions, the trinary contraction's intermediate; split-reduction partials) and the
element-wise plans that must take none.  Each case reaches its path the way the family tests do (the hooks-flavour switches where
needed) and names the path in `expect`, a predicate on the plan's description: a planner change that moves a case off the path it
covers fails the case instead of silently testing something else."""
import ctypes
import json
import os
from contextlib import contextmanager

import guarded as gd

class Desc:
    """ctamdDescribePlan's JSON with every key kept: a nested two-step plan repeats the lone / repack keys of its inner plan"""

    def __init__(self, raw):
        self.raw = raw
        self.pairs = json.loads(raw, object_pairs_hook=lambda kv: kv) if raw else []

    def all(self, key):
        return [v for k, v in self.pairs if k == key]

    def get(self, key, default=None):
        v = self.all(key)
        return v[0] if v else default

    def any(self, key, value=1):
        return value in self.all(key)

    def __repr__(self):
        return self.raw


def describe(ct, plan):
    buf = ctypes.create_string_buffer(4096)
    n = ct.lib.ctamdDescribePlan(plan.plan, buf, 4096)
    return Desc(buf.value.decode() if n > 0 else "")


class Case:
    def __init__(self, id, kind, dtype, ext, modes, expect, env=None, pad=3, c_pad=None, betas=(0.0, 0.7), alpha=1.25, lo=-1.0, hi=1.0,
                 gpu_expect=None, blocks=None, fresh=False):
        self.id, self.kind, self.dtype, self.ext, self.modes = id, kind, dtype, ext, modes
        self.expect, self.env, self.pad = expect, dict(env or {}), pad
        self.c_pad = pad if c_pad is None else c_pad
        self.betas, self.alpha, self.lo, self.hi = betas, alpha, lo, hi
        self.gpu_expect = gpu_expect or (lambda d: True)     # what only a plan made with a device shows
        self.fresh = fresh       # the library reads the case's switch once per process: the case runs in a child started with it set
        self.blocks = blocks                                 # block-sparse: (coordinates of A's, B's, C's blocks); ext = sections per mode

    def __repr__(self):
        return self.id

    def extents(self, m):
        return [sum(self.ext[c]) if self.blocks else self.ext[c] for c in m]


class BlockLayout:
    """a block-sparse tensor's blocks as slices of the dense tensor (modes in descriptor order)"""

    def __init__(self, sections, modes, coords):
        self.modes, self.coords = modes, coords
        starts = {m: [sum(sections[m][:i]) for i in range(len(sections[m]) + 1)] for m in modes}
        self.slices = [tuple(slice(starts[m][ci], starts[m][ci + 1]) for m, ci in zip(modes, c)) for c in coords]
        self.shapes = [[sl.stop - sl.start for sl in s] for s in self.slices]

    def dense(self, blocks, dense_ext):
        import torch
        out = torch.zeros(dense_ext, dtype=blocks[0].dtype)
        for sl, b in zip(self.slices, blocks):
            out[sl] = b
        return out


class GuardedBlocks:
    """every block of a block-sparse D (or C) in a NaN guard of its own (tests/guarded.py)"""

    def __init__(self, layout, dtype_name):
        self.layout = layout
        self.t = [gd.guarded_tensor(shape, dtype_name) for shape in layout.shapes]
        self.ptrs = (ctypes.c_void_p * len(self.t))(*[t.ptr for t in self.t])

    def set(self, dense):
        for sl, t in zip(self.layout.slices, self.t):
            t.set(dense[sl])

    def get(self):
        return torch_cat([t.get().reshape(-1) for t in self.t])

    def check_guard(self, what=""):
        for i, t in enumerate(self.t):
            t.check_guard("%s block %d" % (what, i))

    def refill_nan(self):
        for t in self.t:
            t.refill_nan()

    def bits(self):
        import numpy as np
        return np.concatenate([t.bits() for t in self.t])


def torch_cat(xs):
    import torch
    return torch.cat(xs)


def _family(f, kname=None, split=None):
    def ok(d):
        if d.get("family") != f or (kname is not None and d.get("kname") != kname):
            return False
        return split is None or (d.get("splitK", 1) > 1) == split
    return ok


def _lone(a, b, inner=lambda d: True):
    return lambda d: d.get("lone_reduce_A") == a and d.get("lone_reduce_B") == b and inner(d)


def _repack(a, b, inner=lambda d: True):
    return lambda d: d.get("repack_A") == a and d.get("repack_B") == b and d.get("lone_reduce_A") == 0 and inner(d)


def _split_reduction(d):
    return d.get("op") == "reduction" and d.get("splitR", 1) > 1


def _elementwise(d):
    return d.get("op") == "elementwise"


REPACK = {"CUTENSOR_AMD_REPACK": "f"}
GEN = {"CUTENSOR_AMD_GEN": "force"}
HEAD = dict(a=48, b=16, c=16, d=16, e=48)                 # the headline 'abcd,dcbe->ae' at a small e
T3 = dict(i=200, l=136, j=16, k=72)                     # 'ijk,lkj->il' of tests/test_gpu_repack.py
LONE = dict(i=20, j=7, k=50, l=21)                      # 'ijk,kl->il' reversed
ODD = dict(m=37, n=29, k=3001)
PEEL = dict(a=4, b=3, c=5, d=2, e=6, p=3, q=4, r=2, s=5, t=3, x=4, y=3, z=2)

CASES = [
    # fp32 GETT: no split, split-K (the headline form at a small e)
    Case("f32_nosplit", "contraction", "float32", dict(m=96, n=80, k=64), ("mk", "kn", "mn"), _family(0, "gett_f32_kernel", False)),
    Case("f32_headline_splitk", "contraction", "float32", HEAD, ("dcba", "ebcd", "ea"), _family(0, "gett_f32_kernel", True)),
    # 16-bit LDS-DMA split-K (aligned, and at odd extents: ragged last K-tile)
    Case("bf16_lds_splitk", "contraction", "bfloat16", dict(m=64, n=64, k=4096), ("km", "kn", "mn"), _family(1, None, True)),
    Case("f16_lds_splitk", "contraction", "float16", dict(m=64, n=64, k=4096), ("km", "kn", "mn"), _family(1, None, True)),
    Case("bf16_lds_splitk_odd", "contraction", "bfloat16", ODD, ("mk", "kn", "mn"), _family(1, None, True)),
    # the general MFMA family with split-K
    Case("bf16_gen_splitk_odd", "contraction", "bfloat16", ODD, ("mk", "kn", "mn"), _family(2, "gett_gen_kernel", True), env=GEN),
    Case("f64_gen_splitk", "contraction", "float64", ODD, ("mk", "kn", "mn"), _family(2, "gett_gen_kernel", True)),
    Case("c64_gen_splitk", "contraction", "complex64", ODD, ("mk", "kn", "mn"), _family(2, "gett_gen_kernel", True), alpha=0.75 + 0.5j),
    Case("c128_gen_splitk", "contraction", "complex128", ODD, ("mk", "kn", "mn"), _family(2, "gett_gen_kernel", True), alpha=0.75 + 0.5j),
    # split-K on the stream kernel, whose partials are whole padded tiles (folded by launch_splitk_reduce_frag)
    Case("f32_stream_splitk", "contraction", "float32", dict(a=128, b=32, c=32, d=64, e=128), ("dcba", "ebcd", "ea"),
         _family(0, "gett_f32_stream_kernel", True)),
    # the persistent 16-bit kernel, beta != 0 with C in D's layout (C joins through the row image)
    Case("bf16_persistent_beta", "contraction", "bfloat16", dict(m=1024, n=1024, k=256), ("mk", "kn", "mn"),
         _family(1, "gett_h16w4p_kernel"), env={"CUTENSOR_AMD_H16_WAVES": "4p"}, pad=0, betas=(0.7, 0.0), fresh=True),
    # operands copied into packed temporaries first (plan_repack)
    Case("f32_repack", "contraction", "float32", T3, ("kji", "jkl", "li"), _repack(0, 1, _family(0)), env=REPACK),
    Case("bf16_repack", "contraction", "bfloat16", T3, ("kji", "jkl", "li"), _repack(0, 1, _family(1)), env=REPACK),
    Case("f64_repack", "contraction", "float64", T3, ("kji", "jkl", "li"), _repack(0, 1, _family(2, None, True)), env=REPACK),
    Case("c64_repack", "contraction", "complex64", T3, ("kji", "jkl", "li"), _repack(0, 1, _family(2, None, True)), env=REPACK,
         alpha=0.75 + 0.5j),
    Case("bf16_repack_both", "contraction", "bfloat16", T3, ("jik", "jlk", "li"), _repack(1, 1, _family(1)), env=REPACK),
    # lone modes: one in A, one in B, one in each; every data type; nested (inner split-K, inner repacked)
    Case("f32_lone_A", "contraction", "float32", LONE, ("kji", "lk", "li"), _lone(1, 0, _family(0))),
    Case("f32_lone_B", "contraction", "float32", dict(i=20, k=50, j=17, l=9), ("ki", "ljk", "ji"), _lone(0, 1, _family(0))),
    Case("f32_lone_AB", "contraction", "float32", dict(a=5, i=30, j=50, k=12, b=6), ("jia", "jbk", "ik"), _lone(1, 1, _family(0))),
    Case("bf16_lone", "contraction", "bfloat16", LONE, ("kji", "lk", "li"), _lone(1, 0, _family(1))),
    Case("f16_lone", "contraction", "float16", LONE, ("kji", "lk", "li"), _lone(1, 0, _family(1))),
    Case("f64_lone", "contraction", "float64", LONE, ("kji", "lk", "li"), _lone(1, 0, _family(2))),
    Case("c64_lone", "contraction", "complex64", LONE, ("kji", "lk", "li"), _lone(1, 0, _family(2)), alpha=0.75 + 0.5j),
    Case("c128_lone", "contraction", "complex128", LONE, ("kji", "lk", "li"), _lone(1, 0, _family(2)), alpha=0.75 + 0.5j),
    Case("f32_lone_inner_splitk", "contraction", "float32", dict(i=64, j=5, k=4096, l=64), ("kji", "lk", "li"),
         _lone(1, 0, _family(0, None, True))),
    Case("f32_lone_inner_repack", "contraction", "float32", dict(T3, z=3), ("zkji", "jkl", "li"),
         lambda d: d.any("lone_reduce_A") and d.any("repack_B") and d.get("family") == 0, env=REPACK),
    # peeled wide contraction: a contracted peeled mode accumulates through D, C laid out differently from D
    Case("f32_peeled_c_ne_d", "contraction", "float32", PEEL, ("paqbrcsdte", "xpyqzrst", "abxcydze"),
         lambda d: d.get("peeled_contracted", 0) >= 1 and d.get("peel_launches", 0) >= 2 and d.get("kname") != "gett_wide_kernel", c_pad=0),
    # trinary contraction: the intermediate at the head of the workspace
    Case("f32_trinary_contraction", "contraction_trinary", "float32", dict(a=24, b=20, c=64, d=18, e=30),
         ("acd", "cb", "de", "abe"), lambda d: d.get("op") == "contraction_trinary" and d.get("intermediate_bytes", 0) > 0, pad=0),
    # block-sparse contraction: the largest need of its dense block contractions
    Case("f64_blocksparse", "blocksparse", "float64", dict(k=[1500, 1501], i=[20, 21], l=[3, 4]), ("kil", "kl", "i"),
         lambda d: d.get("op") == "blocksparse" and d.get("workspace", 0) > 0, pad=0,
         blocks=([(0, 0, 0), (1, 1, 1), (0, 1, 0), (1, 0, 1)], [(0, 0), (1, 1), (1, 0)], [(0,), (1,)])),
    # split reductions: [splitR][kept] partials
    Case("f32_reduce_split", "reduction", "float32", dict(a=40000, b=6), ("ab", "b"), _split_reduction),
    Case("bf16_reduce_split", "reduction", "bfloat16", dict(a=40000, b=6), ("ab", "b"), _split_reduction),
    Case("f64_reduce_split", "reduction", "float64", dict(a=40000, b=6), ("ab", "b"), _split_reduction),
    # element-wise plans: no workspace at all
    Case("f32_permutation", "permutation", "float32", dict(a=33, b=20, c=7), ("abc", "cab"), _elementwise, pad=0, betas=(None,)),
    Case("bf16_binary", "binary", "bfloat16", dict(a=33, b=20, c=7), ("abc", "cab"), _elementwise, pad=0, betas=(0.5,)),
    Case("f32_trinary_elementwise", "trinary", "float32", dict(a=33, b=20, c=7), ("abc", "bca", "cab", "cab"), _elementwise, pad=0,
         betas=(0.5,)),
]

NO_HOOKS = [c.id for c in CASES if not c.env]

# ---- planner-only corners of the estimate (tests/test_workspace_contract_cpu.py; they add nothing on the device, so not in CASES) ----
# Problems on which the estimate once took another route than the plan: COMPUTE_DESC_64F on fp32 / complex64 data (the plan runs on the
# simple / the mode-table kernel and takes no workspace), and a caller who names a candidate (such a plan is never repacked).  `est`,
# `req` and the path are those of the plan created at the preference's cap (the same at DEFAULT and at MAX).
T3_BIG = dict(i=2000, l=1360, j=16, k=72)               # 'ijk,lkj->il' at a size where copying B first pays for every data type


def _kname(name):
    return lambda d: d.get("kname") == name and not d.any("repack_A") and not d.any("repack_B")


class Corner:
    def __init__(self, id, dtype, ext, modes, expect, est, req, **plan_kw):
        self.id, self.dtype, self.ext, self.modes, self.expect, self.est, self.req, self.plan_kw = id, dtype, ext, modes, expect, est, req, plan_kw

    def __repr__(self):
        return self.id


_BIG = ("kji", "jkl", "li")
CORNERS = [
    Corner("f32_odd_compute64", "float32", ODD, ("mk", "kn", "mn"), _kname("gett_simple_kernel"), 0, 0, compute="64F"),
    Corner("f32_headline_compute64", "float32", HEAD, ("dcba", "ebcd", "ea"), _kname("gett_simple_kernel"), 0, 0, compute="64F"),
    Corner("c64_odd_compute64", "complex64", ODD, ("mk", "kn", "mn"), _kname("gett_wide_kernel"), 0, 0, compute="64F"),
    # the caller names candidate 0: the operands as they lie
    Corner("bf16_big_algo0", "bfloat16", T3_BIG, _BIG, _kname("gett_gen_kernel"), 0, 0, algo=0),
    Corner("f64_big_algo0", "float64", T3_BIG, _BIG, _kname("gett_gen_kernel"), 0, 0, algo=0),
    # fp32: the best four of the direct list, which holds what candidate 0 (splitK 2) and candidate 1 (splitK 4) need
    Corner("f32_big_algo0", "float32", T3_BIG, _BIG, _kname("gett_f32_kernel"), 43520000, 21760000, algo=0),
    Corner("f32_big_rank1", "float32", T3_BIG, _BIG, _kname("gett_f32_kernel"), 43520000, 43520000, kernel_rank=1),
    # the same shapes without a named candidate: B copied first; bf16 / fp64 need the temporary alone, fp32 keeps the best-four bound of
    # the inner problem's list on top of it
    Corner("bf16_big", "bfloat16", T3_BIG, _BIG, _repack(0, 1, _family(1, "gett_h16w4m4_kernel", False)), 3133440, 3133440),
    Corner("f64_big", "float64", T3_BIG, _BIG, _repack(0, 1, _family(2, "gett_gen_kernel", False)), 12533760, 12533760),
    Corner("f32_big", "float32", T3_BIG, _BIG, _repack(0, 1, _family(0, "gett_f32_stream_kernel", False)), 28026880, 6266880),
]


def corner_contract(ct, ops, corner):
    """estimate, required workspace and path of a corner at the DEFAULT and the MAX cap, and the agreement rule of plan_contract"""
    dt = {"bfloat16": ct.R_16BF, "float32": ct.R_32F, "float64": ct.R_64F, "complex64": ct.C_32F}[corner.dtype]
    e = lambda m: [corner.ext[c] for c in m]   # noqa: E731
    m = corner.modes
    h = ops.Handle()
    for name, pref in (("DEFAULT", ct.WORKSPACE_DEFAULT), ("MAX", ct.WORKSPACE_MAX)):
        p = ops.contraction_plan(h, e(m[0]), m[0], e(m[1]), m[1], e(m[2]), m[2], dtype=dt, workspace_pref=pref, workspace_limit=CAPS[name],
                                 **corner.plan_kw)
        try:
            d = check_agreement(ct, "%s %s" % (corner.id, name), p, p.workspace_estimate)
            assert corner.expect(d), "%s is off its path: %s" % (corner.id, d)
            assert (p.workspace_estimate, p.required_workspace) == (corner.est, corner.req), (corner.id, name, p.workspace_estimate, p.required_workspace)
        finally:
            p.destroy()


@contextmanager
def hook_env(case):
    old = {k: os.environ.get(k) for k in case.env}
    os.environ.update(case.env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _blocksparse_plan(ct, ops, h, case, dt, plan_kw):
    return ops.blocksparse_plan(h, case.ext, case.modes, case.blocks, dtype=dt, **plan_kw)


def make_plan(ct, ops, h, case, **plan_kw):
    """the case's plan; plan_kw: workspace_pref / workspace_limit (default: the DEFAULT estimate, element-wise plans too)"""
    plan_kw.setdefault("workspace_limit", None)
    dt = {"bfloat16": ct.R_16BF, "float16": ct.R_16F, "float32": ct.R_32F, "float64": ct.R_64F, "complex64": ct.C_32F,
          "complex128": ct.C_64F}[case.dtype]
    e = case.extents
    m = case.modes
    with hook_env(case):
        if case.kind == "blocksparse":
            return _blocksparse_plan(ct, ops, h, case, dt, plan_kw)
        if case.kind == "contraction":
            sD = gd.packed_strides(e(m[2]), case.pad)
            sC = gd.packed_strides(e(m[2]), case.c_pad)
            return ops.contraction_plan(h, e(m[0]), m[0], e(m[1]), m[1], e(m[2]), m[2], dtype=dt, strideC=sC, strideD=sD, **plan_kw)
        if case.kind == "contraction_trinary":
            return ops.contraction_trinary_plan(h, e(m[0]), m[0], e(m[1]), m[1], e(m[2]), m[2], e(m[3]), m[3], dtype=dt, **plan_kw)
        if case.kind == "reduction":
            return ops.reduction_plan(h, e(m[0]), m[0], e(m[1]), m[1], dtype=dt, strideC=gd.packed_strides(e(m[1]), case.pad), **plan_kw)
        if case.kind == "permutation":
            return ops.permutation_plan(h, e(m[0]), m[0], e(m[1]), m[1], dtype=dt, **plan_kw)
        if case.kind == "binary":
            return ops.binary_plan(h, e(m[0]), m[0], e(m[1]), m[1], op="ADD", dtype=dt, **plan_kw)
        if case.kind == "trinary":
            return ops.trinary_plan(h, e(m[0]), m[0], e(m[1]), m[1], e(m[2]), m[2], e(m[3]), m[3], dtype=dt, **plan_kw)
    raise ValueError(case.kind)


def check_path(ct, case, plan):
    d = describe(ct, plan)
    assert case.expect(d), "%s is off its path: %s" % (case.id, d)
    return d


# ---- execution on the GPU ----------------------------------------------------------------------------------------------------------
def _inputs(case):
    import torch
    g = torch.Generator()
    g.manual_seed(sum(map(ord, case.id)))
    if case.kind == "blocksparse":   # dense tensors with zeros where a block is absent
        lay = [BlockLayout(case.ext, m, c) for m, c in zip(case.modes, case.blocks)]
        return [lay[i].dense([gd.random_tensor(s, case.dtype, g, case.lo, case.hi) for s in lay[i].shapes], case.extents(case.modes[i]))
                for i in range(2)], g
    ins = [case.modes[0]] + ([case.modes[1]] if case.kind in ("contraction", "contraction_trinary", "trinary") else []) + \
          ([case.modes[2]] if case.kind in ("contraction_trinary", "trinary") else [])
    return [gd.random_tensor(case.extents(m), case.dtype, g, case.lo, case.hi) for m in ins], g


def _out_modes(case):
    return case.modes[{"contraction": 2, "blocksparse": 2, "contraction_trinary": 3, "reduction": 1, "permutation": 1, "binary": 1, "trinary": 3}[case.kind]]


def _reference(case, ins, alpha, beta, c_host):
    m = case.modes
    out = _out_modes(case)
    if case.kind in ("contraction", "blocksparse", "contraction_trinary", "reduction", "permutation"):
        ref = alpha * gd.reference(",".join(m[:len(ins)]) + "->" + out, *ins, dtype_name=case.dtype)
    elif case.kind == "binary":
        ref = alpha * gd.reference(m[0] + "->" + out, ins[0], dtype_name=case.dtype)
    else:   # trinary element-wise, ADD / ADD: alpha A + beta B + gamma C
        ref = sum(s * gd.reference(mi + "->" + out, x, dtype_name=case.dtype) for s, mi, x in zip((alpha, beta, beta), m[:3], ins))
    if c_host is not None and beta:
        ref = ref + beta * c_host.to(ref.dtype)
    return ref


def _execute(case, plan, dev, C, D, beta, ws_ptr, ws_size):
    a = case.alpha
    if case.kind == "blocksparse":
        from cudalibrarysamples_amd import cutensor as ct
        arr = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])   # noqa: E731
        al, be = plan.scalar(a), plan.scalar(beta)
        ct.check(ct.cutensorBlockSparseContract(plan.handle.h, plan.plan, ctypes.byref(al), arr(dev[0]), arr(dev[1]), ctypes.byref(be),
                                                C.ptrs if C else D.ptrs, D.ptrs, ws_ptr or None, ws_size, None))
    elif case.kind == "contraction":
        plan.contract(a, dev[0].data_ptr(), dev[1].data_ptr(), beta, C.ptr if C else 0, D.ptr, ws_ptr, ws_size)
    elif case.kind == "contraction_trinary":
        plan.contract_trinary(a, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), beta, C.ptr if C else 0, D.ptr, ws_ptr, ws_size)
    elif case.kind == "reduction":
        plan.reduce(a, dev[0].data_ptr(), beta, C.ptr if C else 0, D.ptr, ws_ptr, ws_size)
    elif case.kind == "permutation":
        plan.permute(a, dev[0].data_ptr(), D.ptr)
    elif case.kind == "binary":
        plan.binary(a, dev[0].data_ptr(), beta, C.ptr, D.ptr)
    else:
        plan.trinary(a, dev[0].data_ptr(), beta, dev[1].data_ptr(), beta, dev[2].data_ptr(), D.ptr)


def run_guarded(ct, plan, case, what=""):
    """Steps 2-6 of the contract for one plan: D in a NaN guard, a workspace of exactly required_workspace bytes between 0xFF guards,
    alpha != 1, beta = 0 and beta != 0 where the operation has a C; the same bits again from a 0x00 workspace; required - 1 refused."""
    import torch
    what = "%s %s" % (case.id, what)
    ins, g = _inputs(case)
    out_ext = case.extents(_out_modes(case))
    if case.kind == "blocksparse":
        lay = [BlockLayout(case.ext, m, c) for m, c in zip(case.modes, case.blocks)]
        dev = [[gd.packed_device(x[sl]) for sl in lay[i].slices] for i, x in enumerate(ins)]
        out = lambda: GuardedBlocks(lay[2], case.dtype)   # noqa: E731
    else:
        dev = [gd.packed_device(x) for x in ins]
        out = None
    req = plan.required_workspace
    elementwise = case.kind in ("permutation", "binary", "trinary")
    if elementwise:
        assert plan.workspace_estimate == 0 and req == 0, (what, plan.workspace_estimate, req)
    for beta in case.betas:
        c_host, C = None, None
        if case.kind == "binary" or (case.kind in ("contraction", "blocksparse", "contraction_trinary", "reduction") and beta):
            c_host = gd.random_tensor(out_ext, case.dtype, g, case.lo, case.hi)
            C = out() if out else gd.guarded_tensor(out_ext, case.dtype, case.c_pad if case.kind == "contraction" else case.pad)
            C.set(c_host)
        D = out() if out else gd.guarded_tensor(out_ext, case.dtype, case.pad)
        ws = gd.guarded_workspace(req, 0xFF)
        wsp = ws.ptr if req > 0 else 0
        tag = "%s beta=%r" % (what, beta)
        _execute(case, plan, dev, C, D, beta or 0.0, wsp, req)
        torch.cuda.synchronize()
        ws.check(tag + " (0xFF workspace)")
        D.check_guard(tag + " (0xFF workspace)")
        got = D.get()
        if C is not None:
            C.check_guard(tag + " (C)")
        assert not bool(torch.isnan(got).any()), "%s: NaN in D (%d of %d)" % (tag, int(torch.isnan(got).sum()), got.numel())
        ref = _reference(case, ins, case.alpha, beta or 0.0, c_host)
        if out:   # the blocks of D, flattened in block order (every block of C / D present)
            ref = torch.cat([ref[sl].reshape(-1) for sl in lay[2].slices])
        gd.assert_close(got, ref, case.dtype, tag)
        first = D.bits()
        # the same call from a workspace that held zeros: bit for bit the same D
        D.refill_nan()
        ws.refill(0x00)
        _execute(case, plan, dev, C, D, beta or 0.0, wsp, req)
        torch.cuda.synchronize()
        ws.check(tag + " (0x00 workspace)")
        D.check_guard(tag + " (0x00 workspace)")
        second = D.bits()
        if not (first == second).all():
            raise AssertionError("%s: D differs between a 0xFF and a 0x00 workspace at %d bytes" % (tag, int((first != second).sum())))
        if req > 0:   # one byte short: refused, D untouched
            D.refill_nan()
            try:
                _execute(case, plan, dev, C, D, beta or 0.0, ws.ptr, req - 1)
            except ct.CuTensorError as e:
                assert e.status == ct.STATUS_INSUFFICIENT_WORKSPACE, (tag, e.status)
            else:
                raise AssertionError("%s: a workspace of required - 1 bytes was accepted" % tag)
            torch.cuda.synchronize()
            assert (D.bits() == 0xFF).all(), "%s: D written by a refused call" % tag


def run_case(ct, ops, h, case):
    """the whole GPU contract of a case: the DEFAULT-estimate plan guarded, then the MIN-estimate plan (the retry path of the
    reference's binding, cuTENSOR/python/cutensor/torch/einsum.cc:110)"""
    p = make_plan(ct, ops, h, case)
    try:
        d = check_path(ct, case, p)
        assert case.gpu_expect(d), "%s is off its path on the GPU: %s" % (case.id, d)
        run_guarded(ct, p, case, "(DEFAULT estimate %d, required %d)" % (p.workspace_estimate, p.required_workspace))
    finally:
        p.destroy()
    p = make_plan(ct, ops, h, case, workspace_pref=ct.WORKSPACE_MIN)
    try:
        run_guarded(ct, p, case, "(MIN estimate %d, required %d)" % (p.workspace_estimate, p.required_workspace))
    finally:
        p.destroy()


# ---- the planning contract (no GPU) ---------------------------------------------------------------------------------------------
def _plan_or_status(ct, ops, h, case, **kw):
    try:
        return make_plan(ct, ops, h, case, **kw), None
    except ct.CuTensorError as e:
        return None, e.status


def _limits(est_min, req):
    return sorted({0, 128, 255, 256, est_min, max(req - 1, 0), req, 2 * req})


def _check_limits(ct, ops, h, case, est_min, limits):
    for L in limits:
        p, st = _plan_or_status(ct, ops, h, case, workspace_limit=L)
        if p is None:
            assert st == ct.STATUS_INSUFFICIENT_WORKSPACE, (case.id, L, st)
            assert L < est_min, "%s: refused at limit %d although estimate(MIN) = %d" % (case.id, L, est_min)
        else:
            assert p.required_workspace <= L, "%s: limit %d, required %d" % (case.id, L, p.required_workspace)
            p.destroy()


# The workspace limit cutensorEstimateWorkspaceSize routes a problem at, per preference: `cap` in cutensorEstimateWorkspaceSize
# (cudalibrarysamples_amd/csrc/host/api.cpp); WORKSPACE_MIN routes nothing
CAPS = {"DEFAULT": 1 << 30, "MAX": 4 << 30}


def _has_family0(pairs):
    """a kernel of family 0 (the fp32 ranked list) anywhere in a plan's description, top level or inner"""
    for item in pairs:
        if isinstance(item, tuple):
            if item[0] == "family" and item[1] == 0:
                return True
            item = item[1]
        if isinstance(item, list) and _has_family0(item):
            return True
    return False


def check_agreement(ct, what, plan_at_cap, estimate):
    """The estimate is the route cutensorCreatePlan takes at the preference's cap, added up: it equals what the plan created at the cap
    requires.  The one exception is the library's policy for the fp32 ranked list (family 0): the estimate is the largest need among
    its best four candidates, so it bounds the requirement from above."""
    d = describe(ct, plan_at_cap)
    req = plan_at_cap.required_workspace
    if _has_family0(d.pairs):
        assert estimate >= req, "%s: estimate %d below what the plan at the cap requires (%d): %s" % (what, estimate, req, d)
    else:
        assert estimate == req, "%s: estimate %d, the plan at the cap requires %d: %s" % (what, estimate, req, d)
    return d


def plan_contract(ct, ops, case):
    """a plan at each preference's estimate requires at most that estimate; MIN <= DEFAULT <= MAX; at any limit a plan fits or is
    refused with INSUFFICIENT_WORKSPACE, and only below estimate(MIN); the DEFAULT and MAX estimates agree with the plan created at
    the preference's cap (check_agreement)"""
    h = ops.Handle()
    est = {}
    for name, pref in (("MIN", ct.WORKSPACE_MIN), ("DEFAULT", ct.WORKSPACE_DEFAULT), ("MAX", ct.WORKSPACE_MAX)):
        p, st = _plan_or_status(ct, ops, h, case, workspace_pref=pref)
        assert p is not None, "%s: no plan at the %s estimate (status %d)" % (case.id, name, st)
        assert p.required_workspace <= p.workspace_estimate, (case.id, name, p.workspace_estimate, p.required_workspace)
        if name == "DEFAULT":
            check_path(ct, case, p)
            req = p.required_workspace
        est[name] = p.workspace_estimate
        p.destroy()
        if name in CAPS:
            p, st = _plan_or_status(ct, ops, h, case, workspace_pref=pref, workspace_limit=CAPS[name])
            assert p is not None, "%s: no plan at the %s cap (status %d)" % (case.id, name, st)
            check_agreement(ct, "%s %s" % (case.id, name), p, est[name])
            p.destroy()
    assert est["MIN"] <= est["DEFAULT"] <= est["MAX"], (case.id, est)
    if case.kind in ("permutation", "binary", "trinary"):
        assert est["MAX"] == 0 and req == 0, (case.id, est, req)
    _check_limits(ct, ops, h, case, est["MIN"], _limits(est["MIN"], req))


def memo_contract(ct, ops, case):
    """the same limits on a handle with the plan memo, the large limit first: the memo is keyed by the limit, so a small-limit plan
    must not inherit a large-limit requirement"""
    h = ops.Handle()
    p = make_plan(ct, ops, h, case, workspace_pref=ct.WORKSPACE_MIN)
    est_min = p.workspace_estimate
    p.destroy()
    p = make_plan(ct, ops, h, case)
    req = p.required_workspace
    p.destroy()
    hm = ops.Handle(plan_cache=64)
    limits = sorted(set(_limits(est_min, req)) | {1 << 30}, reverse=True)
    for _ in range(2):   # planned, then answered by the memo
        _check_limits(ct, ops, hm, case, est_min, limits)


def in_child(mode, ids, env, timeout):
    """`python workspace_cases.py MODE ids...` in a fresh process (its own time limit; a hang fails the caller instead of stalling it)"""
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    child_env = dict(os.environ, PYTHONPATH=os.pathsep.join([root, here]), **env)
    r = subprocess.run([sys.executable, os.path.join(here, "workspace_cases.py"), mode] + list(ids), capture_output=True, text=True,
                       timeout=timeout, env=child_env, cwd=root)
    assert r.returncode == 0, "child exit %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.count("ok ") == len(ids), r.stdout


if __name__ == "__main__":
    # plan / memo / run: one case each in a process of its own (Case.fresh); production: the cases that need no switch on lib/
    import sys
    from cudalibrarysamples_amd import cutensor as ct_, ops as ops_
    mode = sys.argv[1]
    if mode == "production":
        assert os.environ.get("CTAMD_LIB_FLAVOUR") != "hooks" and "lib_hooks" not in ct_.LIB_PATH, ct_.LIB_PATH
    h_ = ops_.Handle()
    for cid in sys.argv[2:]:
        c_ = next(c for c in CASES if c.id == cid)
        if mode == "plan":
            plan_contract(ct_, ops_, c_)
        elif mode == "memo":
            memo_contract(ct_, ops_, c_)
        else:
            run_case(ct_, ops_, h_, c_)
        print("ok", cid, flush=True)
