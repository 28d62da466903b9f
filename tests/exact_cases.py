"""The case table of the exact-data tests (tests/test_exact_data_cpu.py checks every draw, tests/test_gpu_exact.py runs every case) — a
helper module, not a conftest, in the style of tests/workspace_cases.py.

One case per contraction path: id, data type, extents, modes, the switches that reach the path and a predicate on the plan's
description that proves the path ran.  A case runs twice (the two draws of tests/exact_data.py); every tensor lives in a NaN-filled
buffer (D pre-filled with NaN when beta = 0, its padding and surroundings checked afterwards), at an odd element offset and with padded
pitches where the case says so.  Cases whose switch the library reads once per process run in a child: `python exact_cases.py run ids...`."""
import os
import sys

import exact_data as xd
import workspace_cases as wc
from workspace_cases import GEN, LONE, ODD, PEEL, REPACK, T3, _family, _lone, _repack

GUARD = 2048      # elements of NaN on each side of every tensor


class Case:
    def __init__(self, id, dtype, ext, modes, expect=None, env=None, alpha=1.0, beta=0.0, kind="contraction", algo=None, pad=(0, 0, 0), off=0,
                 align=None, conj=(False, False, False), dense_values=None, one_per_k=False, data_key=None, full_size=False, ws_limit=1 << 28,
                 blocks=None, group=None, gpu_expect=None):
        self.id, self.dtype, self.ext, self.modes, self.kind = id, dtype, ext, modes, kind
        self.expect = expect or (lambda d: True)
        self.gpu_expect = gpu_expect or (lambda d: True)     # what only a plan made with a device shows
        self.env = dict(env or {})
        self.alpha, self.beta, self.algo, self.pad, self.off, self.align = alpha, beta, algo, pad, off, align
        self.conjA, self.conjB, self.conjC = conj
        self.dense_values, self.one_per_k = dense_values, one_per_k
        self.data_key = data_key or id          # cases that share a key share their data and their reference (candidate sweeps)
        self.full_size, self.ws_limit, self.blocks = full_size, ws_limit, blocks
        self.group = group                      # the child process the case runs in (None: the test's own process)
        # what tests/workspace_cases.py's plan helpers read (trinary contraction, block-sparse)
        self.c_pad = 0
        self.betas = (beta,)

    def __repr__(self):
        return self.id

    def extents(self, m):
        return [sum(self.ext[c]) if self.blocks else self.ext[c] for c in m]


# ---- the table ------------------------------------------------------------------------------------------------------------------------
LAYOUTS = (("mk", "kn"), ("km", "kn"), ("mk", "nk"), ("km", "nk"))
LNAME = {("mk", "kn"): "mk_kn", ("km", "kn"): "km_kn", ("mk", "nk"): "mk_nk", ("km", "nk"): "km_nk"}
SCALARS32 = [(1.0, 0.0), (-2.0, 1.0), (0.5, -0.5), (-2.0, 0.0), (1.0, 1.0), (0.5, 0.0)]       # alpha in {1, -2, 0.5}, beta in {0, 1, -0.5}
SCALARS16 = [(1.0, 0.0), (-1.0, 2.0), (2.0, -1.0), (-2.0, 0.0), (1.0, 1.0), (2.0, 0.0)]       # 16-bit: alpha, beta in {+-1, +-2}

CASES = []


def add(*a, **kw):
    c = Case(*a, **kw)
    assert all(c.id != o.id for o in CASES), c.id
    CASES.append(c)
    return c


def _scal(i, dtype):
    s = (SCALARS16 if dtype in xd.H16 else SCALARS32)[i % 6]
    return dict(alpha=s[0], beta=s[1])


def _kname(*names, **more):
    return lambda d: d.get("kname") in names and all(d.get(k) == v for k, v in more.items())


def _split(d):
    return d.get("splitK", 1) > 1


def one_launch(d):
    """the plan is ONE launch of its kernel: nothing peeled, reduced beforehand or repacked, no split-K fold"""
    assert d["splitK"] == 1 and not any(d.get(k) for k in ("peel_launches", "lone_reduce_A", "lone_reduce_B", "repack_A", "repack_B")), d


# M = {a, b} and N = {c, d} interleave in D (and C), so neither fuses: the mixed-radix side of the general family's row clamp and of its
# epilogue offsets.  M = 63 and N = 45 are ragged against the 64-wide tile, k = 37 against every K-tile; two batches.  Pitch padding
# (A, B, D, C): C's pitch differs from D's.
UNFUSED = dict(a=9, b=7, c=5, d=9, k=37, l=2)
UNFUSED_LONG = dict(UNFUSED, k=517)      # 17 K-tiles of 32 (33 of 16) on two output tiles: the planner splits K by itself
UNFUSED_MODES = ("kabl", "kcdl", "acbdl")
UNFUSED_PAD = (0, 0, 1, 3)

HEADLINE = dict(a=96, b=64, c=64, d=64, e=96)
HEAD_MODES = ("dcba", "ebcd", "ea")                     # 'abcd,dcbe->ae' in the ABI's order (fastest mode first)

# fp32 headline at full size, every output: split-K 256 + fold; with the in-launch fold in a child
add("f32_headline_full", "float32", HEADLINE, HEAD_MODES, lambda d: d.get("family") == 0 and d.get("splitK") == 256 and d.get("fusedFold", 0) == 0,
    full_size=True, ws_limit=1 << 30)
add("f32_headline_full_fused_fold", "float32", HEADLINE, HEAD_MODES, lambda d: d.get("family") == 0 and _split(d), gpu_expect=lambda d: d.get("fusedFold") == 1,
    env={"CUTENSOR_AMD_FUSED_FOLD": "1"}, full_size=True, ws_limit=1 << 30, group="fused_fold", data_key="f32_headline_full")
add("f32_headline_full_korder", "float32", HEADLINE, HEAD_MODES, lambda d: d.get("family") == 0 and _split(d),
    env={"CUTENSOR_AMD_KORDER": "B"}, full_size=True, ws_limit=1 << 30, group="korder", data_key="f32_headline_full")
# contraction.cu's default extents: the planner's choice
add("f32_sample_full", "float32", dict(m=96, n=96, u=96, v=64, h=64, k=64), ("mhkn", "ukvh", "munv"), _kname("gett_f32_stream_kernel"),
    alpha=-2.0, full_size=True, ws_limit=None)
# 8192^3 bf16, the planner's choice
add("bf16_8192_full", "bfloat16", dict(m=8192, n=8192, k=8192), ("mk", "kn", "mn"), _family(1), full_size=True, ws_limit=None)

# fp32 off the lanes: the shapes, odd element offsets and NaN guards of tests/test_gpu_f32_unaligned.py (RAG twins of the ring kernel)
F32_UNALIGNED = ((258, 130, 98), (257, 129, 65), (50, 50, 50), (131, 67, 191), (64, 64, 3), (9, 3, 130), (300, 204, 100), (130, 258, 33))
for li, (mA, mB) in enumerate(LAYOUTS):
    L = LNAME[(mA, mB)]
    for i, (m_, n_, k_) in enumerate(F32_UNALIGNED):
        add("f32_unal_%s_%dx%dx%d" % (L, m_, n_, k_), "float32", dict(m=m_, n=n_, k=k_), (mA, mB, "mn"), _family(0), off=3, align=4,
            **_scal(i + li, "float32"))
    add("f32_unal_%s_padded" % L, "float32", dict(m=262, n=134, k=134), (mA, mB, "mn"), _family(0), off=3, align=4, pad=(5, 3, 1), alpha=0.5, beta=1.0)
    add("f32_unal_%s_splitk" % L, "float32", dict(m=100, n=60, k=4099), (mA, mB, "mn"), lambda d: d.get("family") == 0 and _split(d), off=3, align=4,
        alpha=-2.0, beta=-0.5)
    add("f32_unal_%s_1027" % L, "float32", dict(m=1026, n=1030, k=1027), (mA, mB, "mn"), _kname("gett_f32_stream_kernel"), off=3, align=4)
    add("f32_4098_%s" % L, "float32", dict(m=4098, n=4098, k=4098), (mA, mB, "mn"), _kname("gett_f32_stream_kernel"), data_key="f32_4098_" + L)
    # the row-epilogue shapes of tests/test_gpu_f32_rows.py: aligned base (the row image), padded pitches that keep / lose the lanes, batch
    for i, (m_, n_, k_) in enumerate(((260, 132, 96), (100, 52, 128), (1028, 36, 96), (4, 8, 64))):
        add("f32_rows_%s_%dx%dx%d" % (L, m_, n_, k_), "float32", dict(m=m_, n=n_, k=k_), (mA, mB, "mn"), _family(0), off=4, align=16,
            **_scal(i + li + 1, "float32"))
    add("f32_rows_%s_pitch4" % L, "float32", dict(m=264, n=136, k=128), (mA, mB, "mn"), _family(0), off=4, align=16, pad=(5, 3, 4), alpha=1.0, beta=-0.5)
    add("f32_rows_%s_pitch1" % L, "float32", dict(m=264, n=136, k=128), (mA, mB, "mn"), _family(0), off=4, align=16, pad=(0, 0, 1), alpha=-2.0, beta=1.0)
    add("f32_rows_%s_batch" % L, "float32", dict(m=132, n=68, k=64, l=3), (mA + "l", mB + "l", "mnl"), _family(0), off=4, align=16, alpha=0.5, beta=1.0)
add("f32_rows_multi", "float32", dict(m=24, n=20, u=12, v=8, h=16, k=16), ("mhkn", "ukvh", "munv"), _family(0), alpha=-2.0, beta=-0.5)
# short-K batch 'bhqd,bhkd->bhqk'
add("f32_short_k_batch", "float32", dict(b=4, h=6, q=100, k=72, d=16), ("dqhb", "dkhb", "kqhb"), _family(0), alpha=0.5, beta=1.0)

# mode-table / peeled / gett_simple
WIDE_A, WIDE_B = "badcfehgjilknm", "ponmlkqrst"[::-1]
WIDE_C = "".join(c for c in "abcdefghijopqrst" if (c in WIDE_A) != (c in WIDE_B))
WIDE_EXT = {c: (3 if c in "aq" else 2) for c in set(WIDE_A + WIDE_B)}
for dt in ("float32", "float64"):
    add("%s_mode_table" % dt, dt, WIDE_EXT, (WIDE_A, WIDE_B, WIDE_C), _kname("gett_wide_kernel"), alpha=-2.0, beta=-0.5, ws_limit=None)
    add("%s_peeled" % dt, dt, PEEL, ("paqbrcsdte", "xpyqzrst", "abxcydze"),
        lambda d: d.get("peel_launches", 0) >= 2 and d.get("kname") != "gett_wide_kernel", alpha=0.5, beta=1.0, ws_limit=1 << 24)
    add("%s_peel_off" % dt, dt, PEEL, ("paqbrcsdte", "xpyqzrst", "abxcydze"), _kname("gett_wide_kernel"), env={"CUTENSOR_AMD_PEEL": "0"},
        alpha=-2.0, beta=1.0, ws_limit=1 << 24, group="peel0")
add("f64_gen_off_simple", "float64", ODD, ("mk", "kn", "mn"), _kname("gett_simple_kernel"), env={"CUTENSOR_AMD_GEN": "0"}, alpha=0.5, beta=-0.5,
    group="gen0")
add("bf16_gen_off_simple", "bfloat16", dict(m=37, n=29, k=50, j=3), ("mkj", "jkn", "mn"), _kname("gett_simple_kernel"), env={"CUTENSOR_AMD_GEN": "0"},
    alpha=-1.0, beta=2.0, group="gen0")
add("c64_gen_off_mode_table", "complex64", ODD, ("mk", "kn", "mn"), _kname("gett_wide_kernel"), env={"CUTENSOR_AMD_GEN": "0"}, alpha=-2.0, beta=1.0,
    group="gen0")

# the general MFMA family
for dt in ("bfloat16", "float16"):
    add("%s_gen_forced_odd" % dt, dt, ODD, ("mk", "kn", "mn"), _family(2, "gett_gen_kernel", True), env=GEN, group="gen_force", **_scal(1, dt))
    add("%s_gen_forced_aligned" % dt, dt, dict(m=200, n=136, k=104), ("km", "kn", "mn"), _family(2, "gett_gen_kernel"), env=GEN, group="gen_force",
        **_scal(2, dt))
    add("%s_gen_77_53_91" % dt, dt, dict(m=77, n=53, k=91, j=3), ("mkj", "jkn", "mn"), _family(2, "gett_gen_kernel"), **_scal(3, dt))
add("f16_gen_reference_equation", "float16", dict(m=20, l=50, i=50, k=50, j=50), ("kilm", "mjkl", "jil"), _family(2, "gett_gen_kernel"))   # 'mlik,lkjm->lij'
for dt in ("float64", "complex64", "complex128"):
    add("%s_gen_odd_splitk" % dt, dt, ODD, ("mk", "kn", "mn"), _family(2, "gett_gen_kernel", True), alpha=-2.0, beta=1.0)
    add("%s_gen_77_53_91" % dt, dt, dict(m=77, n=53, k=91), ("km", "nk", "mn"), _family(2, "gett_gen_kernel"), alpha=0.5, beta=-0.5)
    add("%s_gen_batch" % dt, dt, dict(m=44, n=36, k=28, l=3), ("mkl", "knl", "mnl"), _family(2, "gett_gen_kernel"), alpha=1.0, beta=1.0)
for dt in ("complex64", "complex128"):
    for name, conj in (("conjA", (True, False, False)), ("conjB", (False, True, False)), ("conjC", (False, False, True)), ("conjABC", (True, True, True))):
        add("%s_gen_%s" % (dt, name), dt, dict(m=44, n=36, k=28, l=3), ("kml", "nkl", "mnl"), _family(2, "gett_gen_kernel"), conj=conj, alpha=-2.0, beta=1.0)

# copies first: the T3 shapes of tests/test_gpu_repack.py
for dt, fam in (("float32", _family(0)), ("bfloat16", _family(1)), ("float64", _family(2, None, True)), ("complex64", _family(2, None, True))):
    add("%s_repack" % dt, dt, T3, ("kji", "jkl", "li"), _repack(0, 1, fam), env=REPACK, group="repack", **_scal(1, dt))
add("bf16_repack_both", "bfloat16", T3, ("jik", "jlk", "li"), _repack(1, 1, _family(1)), env=REPACK, group="repack", alpha=2.0, beta=-1.0)

# lone modes (the shapes of tests/workspace_cases.py)
add("f32_lone_A", "float32", LONE, ("kji", "lk", "li"), _lone(1, 0, _family(0)), alpha=-2.0, beta=1.0)
add("f32_lone_B", "float32", dict(i=20, k=50, j=17, l=9), ("ki", "ljk", "ji"), _lone(0, 1, _family(0)), alpha=0.5, beta=-0.5)
add("f32_lone_AB", "float32", dict(a=5, i=30, j=50, k=12, b=6), ("jia", "jbk", "ik"), _lone(1, 1, _family(0)), alpha=1.0, beta=1.0)
add("f32_lone_inner_splitk", "float32", dict(i=64, j=5, k=4096, l=64), ("kji", "lk", "li"), _lone(1, 0, _family(0, None, True)), alpha=-2.0)
add("f64_lone", "float64", LONE, ("kji", "lk", "li"), _lone(1, 0, _family(2)), alpha=0.5, beta=1.0)
add("c64_lone", "complex64", LONE, ("kji", "lk", "li"), _lone(1, 0, _family(2)), alpha=-2.0, beta=1.0)
add("c128_lone", "complex128", LONE, ("kji", "lk", "li"), _lone(1, 0, _family(2)), alpha=1.0, beta=-0.5)
# 16-bit: the lone-mode sum is rounded to the data type by design.  +-1 over j = 7: |sum| <= 7, nothing rounds ...
add("bf16_lone_small_sums", "bfloat16", LONE, ("kji", "lk", "li"), _lone(1, 0, _family(1)), alpha=-1.0, beta=2.0)
add("f16_lone_small_sums", "float16", LONE, ("kji", "lk", "li"), _lone(1, 0, _family(1)), alpha=2.0, beta=-1.0)
# ... {1, 2, 3} over j = 300: sums of 500 .. 700, bf16 keeps multiples of 4 there — the rounding point is what is asserted
add("bf16_lone_rounded_sums", "bfloat16", dict(i=20, j=300, k=16, l=21), ("kji", "lk", "li"), _lone(1, 0, _family(1)), dense_values=(1, 2, 3),
    one_per_k=True)

# trinary contraction and block-sparse contraction
add("f32_trinary_contraction", "float32", dict(a=24, b=20, c=64, d=18, e=30), ("acd", "cb", "de", "abe"),
    lambda d: d.get("op") == "contraction_trinary" and d.get("intermediate_bytes", 0) > 0, kind="contraction_trinary", alpha=-2.0, beta=1.0)
add("f64_blocksparse", "float64", dict(k=[1500, 1501], i=[20, 21], l=[3, 4]), ("kil", "kl", "i"),
    lambda d: d.get("op") == "blocksparse" and d.get("workspace", 0) > 0, kind="blocksparse", alpha=0.5, beta=1.0,
    blocks=([(0, 0, 0), (1, 1, 1), (0, 1, 0), (1, 0, 1)], [(0, 0), (1, 1), (1, 0)], [(0,), (1,)]))

# 16-bit LDS-DMA kernels: every forced variant x four layouts x {aligned, ragged K, sweep-ragged, no 16-byte lanes}
H16_VARIANTS = {"4x": "gett_h16w4x_kernel", "4p": "gett_h16w4p_kernel", "4m": "gett_h16w4m_kernel", "4m4": "gett_h16w4m4_kernel",
                "8m": "gett_h16w8m_kernel", "4q": "gett_h16w4q_kernel"}
MASKING = ("4x", "4m", "4m4", "4q")                      # the kernels that mask a partial K-tile
SWEEP_LAYOUTS = (("kmj", "kjn"), ("mjk", "kjn"), ("kmj", "nkj"), ("mjk", "nkj"))
H16_UNALIGNED = ((300, 204, 100), (257, 129, 65), (50, 50, 50), (131, 67, 191), (64, 64, 7), (9, 3, 130))


def _h16_variant(waves):
    # (a variant asked for on a shape it cannot stage leaves the problem to another kernel: the predicate names the variant where it applies)
    return lambda d: d.get("family") == 1 and d.get("kname") == H16_VARIANTS[waves]


def _h16_cases(waves):
    env = {"CUTENSOR_AMD_H16_WAVES": waves}
    g = "h16_" + waves
    want = _h16_variant(waves)
    n = 0
    for li, (mA, mB) in enumerate(LAYOUTS):
        L = LNAME[(mA, mB)]
        dt = ("bfloat16", "float16")[li % 2]
        od = ("float16", "bfloat16")[li % 2]
        add("%s_%s_aligned_%s" % (dt, g, L), dt, dict(m=512, n=512, k=256), (mA, mB, "mn"), want, env=env, group=g, **_scal(n, dt)); n += 1
        add("%s_%s_edges_%s" % (od, g, L), od, dict(m=520, n=264, k=192), (mA, mB, "mn"), want, env=env, group=g, **_scal(n, od)); n += 1
        if waves in MASKING:
            for k_ in ((264, 520, 1000) if waves == "4x" else (264, 1000)):      # (the non-default variants: a thinner product)
                add("%s_%s_ragged_k%d_%s" % (dt, g, k_, L), dt, dict(m=384, n=264, k=k_), (mA, mB, "mn"), want, env=env, group=g, **_scal(n, dt)); n += 1
            sA, sB = SWEEP_LAYOUTS[li]
            add("%s_%s_sweep_ragged_%s" % (od, g, L), od, dict(m=264, n=136, k=72, j=5), (sA, sB, "mn"),
                lambda d, w=want: w(d) and d.get("rag") == 1, env=env, group=g, **_scal(n, od)); n += 1
            for i, (m_, n_, k_) in enumerate(H16_UNALIGNED if waves == "4x" else H16_UNALIGNED[:4]):
                t = (dt, od)[i % 2]
                add("%s_%s_unal_%s_%dx%dx%d" % (t, g, L, m_, n_, k_), t, dict(m=m_, n=n_, k=k_), (mA, mB, "mn"), want, env=env, group=g, off=3, align=2,
                    **_scal(n, t)); n += 1
            add("%s_%s_unal_padded_%s" % (dt, g, L), dt, dict(m=260, n=132, k=132), (mA, mB, "mn"), want, env=env, group=g, off=3, align=2, pad=(5, 3, 1),
                alpha=1.0, beta=1.0)


for _w in H16_VARIANTS:
    _h16_cases(_w)

# the persistent kernel on a grid of 8 workgroups: many tiles per workgroup, odd K-tile counts, beta != 0, batch mode
P8 = {"CUTENSOR_AMD_H16_WAVES": "4p", "CUTENSOR_AMD_H16P_GRID": "8"}
for i, (ext, mA, mB, mC, dt) in enumerate([
        (dict(m=1024, n=768, k=256), "mk", "kn", "mn", "bfloat16"), (dict(m=1024, n=768, k=256), "km", "nk", "mn", "float16"),
        (dict(m=768, n=1280, k=64), "mk", "kn", "mn", "bfloat16"), (dict(m=768, n=1280, k=192), "mk", "kn", "mn", "bfloat16"),
        (dict(m=1000, n=712, k=320), "mk", "nk", "mn", "float16"), (dict(m=1280, n=1024, k=320), "km", "kn", "mn", "bfloat16"),
        (dict(m=512, n=768, k=256, l=7), "mkl", "knl", "mnl", "bfloat16"), (dict(m=768, n=512, k=384, l=3), "kml", "nkl", "mnl", "float16"),
        (dict(m=1024, n=512, k=256), "mk", "kn", "nm", "bfloat16")]):
    add("%s_h16p_grid8_%d" % (dt, i), dt, ext, (mA, mB, mC), _kname("gett_h16w4p_kernel"), env=P8, group="h16p_grid8",
        **dict(_scal(i, dt), **({"beta": 1.0} if i in (3, 4, 6) else {})))
# forced split-K factors of the 16-bit family
for sk in (1, 3, 8):
    for dt, ext, mm in (("bfloat16", dict(m=96, n=96, k=4104), ("km", "kn", "mn")), ("float16", dict(m=264, n=120, k=1536), ("mk", "kn", "mn"))):
        add("%s_h16_splitk%d" % (dt, sk), dt, ext, mm, lambda d, sk=sk: d.get("family") == 1 and d.get("splitK", 1) == sk,
            env={"CUTENSOR_AMD_H16_SPLITK": str(sk)}, group="h16_splitk%d" % sk, **_scal(sk, dt))
# the planner's own choice: split-K (aligned, ragged), 4100-class without lanes
for dt in ("bfloat16", "float16"):
    add("%s_lds_splitk" % dt, dt, dict(m=64, n=64, k=4096), ("km", "kn", "mn"), _family(1, None, True), **_scal(1, dt))
    add("%s_lds_splitk_ragged" % dt, dt, dict(m=96, n=96, k=4104), ("km", "kn", "mn"), _family(1, None, True), **_scal(2, dt))
    add("%s_lds_k2048" % dt, dt, dict(m=512, n=256, k=2048), ("mk", "kn", "mn"), _family(1), **_scal(3, dt))
add("bf16_lds_splitk_odd", "bfloat16", ODD, ("mk", "kn", "mn"), _family(1, None, True), alpha=-1.0, beta=2.0)
add("bf16_headline_shape", "bfloat16", dict(a=96, b=16, c=16, d=64, e=96), HEAD_MODES, lambda d: d.get("family") == 1 and _split(d))
for mA, mB in LAYOUTS:
    add("bf16_4100_%s" % LNAME[(mA, mB)], "bfloat16", dict(m=4100, n=4100, k=4100), (mA, mB, "mn"), _family(1), off=3, align=2)
    add("bf16_unal_splitk_%s" % LNAME[(mA, mB)], "bfloat16", dict(m=100, n=60, k=4100), (mA, mB, "mn"), _family(1, None, True), off=3, align=2,
        alpha=2.0, beta=-1.0)

BY_ID = {c.id: c for c in CASES}
IN_PROCESS = [c.id for c in CASES if c.group is None and not c.full_size]
GROUPS = sorted({c.group for c in CASES if c.group})
# the sweep problems of tests/test_gpu_contraction.py::test_every_candidate_kernel_and_split, and the one-tile shapes of its nontemporal twins
SWEEP_PROBLEMS = [
    (dict(a=96, b=4, c=4, d=64, e=96), "dcba", "ebcd", "ea"), (dict(a=96, b=3, c=4, d=64, e=96), "dcba", "ebcd", "ea"),
    (dict(m=160, n=144, k=256), "mk", "nk", "mn"), (dict(m=160, n=144, k=256), "km", "kn", "mn"), (dict(m=144, n=160, k=256), "mk", "kn", "nm"),
    (dict(a=40, b=6, c=20, e=56), "cba", "ebc", "ea"), (dict(m=72, n=40, k=12, j=9), "mkj", "nkj", "mn"), (dict(m=72, n=40, k=12, j=9), "kjm", "kjn", "mn"),
    (dict(m=40, n=72, k=12, j=9), "mkj", "kjn", "nm"), (dict(m=70, n=50, k=300), "mk", "kn", "mn")]
NT_PROBLEMS = [(dict(m=96, n=96, k=512), "km", "kn", "mn"), (dict(m=96, n=96, k=512), "mk", "nk", "mn"), (dict(m=96, n=96, k=512), "mk", "kn", "nm"),
               (dict(a=96, b=4, c=4, d=64, e=96), "dcba", "ebcd", "ea")]
NO_SWITCH = [c.id for c in CASES if not c.env and not c.full_size and c.kind == "contraction" and xd.work(c) < 1e9]


def sweep_case(problems, tag, i, rank, **kw):
    ext, mA, mB, mC = problems[i]
    return Case("f32_%s_p%d_r%d" % (tag, i, rank), "float32", ext, (mA, mB, mC), _family(0), alpha=-2.0, beta=1.0, algo=rank,
                data_key="f32_%s_p%d" % (tag, i), **kw)


# the planner's first candidates (ring kernels and register-staged ones, tiles 32 .. 128, split-K) off the lanes and on the row epilogue,
# as tests/test_gpu_f32_unaligned.py and tests/test_gpu_f32_rows.py sweep them
UNALIGNED_SWEEP = [(dict(m=m_, n=n_, k=k_), mA, mB, "mn") for (mA, mB) in LAYOUTS for (m_, n_, k_) in ((258, 130, 98), (257, 129, 65), (131, 67, 191), (300, 204, 1030))]
ROWS_SWEEP = [(dict(m=m_, n=n_, k=k_), mA, mB, "mn") for (mA, mB) in LAYOUTS for (m_, n_, k_) in ((260, 132, 96), (384, 200, 32), (128, 128, 128))]


# ---- one tensor in a NaN-filled device buffer ------------------------------------------------------------------------------------------
class Placed:
    """extents (first fastest), the first mode's pitch padded by `pad`, at element offset `off` behind a 256-byte-aligned guard"""

    def __init__(self, extents, dtype, pad=0, off=0, strides=None):
        import torch
        import guarded as gd
        self.extents = list(extents)
        self.tdt = xd.TORCH_DTYPES[dtype]
        self.es = torch.empty((), dtype=self.tdt).element_size()
        self.strides = list(strides) if strides is not None else gd.packed_strides(self.extents, pad)     # (strides: any padded pitches)
        span = 1 + sum((e - 1) * s for e, s in zip(self.extents, self.strides)) if self.extents else 1
        self.start = GUARD + off
        self.raw = torch.full(((2 * GUARD + off + span) * self.es,), 0xFF, dtype=torch.uint8, device="cuda")     # 0xFF..: a NaN in every type
        self.buf = self.raw.view(self.tdt)
        self.ptr = self.buf.data_ptr() + self.start * self.es
        self.packed = pad == 0 and strides is None

    def view(self):
        rev = lambda x: list(reversed(x)) or [1]   # noqa: E731
        v = self.buf.as_strided(rev(self.extents), rev(self.strides), self.start)
        return v.permute(*reversed(range(v.dim()))) if self.extents else v.reshape(())

    def set(self, host):
        self.view().copy_(host.to(self.buf.device))

    def get(self):
        return self.view().cpu()

    def refill_nan(self):
        self.raw.fill_(0xFF)

    def check_outside(self, what):
        """every byte outside the tensor's own elements still 0xFF"""
        import torch
        inside = torch.zeros(self.buf.numel(), dtype=torch.bool, device=self.buf.device)
        rev = lambda x: list(reversed(x)) or [1]   # noqa: E731
        inside.as_strided(rev(self.extents), rev(self.strides), self.start).fill_(True)
        touched = (self.raw.view(-1, self.es) != 0xFF).any(dim=1) & ~inside
        assert not bool(touched.any()), "%s: %d elements outside D written; the first at element %d (D starts at %d)" % (
            what, int(touched.sum()), int(torch.nonzero(touched)[0]), self.start)


# ---- running a case ----------------------------------------------------------------------------------------------------------------------
_DATA = {}          # data_key, draw -> (A, B, C host tensors; their device copies; references by (alpha, beta))
STATS = []          # (data type, K, accumulator bound as a fraction of its limit, share of outputs that round) of every run, for the report


def _dt(ct, name):
    return {"bfloat16": ct.R_16BF, "float16": ct.R_16F, "float32": ct.R_32F, "float64": ct.R_64F, "complex64": ct.C_32F, "complex128": ct.C_64F}[name]


def _data(case, swap, make=xd.make_exact):
    key = (case.data_key, swap, case.pad[:2], case.off, make.__name__)
    if key not in _DATA:
        if len(_DATA) >= 2:
            _DATA.clear()
        A, B, C = make(case, swap)
        frac = xd.check_draw(case, A, B, C, swap)
        pa, pb = Placed(case.extents(case.modes[0]), case.dtype, case.pad[0], case.off), Placed(case.extents(case.modes[1]), case.dtype, case.pad[1], case.off)
        pa.set(A)
        pb.set(B)
        _DATA[key] = dict(host=(A, B, C), dev=(pa, pb), frac=frac, ref={})
    return _DATA[key]


def _plan(ct, ops, h, case):
    e, m = case.extents, case.modes
    import guarded as gd
    kw = dict(workspace_limit=case.ws_limit)
    if case.algo is not None:
        kw["algo"] = case.algo
    st = [gd.packed_strides(e(m[i]), case.pad[i]) for i in range(3)]
    conj = [ct.OP_CONJ if c else ct.OP_IDENTITY for c in (case.conjA, case.conjB, case.conjC)]
    return ops.contraction_plan(h, e(m[0]), m[0], e(m[1]), m[1], e(m[2]), m[2], dtype=_dt(ct, case.dtype), strideA=st[0], strideB=st[1], strideC=st[2],
                                alignment=case.align or 128, opA=conj[0], opB=conj[1], opC=conj[2], **kw)


def plan_path(ct, ops, h, case):
    """the case's plan is on the path the case covers (the planner needs no GPU)"""
    with wc.hook_env(case):
        plan = _plan(ct, ops, h, case) if case.kind == "contraction" else wc.make_plan(ct, ops, h, case)
    try:
        d = wc.describe(ct, plan)
        assert case.expect(d), "%s is off its path: %s" % (case.id, d)
    finally:
        plan.destroy()
    return d


def run_contraction_case(ct, ops, h, case, make=xd.make_exact, expect=xd.expected, stats=None):
    """`make` draws the data and `expect` turns the exact reference into (what a correct kernel stores, a figure for the report): the
    exact regime of tests/exact_data.py unless given (tests/rounding_data.py: the rounding regime, with a report of its own in `stats`)"""
    import torch
    stats = STATS if stats is None else stats
    with wc.hook_env(case):
        plan = _plan(ct, ops, h, case)
    try:
        d = wc.describe(ct, plan)
        assert case.expect(d) and case.gpu_expect(d), "%s is off its path: %s" % (case.id, d)
        ws = torch.empty(max(plan.required_workspace, 256), dtype=torch.uint8, device="cuda")
        for swap in (False, True):
            dat = _data(case, swap, make)
            A, B, C = dat["host"]
            pa, pb = dat["dev"]
            rk = (case.alpha, case.beta, case.conjA, case.conjB, case.conjC)
            if rk not in dat["ref"]:
                ref = xd.exact_reference(case, A, B, C, device="cuda")
                dat["ref"][rk] = expect(case, ref)
            want, share = dat["ref"][rk]
            pd = Placed(case.extents(case.modes[2]), case.dtype, case.pad[2], case.off)          # D: NaN everywhere
            pc = None
            if case.beta:
                pc = Placed(case.extents(case.modes[2]), case.dtype, case.pad[2], case.off)
                pc.set(C)
            plan.contract(case.alpha, pa.ptr, pb.ptr, case.beta, pc.ptr if pc else 0, pd.ptr, ws.data_ptr(), plan.required_workspace)
            torch.cuda.synchronize()
            what = "%s (draw %d) %s" % (case.id, int(swap), d)
            xd.assert_exact(pd.get(), want, what)
            pd.check_outside(what)
            m = xd.Modes(*case.modes[:3])
            stats.append((case.dtype, int(xd.np.prod([case.ext[c] for c in m.K])) if m.K else 1, dat["frac"], share))
    finally:
        plan.destroy()
    return d


def run_trinary_case(ct, ops, h, case):
    """D[abe] = alpha A[acd] B[cb] C[de] + beta D: fp32, every product and partial sum an integer below 2^24"""
    import numpy as np
    import torch
    mA, mB, mC, mD = case.modes
    plan = wc.make_plan(ct, ops, h, case)
    try:
        d = wc.check_path(ct, case, plan)
        for swap in (False, True):
            rng = np.random.default_rng([77, int(swap)])
            vals = np.array([-3, -2, -1, 1, 2, 3])
            X = [vals[rng.integers(0, 6, size=case.extents(m))] for m in (mA, mB, mC)]
            E = rng.integers(-3, 4, size=case.extents(mD))
            bound = np.einsum("%s,%s,%s->%s" % (mA, mB, mC, mD), *[np.abs(x) for x in X], optimize=True).max()
            assert abs(case.alpha) * bound + 3 * abs(case.beta) < 2.0 ** 24, bound
            ref = case.alpha * np.einsum("%s,%s,%s->%s" % (mA, mB, mC, mD), *X, optimize=True) + case.beta * E
            dev = [Placed(case.extents(m), case.dtype) for m in (mA, mB, mC)]
            for p, x in zip(dev, X):
                p.set(torch.from_numpy(x).to(p.tdt))
            pe, pd = Placed(case.extents(mD), case.dtype), Placed(case.extents(mD), case.dtype)
            pe.set(torch.from_numpy(E).to(pe.tdt))
            ws = torch.empty(max(plan.required_workspace, 256), dtype=torch.uint8, device="cuda")
            plan.contract_trinary(case.alpha, dev[0].ptr, dev[1].ptr, dev[2].ptr, case.beta, pe.ptr, pd.ptr, ws.data_ptr(), plan.required_workspace)
            torch.cuda.synchronize()
            want, share = xd.expected(case, torch.from_numpy(ref.astype(np.float64)))
            xd.assert_exact(pd.get(), want, "%s (draw %d) %s" % (case.id, int(swap), d))
            pd.check_outside(case.id)
            STATS.append((case.dtype, case.ext["c"] * case.ext["d"], float(abs(case.alpha) * bound + 3) / 2.0 ** 24, share))
    finally:
        plan.destroy()
    return d


def blocksparse_inputs(case, swap):
    """dense draws of the summed extents (checked as such), then zeros where a block is absent"""
    dense = Case(case.id, case.dtype, {c: sum(v) for c, v in case.ext.items()}, case.modes, alpha=case.alpha, beta=case.beta)
    A, B, C = xd.make_exact(dense, swap)
    frac = xd.check_draw(dense, A, B, C, swap)
    lay = [wc.BlockLayout(case.ext, m, c) for m, c in zip(case.modes, case.blocks)]
    A, B = (lay[i].dense([x[sl] for sl in lay[i].slices], list(x.shape)) for i, x in enumerate((A, B)))
    return dense, lay, A, B, C, frac


def run_blocksparse_case(ct, ops, h, case):
    import torch
    import guarded as gd
    plan = wc.make_plan(ct, ops, h, case)
    try:
        d = wc.check_path(ct, case, plan)
        for swap in (False, True):
            dense, lay, A, B, C, frac = blocksparse_inputs(case, swap)
            dev = [[gd.packed_device(x[sl]) for sl in lay[i].slices] for i, x in enumerate((A, B))]
            Cb, Db = wc.GuardedBlocks(lay[2], case.dtype), wc.GuardedBlocks(lay[2], case.dtype)
            Cb.set(C)
            ws = torch.empty(max(plan.required_workspace, 256), dtype=torch.uint8, device="cuda")
            wc._execute(case, plan, dev, Cb, Db, case.beta, ws.data_ptr(), plan.required_workspace)
            torch.cuda.synchronize()
            want, share = xd.expected(dense, xd.exact_reference(dense, A, B, C))
            xd.assert_exact(Db.get(), torch.cat([want[sl].reshape(-1) for sl in lay[2].slices]), "%s (draw %d) %s" % (case.id, int(swap), d))
            Db.check_guard(case.id)
            STATS.append((case.dtype, sum(case.ext["k"]) * sum(case.ext["l"]), frac, share))
    finally:
        plan.destroy()
    return d


def run_case(ct, ops, h, case):
    return {"contraction": run_contraction_case, "contraction_trinary": run_trinary_case, "blocksparse": run_blocksparse_case}[case.kind](ct, ops, h, case)


def sweep(ct, ops, h, problems, tag, ranks=None, **case_kw):
    """every ranked candidate (kernel, split-K) of every problem (or the first `ranks`); returns the kernel indices and names seen and
    whether a split-K plan was among them"""
    seen, names, split = set(), set(), False
    for i, (ext, mA, mB, mC) in enumerate(problems):
        n = ranks
        if n is None:
            p0 = ops.contraction_plan(h, [ext[c] for c in mA], mA, [ext[c] for c in mB], mB, [ext[c] for c in mC], mC, workspace_limit=1 << 28)
            n = ct.lib.ctamdCountCandidates(h.h, p0.op, 1 << 28)
            p0.destroy()
        assert n > 0, (tag, i)
        for r in range(n):
            d = run_contraction_case(ct, ops, h, sweep_case(problems, tag, i, r, **case_kw))
            seen.add(d.get("kernel"))
            names.add(d.get("kname"))
            split |= d.get("splitK", 1) > 1
    return seen, names, split


def report(stats):
    """per data type: runs, largest K, largest accumulator bound (fraction of its limit), largest share of outputs that round"""
    out = {}
    for dt, k, frac, share in stats:
        n, mk, mf, ms = out.get(dt, (0, 0, 0.0, 0.0))
        out[dt] = (n + 1, max(mk, k), max(mf, frac), max(ms, share))
    return out


def _stop(why):
    """a child that hung or died of a signal may have left the GPU in a bad state: end the whole session instead of starting the next test on it"""
    import pytest
    pytest.exit(why, returncode=3)


def in_child(ids, env, timeout, mode="run", script="exact_cases.py"):
    """`python exact_cases.py MODE ids...` (or another case table's script) in a fresh process with its own time limit; returns the child's output"""
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    child_env = dict(os.environ, PYTHONPATH=os.pathsep.join([root, here]), **env)
    try:
        r = subprocess.run([sys.executable, os.path.join(here, script), mode] + list(ids), capture_output=True, text=True, timeout=timeout,
                           env=child_env, cwd=root)
    except subprocess.TimeoutExpired as e:
        _stop("a child (%s %s) ran into its time limit of %d s\n%s" % (mode, env, timeout, (e.stdout or b"")[-2000:]))
    if r.returncode < 0 or r.returncode in (134, 139):
        _stop("a child (%s %s) died of signal %d\n%s\n%s" % (mode, env, r.returncode, r.stdout[-2000:], r.stderr[-4000:]))
    assert r.returncode == 0, "child exit %d\n%s\n%s" % (r.returncode, r.stdout[-3000:], r.stderr[-6000:])
    assert r.stdout.count("ok ") == len(ids), r.stdout[-3000:]
    if "REPORT " in r.stdout:
        import json
        STATS.extend(tuple(x) for x in json.loads(r.stdout.split("REPORT ", 1)[1].splitlines()[0]))
    return r.stdout


if __name__ == "__main__":
    from cudalibrarysamples_amd import cutensor as ct_, ops as ops_
    mode_ = sys.argv[1]
    if mode_ == "production":
        assert os.environ.get("CTAMD_LIB_FLAVOUR") != "hooks" and "lib_hooks" not in ct_.LIB_PATH, ct_.LIB_PATH
    h_ = ops_.Handle()
    if mode_ == "nt_sweep":
        seen_, _, _ = sweep(ct_, ops_, h_, NT_PROBLEMS, "nt")
        print("KERNELS", sorted(seen_))
    for cid in sys.argv[2:]:
        if mode_ == "plan":
            plan_path(ct_, ops_, h_, BY_ID[cid])
        else:
            run_case(ct_, ops_, h_, BY_ID[cid])
        print("ok", cid, flush=True)
    import json
    print("REPORT", json.dumps(STATS))
