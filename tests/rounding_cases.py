"""Which contraction cases run in the rounding regime of tests/rounding_data.py, and how (tests/test_round16_data_cpu.py checks every
draw and plan on the CPU, tests/test_gpu_round16_exact.py runs them) — a helper module, not a conftest.

ROUNDING: every 16-bit case of exact_cases.CASES that is not full-size and has fewer than 1e9 multiply-adds, with its own path predicate,
switches, scalars, offsets and pitches; only the data maker and the comparator differ.  The 16-bit lone-mode cases are left out: the
library reduces a lone mode into a 16-bit temporary first, they round twice by design and tests/test_gpu_exact.py pins that.

BETA: one small case per place that has beta arithmetic of its own, alpha = 1, beta = 2^-14, C odd in [-15, 15]
(rounding_data.expected_beta: fp16 rounds alpha * acc + beta * c once, bf16 after an fp32 fused multiply-add).

Cases whose switch the library reads once per process run in a child: `python rounding_cases.py run|beta|plan_beta ids...`, which prints
its counts behind "ROUNDING" (exact_cases.in_child's own "REPORT" feeds the exact regime's statistics and stays out of it)."""
import json
import sys

import exact_cases as xc
import exact_data as xd
import rounding_data as rd
from workspace_cases import GEN, _family

STATS = []          # (part, data type, case id, rounding_data.counts()) of every run of this process and of its children


def _has_lone(c):
    m = xd.Modes(*c.modes[:3])
    return bool(m.loneA or m.loneB)


ROUNDING = [c for c in xc.CASES if c.dtype in xd.H16 and c.kind == "contraction" and not c.full_size and xd.work(c) < 1e9 and not _has_lone(c)]
ROUNDING_IN_PROCESS = [c.id for c in ROUNDING if c.group is None]
ROUNDING_GROUPS = sorted({c.group for c in ROUNDING if c.group})

BETA = []
SPLITK8 = {"CUTENSOR_AMD_H16_SPLITK": "8"}
W4X_ONE = {"CUTENSOR_AMD_H16_WAVES": "4x", "CUTENSOR_AMD_H16_SPLITK": "1"}


W4M_ONE = {"CUTENSOR_AMD_H16_WAVES": "4m", "CUTENSOR_AMD_H16_SPLITK": "1"}


def _W4X_ONE(d):
    return xc._h16_variant("4x")(d) and d.get("splitK", 1) == 1


def _W4M_ONE(d):
    return xc._h16_variant("4m")(d) and d.get("splitK", 1) == 1


for _dt, _s in (("bfloat16", "bf16"), ("float16", "f16")):
    _kw = dict(alpha=1.0, beta=rd.BETA)
    # The LDS-DMA kernels' epilogue (HEpilogue, gett_h16_common.h).  D is "mn" with m fastest, so the planner swaps the operands and the
    # kernel's N group is {m}.  init() admits 16-byte chunks when the N group's stride in D is 1 and it is ONE mode or its fastest extent
    # is a multiple of 8 (there is no alignment condition); C shares D's strides in these plans, so vecC follows vecD.
    #   chunks:        one N mode -> vecD and vecC: gett_h16w4x_kernel's pipelined chunk path (store_chunk_with_c)
    #   flush_chunks:  the same shape under the 4m variant, whose beta path is flush(): its chunk form with load16 of C
    #   elements:      D is "abn", A is "kba": the N group is {a, b}, which fuse in neither order, and a = 12 is no multiple of 8 ->
    #                  vecD false: flush()'s element-wise form (h_round16_with_c per element)
    # one slice each, so that the kernel's own epilogue adds beta * C and not a fold
    BETA.append(xc.Case("%s_beta_chunks" % _s, _dt, dict(m=256, n=128, k=256), ("mk", "kn", "mn"), _W4X_ONE, env=W4X_ONE, group="h16_4x_one_slice", **_kw))
    BETA.append(xc.Case("%s_beta_elements" % _s, _dt, dict(a=12, b=22, n=129, k=520), ("kba", "kn", "abn"), _W4X_ONE, env=W4X_ONE, group="h16_4x_one_slice",
                        **_kw))
    BETA.append(xc.Case("%s_beta_flush_chunks" % _s, _dt, dict(m=256, n=128, k=256), ("mk", "kn", "mn"), _W4M_ONE, env=W4M_ONE, group="h16_4m_one_slice",
                        **_kw))
    BETA.append(xc.Case("%s_beta_persistent" % _s, _dt, dict(m=256, n=256, k=320), ("mk", "kn", "mn"), xc._kname("gett_h16w4p_kernel"), env=xc.P8,
                        group="h16p_grid8", **_kw))
    # the two split-K folds.  launch_splitk_reduce (gett_f32.hip) takes splitk_reduce_wide_kernel when the kernel's N total is a multiple
    # of four, there are at most 16 slices and 4096 outputs or more; the kernel's N group is {m} (D is "mn", operands swapped):
    # m = 130 -> splitk_reduce_kernel, m = 264 -> splitk_reduce_wide_kernel.  The description's "N" is that total.
    BETA.append(xc.Case("%s_beta_fold" % _s, _dt, dict(m=130, n=264, k=1536), ("km", "kn", "mn"),
                        lambda d: d.get("family") == 1 and d.get("splitK", 1) == 8 and d.get("swapped") == 1 and d.get("N") == 130,
                        env=SPLITK8, group="h16_splitk8", **_kw))
    BETA.append(xc.Case("%s_beta_fold_wide" % _s, _dt, dict(m=264, n=120, k=1536), ("mk", "kn", "mn"),
                        lambda d: d.get("family") == 1 and d.get("splitK", 1) == 8 and d.get("swapped") == 1 and d.get("N") == 264,
                        env=SPLITK8, group="h16_splitk8", **_kw))
    BETA.append(xc.Case("%s_beta_gen" % _s, _dt, dict(m=200, n=136, k=104), ("km", "kn", "mn"), _family(2, "gett_gen_kernel"), env=GEN, group="gen_force", **_kw))
    BETA.append(xc.Case("%s_beta_simple" % _s, _dt, dict(m=137, n=129, k=50, j=3), ("mkj", "jkn", "mn"), xc._kname("gett_simple_kernel"),
                        env={"CUTENSOR_AMD_GEN": "0"}, group="gen0", **_kw))
    # the mode-table kernel (gett_simple.hip's other kernel): the 24-mode problem of exact_cases, no switch
    BETA.append(xc.Case("%s_beta_mode_table" % _s, _dt, xc.WIDE_EXT, (xc.WIDE_A, xc.WIDE_B, xc.WIDE_C), xc._kname("gett_wide_kernel"), ws_limit=None, **_kw))
BETA_BY_ID = {c.id: c for c in BETA}
BETA_GROUPS = sorted({c.group or "in_process" for c in BETA})


def run_rounding(ct, ops, h, case):
    got = []
    xc.run_contraction_case(ct, ops, h, case, make=rd.make_rounding, expect=rd.expected_rounded, stats=got)
    STATS.extend(("contraction", case.dtype, case.id, g[3]) for g in got)


def run_beta(ct, ops, h, case):
    got = []
    xc.run_contraction_case(ct, ops, h, case, make=rd.make_beta, expect=rd.expected_beta, stats=got)
    STATS.extend(("beta", case.dtype, case.id, g[3]) for g in got)


def in_child(ids, env, timeout, mode):
    out = xc.in_child(ids, env, timeout, mode=mode, script="rounding_cases.py")
    if "ROUNDING " in out:
        STATS.extend(tuple(x) for x in json.loads(out.split("ROUNDING ", 1)[1].splitlines()[0]))


if __name__ == "__main__":
    from cudalibrarysamples_amd import cutensor as ct_, ops as ops_
    mode_ = sys.argv[1]
    h_ = ops_.Handle()
    for cid in sys.argv[2:]:
        if mode_ == "plan_beta":
            xc.plan_path(ct_, ops_, h_, BETA_BY_ID[cid])
        elif mode_ == "beta":
            run_beta(ct_, ops_, h_, BETA_BY_ID[cid])
        else:
            run_rounding(ct_, ops_, h_, xc.BY_ID[cid])
        print("ok", cid, flush=True)
    print("ROUNDING", json.dumps(STATS))
