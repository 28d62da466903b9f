"""One table of plan-only cuTENSORMg contraction cases: the layouts the CPU tests of the multi-device path plan (tests/test_mg_plan_cpu.py,
tests/test_mg_replay_cpu.py), each with the handle size, the environment switches it is planned under and its data type.  The layout
builders live here and the tests import them; tools/gen_mg_plan_descriptions.py describes every case of CASES into
tests/golden/mg_plan_descriptions.json.gz and tests/test_mg_plan_descriptions_cpu.py compares every later library with that file.

A case is planned on a plan-only handle (no GPU visible) over the device ids 0 .. n - 1.  `describe_raw` returns ctamdMgDescribePlan's
text as the library wrote it, or, for a plan the library refuses, the JSON object {"status": <cutensorStatus_t>}."""
import collections
import contextlib
import math
import os

import numpy as np

Case = collections.namedtuple("Case", "id n modes extent block dcount env dtype compute")

HIP_R_32F, HIP_R_64F, HIP_R_16BF = 0, 1, 14
COMPUTE_32F, COMPUTE_64F = 1 << 2, 1 << 4
MATMUL = ["ik", "kj", "ij"]


def free_mode_layout(n, E):
    """The layout bench.py uses for the cuTENSORMg case: C[i,j] = A[i,k] B[k,j] with the largest free mode i cut n ways
    (A and C hold row slabs), B distributed along j (column slabs) — every device needs all of B: the all-gather."""
    modes = ["ik", "kj", "ij"]
    extent = dict(i=E, j=E, k=E)
    block = [dict(i=E // n), dict(j=E // n), dict(i=E // n, j=E // n)]
    dcount = [dict(i=n), dict(j=n), dict(i=n)]
    return modes, extent, block, dcount


def sample_block_cyclic_layout(E, BS):
    """contraction_multi_gpu.cu:154-217: 2 x 2 block-cyclic descriptors of C[i,j] = A[i,k] B[k,j]."""
    block = [dict(i=BS, k=BS), dict(k=BS, j=BS), dict(i=BS, j=BS)]
    dcount = [dict(i=2, k=2), dict(k=2, j=2), dict(i=2, j=2)]
    return list(MATMUL), dict(i=E, j=E, k=E), block, dcount


def ragged_free_mode_layout(seed):
    """Seeded random block-cyclic layout over 2-4 devices whose FREE extents do not divide the block size -> (n, modes, extent, block, dcount)"""
    rng = np.random.default_rng(100 + seed)
    n = int(rng.choice([2, 3, 4]))
    Ei, Ej, Ek = (int(rng.integers(40, 200)) for _ in range(3))
    bi, bj = int(rng.integers(8, 48)), int(rng.integers(8, 48))
    di = n
    dj = int(rng.choice([1, 2])) if n % 2 == 0 else 1
    block = [dict(i=bi), dict(j=bj), dict(i=bi, j=bj)]
    dcount = [dict(i=di), dict(j=dj), dict(i=di, j=dj)]
    return n, list(MATMUL), dict(i=Ei, j=Ej, k=Ek), block, dcount


def ragged_block_cyclic_layout(seed):
    """Seeded random block-cyclic layout over 2-4 devices, ragged in free AND contracted modes -> (n, modes, extent, block, dcount, beta)"""
    rng = np.random.default_rng(300 + seed)
    n = int(rng.choice([2, 3, 4]))
    Ei, Ej, Ek = (int(rng.integers(20, 70)) for _ in range(3))
    bi, bj, bk = (int(rng.integers(4, 20)) for _ in range(3))
    di = n
    dj = int(rng.choice([1, 2])) if n % 2 == 0 else 1
    dk = int(rng.choice([1, 2]))
    block = [dict(i=bi, k=bk), dict(k=bk, j=bj), dict(i=bi, j=bj)]
    dcount = [dict(i=di, k=dk), dict(k=dk, j=dj), dict(i=di, j=dj)]
    beta = float(rng.choice([0.0, 1.5]))
    return n, list(MATMUL), dict(i=Ei, j=Ej, k=Ek), block, dcount, beta


def ragged_contracted_layout(k):
    """k in blocks of 32 over 2 devices (k = 176: 5.5 blocks, padded to 6; k = 192 fills its padded space)"""
    block = [dict(i=32, k=32), dict(k=32, j=32), dict(i=32, j=32)]
    dcount = [dict(i=2, k=2), dict(k=2, j=2), dict(i=2, j=2)]
    return list(MATMUL), dict(i=128, j=128, k=k), block, dcount


def _blog_post_shapes(n, s):
    """cuTENSORMg/blog_post.cu:155-175 (extents, ceil()-derived block sizes — including its N1 expression as written) and
    :78-101 (device counts: from the last mode down, double while blocks and devices remain)."""
    M0, M1, M2, N0, N1, N2, K0, K1, K2 = "abcdefghi"
    ext = {M0: 16, M1: 8 * s, M2: 8, N0: 16, N1: 8 * s, N2: 8, K0: 16, K1: 32, K2: 8}
    nM = n // 2 if n >= 4 else n
    nN = n // nM
    M = ext[M0] * ext[M1] * ext[M2]
    N = ext[N0] * ext[N1] * ext[N2]
    bs = {M0: 16, M2: 8, N0: 16, N2: 8, K0: 16, K1: 16, K2: 8}
    bs[M1] = math.ceil(math.ceil(M / math.ceil(M / 4096.0 / nM)) / nM / ext[M0] / ext[M2])
    bs[N1] = math.ceil(math.ceil(N / math.ceil(N / 4096.0 / nN)) / nN / ext[N0] / ext[N1])
    modes = [K0 + M0 + M1 + K1 + M2 + K2, K0 + N0 + K1 + N1 + K2 + N2, M0 + N0 + M1 + N1 + M2 + N2]
    block, dcount = [], []
    for m in modes:
        dc = {c: 1 for c in m}
        rem, changed = n, True
        while changed:
            changed = False
            for c in reversed(m):
                if rem <= 1:
                    break
                if dc[c] < ext[c] // bs[c]:
                    dc[c] *= 2
                    rem //= 2
                    changed = True
        assert rem == 1 or n == 1 or all(dc[c] >= ext[c] // bs[c] for c in m)
        block.append({c: bs[c] for c in m})
        dcount.append(dc)
    return modes, ext, block, dcount


def _case(id, n, layout, env=None, dtype=HIP_R_32F, compute=COMPUTE_32F):
    modes, extent, block, dcount = layout
    return Case(id, n, modes, extent, block, dcount, dict(env or {}), dtype, compute)


def _cases():
    for n in (2, 4, 8):
        yield _case("free_mode-n%d" % n, n, free_mode_layout(n, 128 * n))
    for n, waves in ((4, 3), (8, 7), (8, 2)):
        yield _case("waves-n%d-w%d" % (n, waves), n, free_mode_layout(n, 64 * n), env={"CUTENSORMG_AMD_WAVES": str(waves)})
    for n in (1, 2, 4, 8):
        yield _case("sample_2x2-n%d" % n, n, sample_block_cyclic_layout(256, 64))
    for seed in range(6):
        yield _case("ragged_free-seed%d" % seed, ragged_free_mode_layout(seed)[0], ragged_free_mode_layout(seed)[1:])
    for seed in range(6):
        yield _case("ragged_block_cyclic-seed%d" % seed, ragged_block_cyclic_layout(seed)[0], ragged_block_cyclic_layout(seed)[1:5])
    for k in (176, 192):
        yield _case("ragged_contracted-k%d" % k, 2, ragged_contracted_layout(k))
    for n in (1, 2, 4, 8):
        for s in range(1, 13):
            yield _case("blog_post-n%d-s%d" % (n, s), n, _blog_post_shapes(n, s))
    for n in (1, 2, 4):
        for transport in ("", "allgather", "sendrecv"):
            env = {"CUTENSORMG_AMD_FORCE_GATHER": "1", "CUTENSORMG_AMD_ASSUME_RCCL": "1"}
            if transport:
                env["CUTENSORMG_AMD_TRANSPORT"] = transport
            yield _case("forced_gather-n%d-%s" % (n, transport or "auto"), n, free_mode_layout(n, 32 * n), env=env)
    # RCCL assumed (all-gather transport of the free-mode layout; send/recv for the sample's layout), and the peer transport without it
    for n in (2, 4, 8):
        yield _case("rccl_free_mode-n%d" % n, n, free_mode_layout(n, 128 * n), env={"CUTENSORMG_AMD_ASSUME_RCCL": "1"})
    yield _case("rccl_sample_2x2-n4", 4, sample_block_cyclic_layout(256, 64), env={"CUTENSORMG_AMD_ASSUME_RCCL": "1"})
    yield _case("peer_transport-n4", 4, free_mode_layout(4, 128 * 4), env={"CUTENSORMG_AMD_TRANSPORT": "peer"})
    for switch in ("QSPLIT", "SHARD2", "DIRECT", "PEEL"):
        env = {"CUTENSORMG_AMD_" + switch: "0"}
        yield _case("free_mode-n8-%s0" % switch.lower(), 8, free_mode_layout(8, 128 * 8), env=env)
        yield _case("blog_post-n8-s2-%s0" % switch.lower(), 8, _blog_post_shapes(8, 2), env=env)
    yield _case("sample_2x2-n2-fp64", 2, sample_block_cyclic_layout(256, 64), dtype=HIP_R_64F, compute=COMPUTE_64F)
    yield _case("ragged_contracted-k176-bf16", 2, ragged_contracted_layout(176), dtype=HIP_R_16BF)      # refused: the status is recorded


CASES = list(_cases())
assert len({c.id for c in CASES}) == len(CASES)


@contextlib.contextmanager
def case_environment(case):
    """The process environment with exactly the case's CUTENSORMG_AMD_* switches set (plans read them at handle and plan creation)."""
    saved = {k: v for k, v in os.environ.items() if k.startswith("CUTENSORMG_AMD_")}
    for k in saved:
        del os.environ[k]
    os.environ.update(case.env)
    try:
        yield
    finally:
        for k in case.env:
            os.environ.pop(k, None)
        os.environ.update(saved)


def describe_raw(cm, case):
    """ctamdMgDescribePlan of the case's plan, as text; {"status":N} for a plan the library refuses"""
    from cudalibrarysamples_amd import cutensor as ct
    with case_environment(case):
        try:
            con = cm.Contraction(list(range(case.n)), case.modes, case.extent, case.block, case.dcount, dtype=case.dtype, compute=case.compute)
        except ct.CuTensorError as e:
            return '{"status":%d}' % e.status
        with con:
            return cm.describe_plan_raw(con.plan)
