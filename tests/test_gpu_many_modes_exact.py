"""Element-wise operations and reductions on tensors of many modes, bit for bit on integer-valued data (the case table, the buffers and
the checks are tests/many_mode_cases.py; tests/test_many_modes_cpu.py checks the table and replays every plan's index arithmetic on the
CPU): the mode-table kernels of kernels/elementwise_table.hip behind cutensorPermute, cutensorElementwiseBinaryExecute and
cutensorReduce.  Every case names its kernel with a predicate on the plan's description; D is compared with zero tolerance, everything
outside D's elements must still be NaN, A and a separate C must be unchanged.  Before these kernels existed every case here was refused
at cutensorCreatePermutation / ElementwiseBinary / Reduction with NOT_SUPPORTED."""
import pytest

import exact_cases as xc
import many_mode_cases as mm
import stream_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(built):
    import torch
    assert torch.cuda.is_available()
    from cudalibrarysamples_amd import cutensor as ct, ops
    return ct, ops, ops.Handle()


@pytest.mark.parametrize("cid", mm.NO_SWITCH)
def test_many_modes_exact(env, cid):
    ct, ops, h = env
    mm.run_case(ct, ops, h, mm.BY_ID[cid])


def test_the_gather_kernel_where_the_tile_kernel_applies(env):
    """rev12 once more under CUTENSOR_AMD_EW_TABLE=gather, in a child process: the predicate separates the two kernels"""
    xc.in_child([mm.REV12_GATHER.id], mm.GATHER, timeout=300, script="many_mode_cases.py")


def test_many_modes_exact_on_the_production_libraries(env):
    """the table once more on lib/ (the suite loads lib_hooks/), in one child with its own time limit"""
    xc.in_child(mm.NO_SWITCH, {"CTAMD_LIB_FLAVOUR": "production"}, timeout=600, mode="production", script="many_mode_cases.py")


def test_25_modes_three_of_them_to_the_front(env):
    """the 25-mode extent-2 tensor of the reference's contraction_jit.cu, 128 MiB of fp32: modes f, m and t move to the front of the
    others — seven groups after fusion, one more than the tiled kernels describe"""
    import torch
    ct, ops, h = env
    m = mm.M25
    plan = ops.permutation_plan(h, [2] * 25, m, [2] * 25, mm.FRONT3_D)
    try:
        d = ct.describe_plan(plan.plan)
        assert d["kname"] == "ew_table_tile_kernel" and d["modes"] == 7, d
        x = torch.randint(-3, 4, (1 << 25,), device="cuda").to(torch.float32)
        out = torch.full((1 << 25,), float("nan"), device="cuda")
        plan.permute(1.0, x.data_ptr(), out.data_ptr())
        torch.cuda.synchronize()
        # A's groups, slowest first: [uvwxy] t [nopqrs] m [ghijkl] f [abcde]; D's: [uvwxy] [nopqrs] [ghijkl] [abcde] t m f
        want = x.view(32, 2, 64, 2, 64, 2, 32).permute(0, 2, 4, 6, 1, 3, 5).contiguous().view(-1)
        assert torch.equal(out, want)
    finally:
        plan.destroy()


@pytest.mark.parametrize("eq", ["abcdefgh->hgfedcba", "abcdefghij->acegi"])
def test_einsum_with_one_operand_of_many_modes(env, eq):
    """torch_einsum.einsum — Einsum<float> behind it — goes through cutensorCreateReduction: a reversal of eight modes, and five of ten
    modes summed away.  Integer-valued data: the comparison with torch is exact."""
    import torch
    from cudalibrarysamples_amd import torch_einsum
    lhs = eq.split("->")[0]
    shape = [3 if c in "ch" else 2 for c in lhs]
    x = torch.randint(-3, 4, shape, device="cuda").to(torch.float32)
    got = torch_einsum.einsum(eq, x)
    plan = torch_einsum.EinsumPlan(eq, x.shape, (), x.dtype)
    raw = plan.describe() if hasattr(plan, "describe") else None
    torch.cuda.synchronize()
    want = torch.einsum(eq, x)
    assert got.shape == want.shape and torch.equal(got, want)
    if raw is not None:
        assert "table" in raw.get("kname", ""), raw


@pytest.mark.parametrize("cid", ["f32_perm_rev12", "f32_red_alt10_add"])
def test_gated_many_mode_calls_keep_stream_order(env, cid):
    """one permutation and one reduction through the gate of tests/stream_cases.py: the call returns while its stream is still held up
    (no host wait) and runs behind the work queued before it (stream order)"""
    ct, ops, h = env
    case = mm.BY_ID[cid]
    for run in case.runs[-1:]:
        p = sc.prepare_ew(ct, ops, h, case, run)
        try:
            for k in (0, 1):
                sc.gated([(p, k, sc.side_stream(0))])
        finally:
            p.close()
