"""torch_einsum.einsum(..., compute=...) on float32 tensors: the reduced-precision compute descriptors through Einsum<> and the PyTorch
front end, against torch.einsum in fp64 on the CPU with the worst-case bounds of tests/test_gpu_f32x.py."""
import pytest

pytestmark = pytest.mark.gpu

ELEM = {"16BF": 5, "16F": 6, "TF32": 7}


def bound_factor(compute, K):
    head = {"TF32": 3.1 * 2.0 ** -16, "16BF": 2.01 * 2.0 ** -8, "16F": 2.01 * 2.0 ** -11}[compute]
    return head + K * 2.0 ** -23


@pytest.fixture(scope="module")
def env(built):
    import torch
    assert torch.cuda.is_available()
    from cudalibrarysamples_amd import cutensor as ct, torch_einsum
    return ct, torch_einsum, torch


def _draw(torch, gen, compute, shape):
    if compute == "16F":       # +-U(2^-4, 1): away from fp16's subnormal range
        mag = torch.rand(shape, generator=gen, dtype=torch.float64) * (1.0 - 2.0 ** -4) + 2.0 ** -4
        return (mag * (torch.randint(0, 2, shape, generator=gen) * 2 - 1)).to(torch.float32)
    return (torch.rand(shape, generator=gen, dtype=torch.float64) * 2 - 1).to(torch.float32)


@pytest.mark.parametrize("compute", ("16BF", "16F", "TF32"))
@pytest.mark.parametrize("eq,sa,sb,K", [("ik,kj->ij", (192, 256), (256, 160), 256), ("mlik,lkjm->lij", (20, 50, 50, 50), (50, 50, 50, 20), 1000)],
                         ids=["matmul", "multi_mode"])
def test_einsum_with_a_compute_mode(env, monkeypatch, compute, eq, sa, sb, K):
    ct, te, torch = env
    monkeypatch.setenv("CUTENSOR_AMD_F32X", "force")
    gen = torch.Generator().manual_seed(3)
    a, b = _draw(torch, gen, compute, sa), _draw(torch, gen, compute, sb)
    key = (eq, tuple(sa), tuple(sb), torch.float32, False, False, compute)
    te._plans.pop(key, None)                  # (a plan of an earlier test made without the switch)
    before = ct.launch_counts()["gen"]
    got = te.einsum(eq, a.cuda(), b.cuda(), compute=compute)
    torch.cuda.synchronize()
    d = te._plans[key].describe()
    assert d["family"] == 2 and d["elem"] == ELEM[compute] and ct.launch_counts()["gen"] > before, d
    ref = torch.einsum(eq, a.double(), b.double())
    mag = torch.einsum(eq, a.double().abs(), b.double().abs())
    err = (got.cpu().double() - ref).abs()
    print("f32x einsum %s %s: worst err / mag %.3g, bound %.3g" % (compute, eq, float((err / mag).max()), bound_factor(compute, K)))
    assert bool((err <= bound_factor(compute, K) * mag).all())
    te._plans.pop(key, None)


def test_compute_needs_float32_and_is_part_of_the_plan_key(env, monkeypatch):
    ct, te, torch = env
    x = torch.ones(64, 64, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(ValueError):
        te.einsum("ik,kj->ij", x, x, compute="TF32")
    with pytest.raises(ValueError):
        te.einsum("ik,kj->ij", x.float(), x.float(), compute="8F")
    monkeypatch.setenv("CUTENSOR_AMD_F32X", "force")
    a = torch.ones(128, 64, device="cuda")
    b = torch.ones(64, 96, device="cuda")
    base = ("ik,kj->ij", (128, 64), (64, 96), torch.float32, False, False)
    for k in (base, base + ("16BF",)):
        te._plans.pop(k, None)
    te.einsum("ik,kj->ij", a, b)
    out = te.einsum("ik,kj->ij", a, b, compute="16BF")
    assert te._plans[base].describe()["family"] == 0            # (the default plan keeps the key it always had)
    d = te._plans[base + ("16BF",)].describe()
    assert d["family"] == 2 and d["elem"] == 5, d
    assert te._plans[base] is not te._plans[base + ("16BF",)]
    assert bool((out == 64).all())
    # "32F" is the default and shares its plan
    te.einsum("ik,kj->ij", a, b, compute="32F")
    assert base + ("32F",) not in te._plans
    for k in (base, base + ("16BF",)):
        te._plans.pop(k, None)
