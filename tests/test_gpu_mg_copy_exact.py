"""cutensorMgCopy on the GPU, bit for bit: every case of tests/mg_copy_cases.py with a one-device handle and with a handle that
lists device 0 four times (logical devices: the cells are dealt to the four entries round-robin, every entry launches on a stream of
its own), against the NumPy reference with the poison checks; a call whose cell buffers are not 16-byte aligned; and the chain
scatter -> cutensorMgContraction -> gather, which shows that the layouts the copy writes are the ones the contraction reads."""
import numpy as np
import pytest

from tests import mg_copy_cases as mc

pytestmark = pytest.mark.gpu
HANDLES = [[0], [0, 0, 0, 0]]
_STREAMS = []


@pytest.fixture(scope="module")
def mg(built):
    import torch
    assert torch.cuda.is_available()
    from cudalibrarysamples_amd import cutensormg
    return cutensormg, torch


def streams_for(torch, n):
    while len(_STREAMS) < n:
        _STREAMS.append(torch.cuda.Stream())
    return _STREAMS[:n]


def upload(torch, cells, shift=0):
    """device copies of host cells (as bytes); shift: the cell starts that many bytes into its allocation"""
    out = []
    for x in cells:
        raw = torch.empty(x.nbytes + shift, dtype=torch.uint8, device="cuda")
        raw[shift:].copy_(torch.from_numpy(x.view(np.uint8)))
        out.append(raw[shift:])
    return out


def download(tensors, np_dt):
    return [t.cpu().numpy().view(np_dt) for t in tensors]


def run_copy(cm, torch, plan, D, S):
    n = len(plan.devices)
    ws = [torch.full((max(int(s), 1),), 0xFF, dtype=torch.uint8, device="cuda") for s in plan.ws_sizes]
    streams = streams_for(torch, n)
    torch.cuda.synchronize()
    st = plan.run([t.data_ptr() for t in D], [t.data_ptr() for t in S], [w.data_ptr() for w in ws] if any(plan.ws_sizes) else None,
                  [s.cuda_stream for s in streams])
    assert st == 0, st
    torch.cuda.synchronize()


def run_on_gpu(cm, torch, devices, src, dst, dtype, seed, what, shift=0):
    S, D, W = mc.make_data(src, dst, dtype, seed)
    dS, dD = upload(torch, S, shift), upload(torch, D, shift)
    with cm.CopyPlan(devices, dst.layout(), src.layout(), dtype=mc.DTYPES[dtype][0]) as p:
        d = p.describe()
        run_copy(cm, torch, p, dD, dS)
    got = download(dD, mc.DTYPES[dtype][1])
    mc.check(got, W, dtype, what)
    assert all((a == b).all() for a, b in zip(download(dS, mc.DTYPES[dtype][1]), S)), "%s: the source was written" % what
    return d, got


@pytest.mark.parametrize("devices", HANDLES, ids=["one", "four_logical"])
@pytest.mark.parametrize("case,dtype", mc.RUNS, ids=mc.RUN_IDS)
def test_every_case_is_exact(mg, case, dtype, devices):
    cm, torch = mg
    d, _ = run_on_gpu(cm, torch, devices, case.src, case.dst, dtype, len(devices), "%s %s on %s" % (case.id, dtype, devices))
    assert case.expect(d, dtype), d
    assert d["dstOwners"] == [c % len(devices) for c in range(case.dst.cells)]     # logical devices: round-robin


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_cells_that_are_not_16_byte_aligned_take_element_lanes(mg, dtype):
    """the plan grants 16-byte lanes; this call's cell buffers start 4 (2) bytes past a 16-byte boundary, so the call runs the
    element-lane kernel of the same form — the result is the same"""
    cm, torch = mg
    case = mc.BY_ID["rows_misaligned"]
    d, _ = run_on_gpu(cm, torch, [0, 0], case.src, case.dst, dtype, 3, "rows_misaligned %s shifted" % dtype, shift=mc.ELEM(dtype))
    assert mc.form("rows", 16)(d, dtype)


def test_call_arguments_are_checked(mg):
    """a plan on another handle's device list and a workspace that cannot hold pointers are INVALID_VALUE; nothing is launched"""
    cm, torch = mg
    case = mc.BY_ID["many_cells"]
    S, D, W = mc.make_data(case.src, case.dst, "fp32", 1)
    dS, dD = upload(torch, S), upload(torch, D)
    with cm.CopyPlan([0], case.dst.layout(), case.src.layout()) as p, cm.CopyPlan([0, 0], case.dst.layout(), case.src.layout()) as q:
        ws = torch.empty(int(p.ws_sizes[0]) + 8, dtype=torch.uint8, device="cuda")
        args = (cm.ptr_array([t.data_ptr() for t in dD]), cm.ptr_array([t.data_ptr() for t in dS]))
        stream = cm.ptr_array([streams_for(torch, 1)[0].cuda_stream])
        assert cm.cutensorMgCopy(p.h, p.plan, *args, cm.ptr_array([ws.data_ptr() + 4]), None, stream) == 7
        assert cm.cutensorMgCopy(p.h, p.plan, *args, None, None, stream) == 7
        assert cm.cutensorMgCopy(p.h, q.plan, *args, cm.ptr_array([ws.data_ptr()]), None, stream) == 7
        torch.cuda.synchronize()
        assert all((a == b).all() for a, b in zip(download(dD, np.uint32), D)), "a refused call wrote"
        assert cm.cutensorMgCopy(p.h, p.plan, *args, cm.ptr_array([ws.data_ptr()]), None, stream) == 0
        torch.cuda.synchronize()
    mc.check(download(dD, np.uint32), W, "fp32", "many_cells after the refused calls")


@pytest.mark.parametrize("first,second", mc.ROUND_TRIPS)
def test_scatter_then_gather_gives_back_the_input_bits(mg, first, second):
    cm, torch = mg
    a, b = mc.BY_ID[first], mc.BY_ID[second]
    S, D, W = mc.make_data(a.src, a.dst, "fp32", 11)
    dS, dD = upload(torch, S), upload(torch, D)
    back = upload(torch, mc.aligned_cells(b.dst.cells, b.dst.span, np.uint32, mc.DST_POISON))
    with cm.CopyPlan([0, 0, 0, 0], a.dst.layout(), a.src.layout()) as p, cm.CopyPlan([0, 0, 0, 0], b.dst.layout(), b.src.layout()) as q:
        run_copy(cm, torch, p, dD, dS)
        run_copy(cm, torch, q, back, dD)
    mc.check(download(dD, np.uint32), W, "fp32", first)
    assert (download(back, np.uint32)[0] == S[0]).all()


def test_scatter_contraction_gather_chain(mg):
    """A[i,k] and B[k,j] (256 x 256 fp32, one cell each, first mode fastest) are scattered into the 2 x 2 grid of 64-blocks of
    contraction_multi_gpu.cu's descriptors by cutensorMgCopy, contracted by cutensorMgContraction, and C's cells are gathered into one
    cell: the result is the dense product.  Tolerance as tests/test_gpu_mg.py: rtol 1e-4 against the fp64 product — the operands are in
    [0, 1), so every sum of 256 products carries at most 256 x 2^-24 = 1.5e-5 of itself as fp32 rounding error.  The device is
    synchronised between the steps: this test is about layouts (the ordering of the copy has tests/test_gpu_mg_copy_stream_order.py)."""
    cm, torch = mg
    E, BS, DC, devices = 256, 64, 2, [0, 0, 0, 0]
    rng = np.random.default_rng(5)
    A, B = rng.random((E, E), dtype=np.float32), rng.random((E, E), dtype=np.float32)
    one = lambda m: mc.Side(m, [E, E], [E, E], [1, 1])               # noqa: E731
    grid = lambda m: mc.Side(m, [E, E], [BS, BS], [DC, DC])          # noqa: E731
    cells = {}
    for m, G in (("ik", A), ("kj", B)):
        src = upload(torch, [np.ascontiguousarray(G.ravel(order="F")).view(np.uint32)])
        cells[m] = upload(torch, mc.aligned_cells(DC * DC, grid(m).span, np.uint32, mc.DST_POISON))
        with cm.CopyPlan(devices, grid(m).layout(), one(m).layout()) as p:
            assert mc.form("rows", 16)(p.describe(), "fp32")
            run_copy(cm, torch, p, cells[m], src)
    cells["ij"] = upload(torch, mc.aligned_cells(DC * DC, grid("ij").span, np.uint32, mc.DST_POISON))
    blocks = dict(i=BS, j=BS, k=BS)
    with cm.Contraction(devices, ("ik", "kj", "ij"), dict(i=E, j=E, k=E), [blocks] * 3, [dict(i=DC, j=DC, k=DC)] * 3) as con:
        ws = [torch.empty(int(s), dtype=torch.uint8, device="cuda") for s in con.ws_sizes]
        ptrs = {m: [t.data_ptr() for t in cells[m]] for m in cells}
        torch.cuda.synchronize()
        st = con.run(1.0, ptrs["ik"], ptrs["kj"], 0.0, ptrs["ij"], ptrs["ij"], [w.data_ptr() for w in ws],
                     [s.cuda_stream for s in streams_for(torch, len(devices))])
        assert st == 0, st
        torch.cuda.synchronize()
    out = upload(torch, mc.aligned_cells(1, E * E, np.uint32, mc.DST_POISON))
    with cm.CopyPlan(devices, one("ij").layout(), grid("ij").layout()) as p:
        run_copy(cm, torch, p, out, cells["ij"])
    got = download(out, np.float32)[0].reshape((E, E), order="F")
    np.testing.assert_allclose(got, A.astype(np.float64) @ B.astype(np.float64), rtol=1e-4)
