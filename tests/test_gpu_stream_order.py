"""Stream order and asynchrony of every execute entry point (the harness and the case table are tests/stream_cases.py).

Every multi-launch plan kind runs once per draw on a side stream that is blocked while the call is made: the real inputs reach their
buffers only after a gate event that the host finds unsignalled when the call has returned, the buffers and the workspace hold 0xFF before
and after, and D's snapshot on the same stream must be the exact result.  A launch that forgot its `stream` argument, or a host
synchronisation inside an execute path, fails the case; a gate that is open fails it as inconclusive.

    test_control_*           the harness fails when the library is handed the null stream (else this file proves nothing)
    test_gated_*             one case per launch sequence: contractions, reductions, permutations, element-wise forms; switches in children
    test_captured_*          the multi-launch kinds captured in a graph on S and replayed twice on the second draw's data
    test_one_plan_*          one plan object on two gated streams with operands, outputs and workspaces of their own
    test_einsum_*            the einsum front end under `with torch.cuda.stream(S)`; one workspace per (device, stream)

Measured on an MI355X (the ENQUEUE lines of `pytest -s`; test_zz_enqueue_times_and_delay prints the table), time on the host from entry
to return of the gated call:
    element-wise, permutation, reduction + finalize      5 .. 10 us
    single contractions, GETT + fold (every family)      7 .. 17 us;  two-step plans 9 .. 14 us;  trinary contraction 10 us
    peeled plan (4 launches) 29 us; block-sparse 32 us; repack plans 29 .. 32 us; persistent 16-bit kernel 19 us
    einsum() split-K 37 us, unary 13 .. 14 us; EinsumFunction forward + backward 383 us (the largest: three einsums and the autograd
    engine's hand-over to its device thread)
The delay is stream_cases.DELAY_MS = 50 ms (the device's events measured 49.9 .. 50.1 ms between the stream's start and the gate), 130
times the largest enqueue time where ten times is asked for; no gate was found open, no case needed its second attempt (200 ms; the cap
is 400 ms).

Not in the table: the in-launch fold.  Under CUTENSOR_AMD_FUSED_FOLD=1 the shrunk headline (a=96, b=16, c=16, d=64, e=96) plans
gett_f32_kernel, split-K 64, "fusedFold":0; the full-size headline gets the fold, and tests/test_gpu_exact.py runs it there."""
import pytest

import exact_cases as xc
import stream_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(built):
    import torch
    assert torch.cuda.is_available()
    from cudalibrarysamples_amd import cutensor as ct, ops
    return ct, ops, ops.Handle(), torch


# ---- 2. the control ---------------------------------------------------------------------------------------------------------------------
def test_control_a_call_on_the_null_stream_is_reported(env):
    ct, ops, h, torch = env
    p = sc.prepare(ct, ops, h, sc.CONTROL)
    try:
        sc.control(p)
        sc.gated([(p, 0, sc.side_stream(0))], "after the control")          # ... and the same buffers pass on the right stream
    finally:
        p.close()


# ---- 3. the case table ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", sc.CONTRACTIONS)
def test_gated_contraction(env, cid):
    ct, ops, h, torch = env
    sc.run_contraction_gated(ct, ops, h, cid)


@pytest.mark.parametrize("group", sorted(sc.CHILDREN))
def test_gated_contraction_under_a_switch(env, group):
    ids, switch = sc.CHILDREN[group]
    out = xc.in_child(ids, switch, timeout=300, script="stream_cases.py")
    sc.parse_times(out)


@pytest.mark.parametrize("cid", [c for c, _ in sc.EW])
def test_gated_reduction_and_elementwise(env, cid):
    ct, ops, h, torch = env
    for case, run in sc.ew_runs(cid):
        p = sc.prepare_ew(ct, ops, h, case, run)
        try:
            for k in (0, 1):
                sc.gated([(p, k, sc.side_stream(0))])
        finally:
            p.close()


def test_gated_padded_permutation(env):
    ct, ops, h, torch = env
    for run in (0, 1):
        p = sc.prepare_padded(ct, ops, h, run)
        try:
            sc.gated([(p, run, sc.side_stream(0))])
        finally:
            p.close()


# ---- 4. capture and replay --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", sc.CAPTURED)
def test_captured_contraction(env, cid):
    ct, ops, h, torch = env
    p = sc.prepare(ct, ops, h, cid)
    try:
        sc.capture_replay(p)
    finally:
        p.close()


@pytest.mark.parametrize("cid,run", sc.EW_CAPTURED)
def test_captured_reduction_and_elementwise(env, cid, run):
    ct, ops, h, torch = env
    (case, r), = sc.ew_runs(cid, run)
    p = sc.prepare_ew(ct, ops, h, case, r)
    try:
        sc.capture_replay(p)
    finally:
        p.close()


def test_captured_padded_permutation(env):
    ct, ops, h, torch = env
    p = sc.prepare_padded(ct, ops, h)
    try:
        sc.capture_replay(p)
    finally:
        p.close()


# ---- 5. one plan, two streams -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", sc.TWO_STREAMS)
def test_one_plan_on_two_streams(env, cid):
    """cannot force the two runs to overlap and cannot fail on a correct library: it is what would show execution state kept in the plan
    or the handle.  Both gates are still closed when the second call has returned, so both runs were queued before either could start."""
    ct, ops, h, torch = env
    p1 = sc.prepare(ct, ops, h, cid)
    try:
        p2 = sc.prepare(ct, ops, h, cid, plan=p1.plan)
        assert p1.ws.data_ptr() != p2.ws.data_ptr() and p1.outs[0].ptr != p2.outs[0].ptr
        sc.gated([(p1, 0, sc.side_stream(0)), (p2, 1, sc.side_stream(1))], "two streams")
    finally:
        p1.close()


# ---- 6. the einsum front end ------------------------------------------------------------------------------------------------------------
def _ints(torch, shape, seed):
    g = torch.Generator()
    g.manual_seed(seed)
    v = torch.tensor([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0], dtype=torch.float64)
    return v[torch.randint(0, 6, shape, generator=g)]


def _einsum_call(torch, tein, eq, hosts, what):
    """hosts: fp64 CPU tensors of integers; the exact expectation by torch.einsum in fp64 on the CPU (every sum below 2^24)"""
    want = torch.einsum(eq, *hosts)
    assert float(torch.einsum(eq, *[x.abs() for x in hosts]).max()) < 2.0 ** 24
    stagings = [x.to(torch.float32).cuda() for x in hosts]
    lives = [torch.empty_like(s) for s in stagings]
    return sc.TorchCall(what, lives, stagings, lambda: [tein.einsum(eq, *lives)], [want])


HEAD_EQ, HEAD_A, HEAD_B = "abcd,dcbe->ae", (96, 16, 16, 64), (64, 16, 16, 96)


@pytest.fixture
def tein(env):
    from cudalibrarysamples_amd import torch_einsum as te
    old = dict(te._workspace)
    te._workspace.clear()
    yield te
    env[3].cuda.synchronize()
    te._workspace.clear()
    te._workspace.update(old)


def test_einsum_split_k_on_a_gated_stream(env, tein):
    torch = env[3]
    call = _einsum_call(torch, tein, HEAD_EQ, [_ints(torch, HEAD_A, 1), _ints(torch, HEAD_B, 2)], "einsum " + HEAD_EQ)
    sc.gated([(call, 0, sc.side_stream(0))])
    plan = tein._plans[(HEAD_EQ, HEAD_A, HEAD_B, torch.float32, False, False)]
    assert plan.describe()["splitK"] > 1 and plan.required_workspace > 0, plan.describe()


@pytest.mark.parametrize("eq", ["nij->ji", "nij->ijn"])
def test_einsum_unary_on_a_gated_stream(env, tein, eq):
    torch = env[3]
    call = _einsum_call(torch, tein, eq, [_ints(torch, (5, 37, 52), 3)], "einsum " + eq)
    sc.gated([(call, 0, sc.side_stream(0))])


def test_einsum_function_forward_and_backward_on_a_gated_stream(env, tein):
    torch = env[3]
    eq = "lik,lkj->lij"
    a, b, g = _ints(torch, (3, 40, 36), 4), _ints(torch, (3, 36, 28), 5), _ints(torch, (3, 40, 28), 6)
    wants = [torch.einsum(eq, a, b), torch.einsum("lij,lkj->lik", g, b), torch.einsum("lik,lij->lkj", a, g)]
    stagings = [x.to(torch.float32).cuda() for x in (a, b, g)]
    lives = [torch.empty_like(s) for s in stagings]
    lives[0].requires_grad_(True)
    lives[1].requires_grad_(True)

    def fn():
        out = tein.EinsumFunction.apply(eq, lives[0], lives[1])
        da, db = torch.autograd.grad(out, (lives[0], lives[1]), lives[2])
        return [out, da, db]

    call = sc.TorchCall("EinsumFunction " + eq, lives, stagings, fn, wants)
    sc.gated([(call, 0, sc.side_stream(0))])


def test_einsum_workspace_is_per_stream(env, tein, monkeypatch):
    """two gated streams, each the split-K einsum on data of its own: the two calls must be handed different workspaces (one growing
    buffer per device would hold the partials of both), and both results are exact"""
    torch = env[3]
    seen = []
    real = tein.EinsumPlan.execute

    def spy(self, a, b, out, workspace):
        seen.append((torch.cuda.current_stream().cuda_stream, workspace.data_ptr() if workspace is not None else 0))
        return real(self, a, b, out, workspace)

    calls = [_einsum_call(torch, tein, HEAD_EQ, [_ints(torch, HEAD_A, 10 + i), _ints(torch, HEAD_B, 20 + i)], "einsum %s stream %d" % (HEAD_EQ, i))
             for i in (0, 1)]
    streams = [sc.side_stream(0), sc.side_stream(1)]
    sc.gated([(calls[0], 0, streams[0])], "alone")                # plans and code objects are there before the spy counts
    monkeypatch.setattr(tein.EinsumPlan, "execute", spy)

    def distinct_workspaces():
        last = {s: p for s, p in seen}                            # the gated calls are the last ones on their streams
        p0, p1 = last[streams[0].cuda_stream], last[streams[1].cuda_stream]
        assert p0 and p1, seen
        assert p0 != p1, "both streams were given the workspace at %#x" % p0

    sc.gated([(c, 0, s) for c, s in zip(calls, streams)], "two streams", before_check=distinct_workspaces)


# ---- the figures ------------------------------------------------------------------------------------------------------------------------
def test_zz_enqueue_times_and_delay():
    """what this session measured (printed: pytest -s): every gated call's time from entry to return, the largest, the delay"""
    if not sc.TIMES:
        return                      # (selected alone: nothing ran)
    for name, t in sorted(sc.TIMES.items(), key=lambda kv: -kv[1]):
        print("enqueue %8.1f us  %s" % (t * 1e6, name))
    print("largest enqueue time %.1f us over %d calls; delay %g ms (measured %.1f .. %.1f ms), cap %g ms" % (
        max(sc.TIMES.values()) * 1e6, len(sc.TIMES), sc.DELAY_MS, min(sc.DELAYS), max(sc.DELAYS), sc.DELAY_CAP_MS))
