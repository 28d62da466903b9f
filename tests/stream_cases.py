"""The gated-stream harness and its case table (tests/test_gpu_stream_order.py runs every case) — a helper module, not a conftest, in
the style of tests/exact_cases.py.

The value tests call the library on the null stream, or on a side stream between two device-wide synchronisations: there a kernel
launched on the wrong stream still gives the right answer.  Here one library call runs on a side stream S (non-blocking with respect to
the null stream, as every torch.cuda.Stream is) that is BLOCKED while the call is made:

    expected result on the default stream (the exact-data makers and references of the value tests); torch.cuda.synchronize()
    every live input (A, B, C where beta != 0, a C that is D included) in an exact_cases.Placed buffer full of 0xFF; the real contents
    wait in device-resident staging copies
    on S:   a delay | gate = Event().record(S) | staging -> live inputs (device to device) | workspace <- 0xFF | THE CALL (stream = S) |
            a snapshot of D's whole raw buffer | live inputs and workspace <- 0xFF
    on the host, right after the call returns: gate.query() must be False
    S.synchronize() — nothing wider; the snapshot equals the exact expectation (exact_data.assert_exact, zero tolerance) and nothing
    outside D's elements was written (Placed.check_outside on the snapshot)

A closed gate after the call proves that everything the call launched was enqueued while S had not reached the inputs' arrival: a launch
on any other stream ran at once, on 0xFF (NaN in every type) inputs or before the GETT whose partials it folds, and its NaN or its missing
result is in the snapshot; and the call did not wait for the device.  A case whose gate is found open is repeated once with four times
the delay and then fails as inconclusive: it never passes and never skips.

Before the gated call the same call runs once on S with the real data, ungated (the runtime loads a kernel's code object at its first
launch: tens of milliseconds that say nothing about the call); everything is poisoned again afterwards.  Every gated call is timed from
entry to return (ENQUEUE lines, TIMES); DELAY_MS is the delay the gate starts with.

Cases whose switch the library reads once per process run in a child: `python stream_cases.py run ids...` (exact_cases.in_child)."""
import copy
import ctypes
import sys
import time

import numpy as np

import convert_cases as cc
import ew_exact_cases as ec
import exact_cases as xc
import exact_data as xd
import workspace_cases as wc

DELAY_MS = 50.0          # the gate's first delay: 130 times the largest enqueue time measured (tests/test_gpu_stream_order.py)
DELAY_CAP_MS = 400.0
TIMES = {}               # what -> the longest time (seconds) the gated call took from entry to return
DELAYS = []              # the delays (ms, as the device's events measured them) the gates stayed closed for
_STREAMS = []            # at most two side streams per process (three with the null stream)


def side_stream(i=0):
    import torch
    assert i < 2
    while len(_STREAMS) <= i:
        _STREAMS.append(torch.cuda.Stream())
    return _STREAMS[i]


# ---- the delay ---------------------------------------------------------------------------------------------------------------------------
class Delay:
    """keeps a stream busy for about `ms`: torch.cuda._sleep with its cycles calibrated once per process against the device's events, or
    (where the sleep kernel is missing or does not last) a chain of 64 MiB device copies"""
    unit = None           # ("sleep", cycles, ms) or ("copy", (src, dst), ms)

    @staticmethod
    def _time(S, fn):
        import torch
        ms = 0.0
        for _ in range(2):                                   # (the first run loads the kernel)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(S):
                e0.record(S)
                fn()
                e1.record(S)
            S.synchronize()
            ms = e0.elapsed_time(e1)
        return ms

    @classmethod
    def calibrate(cls, S):
        import torch
        if cls.unit is not None:
            return
        if hasattr(torch.cuda, "_sleep"):
            n = 1000000
            for _ in range(4):
                ms = cls._time(S, lambda: torch.cuda._sleep(n))
                if ms >= 2.0:
                    break
                n *= 8
            if 2.0 <= ms <= 1000.0:
                cls.unit = ("sleep", n, ms)
                return
        src = torch.zeros(64 << 20, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        cls.unit = ("copy", (src, dst), cls._time(S, lambda: dst.copy_(src)))

    @classmethod
    def enqueue(cls, S, ms):
        """on the current stream (S)"""
        import torch
        cls.calibrate(S)
        kind, x, unit_ms = cls.unit
        if kind == "sleep":
            torch.cuda._sleep(int(x * ms / unit_ms))
        else:
            for _ in range(int(np.ceil(ms / unit_ms))):
                x[1].copy_(x[0])


# ---- one call, ready to be gated ---------------------------------------------------------------------------------------------------------
def snapshot_of(p, snap):
    """the Placed buffer's geometry over a snapshot of its raw bytes"""
    q = copy.copy(p)
    q.raw = snap
    q.buf = snap.view(p.tdt)
    return q


def short_name(what):
    """a call's name without its plan description, in one word (the ENQUEUE lines, TIMES)"""
    return what.split(" {", 1)[0].replace(" ", "_")


def stage(ins, hosts):
    """the real contents of the live inputs as device-resident images of their whole raw buffers (padding and guards 0xFF); the live
    buffers are left full of 0xFF"""
    out = []
    for p, x in zip(ins, hosts):
        p.raw.fill_(0xFF)
        p.set(x)
        out.append(p.raw.clone())
        p.raw.fill_(0xFF)
    return out


class Prepared:
    """one library call on Placed buffers: ins (the live inputs; a C that is D is among them), outs (D — one Placed, or one per block), the
    workspace, launch(stream handle), and per draw the staging images of ins and the expected outs"""

    def __init__(self, what, plan, ins, outs, ws, launch, draws, keep=()):
        self.what, self.plan, self.ins, self.outs, self.ws, self._launch, self.draws, self.keep = what, plan, ins, outs, ws, launch, draws, keep
        self.name = short_name(what)
        self.snaps = None

    def alloc_snapshots(self):
        import torch
        self.snaps = [torch.empty_like(o.raw) for o in self.outs]

    def load(self, k):
        for p, s in zip(self.ins, self.draws[k][0]):
            p.raw.copy_(s, non_blocking=True)

    def poison_inputs(self):
        for p in self.ins:
            p.raw.fill_(0xFF)
        if self.ws is not None:
            self.ws.fill_(0xFF)

    def poison_all(self):
        self.poison_inputs()
        for p in self.outs:
            p.raw.fill_(0xFF)

    def fill_workspace(self):
        if self.ws is not None:
            self.ws.fill_(0xFF)

    def launch(self, stream):
        self._launch(stream)

    def snapshot(self):
        for s, o in zip(self.snaps, self.outs):
            s.copy_(o.raw, non_blocking=True)

    def check(self, k, what=""):
        for i, (o, s, want) in enumerate(zip(self.outs, self.snaps, self.draws[k][1])):
            q = snapshot_of(o, s)
            tag = "%s %s (draw %d%s)" % (self.what, what, k, ", block %d" % i if len(self.outs) > 1 else "")
            xd.assert_exact(q.get(), want, tag)
            q.check_outside(tag)

    def has_nan(self):
        import torch
        return any(bool(torch.isnan(snapshot_of(o, s).get()).any()) for o, s in zip(self.outs, self.snaps))

    def close(self):
        if self.plan is not None:
            self.plan.destroy()
            self.plan = None


class TorchCall:
    """a call of the einsum front end under the same protocol: live torch tensors full of NaN, their staging copies, fn() -> the output
    tensors (it runs on the current stream, which is S), the expected outputs.  One draw."""

    def __init__(self, what, lives, stagings, fn, wants):
        self.what, self.lives, self.stagings, self.fn, self.wants = what, lives, stagings, fn, wants
        self.name = short_name(what)
        self.result = self.snaps = None
        self.poison_all()

    def alloc_snapshots(self):
        pass

    def load(self, k):
        for l, s in zip(self.lives, self.stagings):
            l.detach().copy_(s, non_blocking=True)

    def poison_inputs(self):
        for l in self.lives:
            l.detach().fill_(float("nan"))
            l.grad = None

    poison_all = poison_inputs

    def fill_workspace(self):
        pass

    def launch(self, stream):
        self.result = self.fn()

    def snapshot(self):
        self.snaps = [r.detach().clone() for r in self.result]
        self.result = None

    def check(self, k, what=""):
        assert len(self.snaps) == len(self.wants)
        for i, (s, want) in enumerate(zip(self.snaps, self.wants)):
            xd.assert_exact(s, want, "%s %s (output %d)" % (self.what, what, i))

    def close(self):
        pass


# ---- the protocol ------------------------------------------------------------------------------------------------------------------------
def run_gated(items, delay_ms, lib_stream=None, warm=True):
    """items: (call, draw, stream) — each call behind a delay and a gate of its own on its stream, all enqueued before any stream is
    waited for.  lib_stream: the handle the library is given instead of the call's stream (the control).  Returns per item the seconds
    the call took on the host and whether its gate was still closed when the LAST call had returned."""
    import torch
    for c, k, S in items:
        c.alloc_snapshots()
        if warm:
            with torch.cuda.stream(S):
                c.load(k)
                c.launch(S.cuda_stream)
            S.synchronize()
        c.poison_all()
    for _, _, S in items:
        Delay.calibrate(S)
    torch.cuda.synchronize()
    gates, took = [], []
    for c, k, S in items:
        with torch.cuda.stream(S):
            e0 = torch.cuda.Event(enable_timing=True)
            e0.record(S)
            Delay.enqueue(S, delay_ms)
            gate = torch.cuda.Event(enable_timing=True)
            gate.record(S)
            c.load(k)
            c.fill_workspace()
            t0 = time.perf_counter()
            c.launch(S.cuda_stream if lib_stream is None else lib_stream)
            took.append(time.perf_counter() - t0)
            gates.append((e0, gate))
    closed = [g.query() is False for _, g in gates]
    for c, k, S in items:
        with torch.cuda.stream(S):
            c.snapshot()
            c.poison_inputs()
    for _, _, S in items:
        S.synchronize()
    for (c, _, _), t, (e0, g), ok in zip(items, took, gates, closed):
        print("ENQUEUE %s %.1f us (gate %s, delay %.1f ms)" % (c.name, t * 1e6, "closed" if ok else "OPEN", e0.elapsed_time(g)), flush=True)
        TIMES[c.name] = max(TIMES.get(c.name, 0.0), t)
        DELAYS.append(e0.elapsed_time(g))
    return took, closed


def gated(items, what="", before_check=None):
    """the whole protocol for one call (or several on streams of their own): gate, repeat once at four times the delay, compare.
    before_check(): what the caller asserts once the gates are known to have held, ahead of the comparison"""
    for delay in (DELAY_MS, min(4 * DELAY_MS, DELAY_CAP_MS)):
        took, closed = run_gated(items, delay)
        if all(closed):
            break
    else:
        raise AssertionError("%s: inconclusive — the gate was open when the call returned (the call took %s ms on the host, the delay was %g ms): "
                             "either the call waits for the device, or the host was too slow to prove that it does not" % (
                                 " / ".join(c.what for c, _, _ in items), ["%.2f" % (t * 1e3) for t in took], delay))
    if before_check is not None:
        before_check()
    for c, k, _ in items:
        c.check(k, what)


def control(call, k=0):
    """the harness must be able to fail: the library is given the NULL stream while the inputs arrive late on S.  Every buffer is valid;
    the kernels read 0xFF inputs at once, so D holds NaN when S takes its snapshot."""
    import torch
    S = side_stream(0)
    took, closed = run_gated([(call, k, S)], DELAY_MS, lib_stream=0)
    torch.cuda.synchronize()
    assert closed[0], "%s: inconclusive control — the gate was open when the call returned" % call.what
    try:
        call.check(k, "control")
    except AssertionError:
        assert call.has_nan(), "%s: the control differs from the expectation, but not by the NaN of its poisoned inputs" % call.what
        return
    raise AssertionError("%s: a call on the null stream saw inputs that arrive later on a side stream — the runtime has serialised the "
                         "streams, and no test of this file proves anything" % call.what)


def capture_replay(call):
    """one eager run on S, the call captured on S, then twice: the second draw into the inputs, D and the workspace full of 0xFF, one
    replay, the second draw's exact expectation"""
    import torch
    S = side_stream(0)
    call.alloc_snapshots()
    with torch.cuda.stream(S):
        call.load(0)
        call.launch(S.cuda_stream)
    S.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=S):
        call.launch(S.cuda_stream)
    for rep in range(2):
        with torch.cuda.stream(S):
            call.poison_all()
            call.load(1)
            g.replay()
            call.snapshot()
        S.synchronize()
        call.check(1, "replay %d of the captured call" % rep)
    del g


# ---- contractions ------------------------------------------------------------------------------------------------------------------------
F32X = xc.Case("f32x_splitk_odd", "float32", dict(m=100, n=60, k=4099), ("mk", "kn", "mn"),
               lambda d: d.get("family") == 2 and d.get("kname") == "gett_gen_f32x_kernel" and d.get("elem") == 7 and d.get("splitK", 1) > 1,
               env={"CUTENSOR_AMD_F32X": "force"}, alpha=0.5, beta=-0.5)
F32X.compute, F32X.inplace = "TF32", True
EXTRA = {c.id: c for c in (F32X,)}

CONTRACTIONS = ["f32_rows_multi", "f32_unal_mk_kn_splitk", "bfloat16_lds_splitk", "float64_gen_odd_splitk", "complex64_gen_odd_splitk", "f32x_splitk_odd",
                "f32_lone_AB", "f32_lone_inner_splitk", "bf16_lone_small_sums", "float32_peeled", "float32_mode_table", "f32_trinary_contraction",
                "f64_blocksparse"]
# (no in-launch fold: under CUTENSOR_AMD_FUSED_FOLD=1 the shrunk headline a=96, b=16, c=16, d=64, e=96 plans gett_f32_kernel with split-K 64 and
# "fusedFold":0 — the fold is offered to the kernels with fragment partials only, and this shape is not given one)
CHILDREN = {"repack": (["float32_repack", "bf16_repack_both"], wc.REPACK), "h16p_grid8": (["bfloat16_h16p_grid8_3"], xc.P8)}
CAPTURED = ["f32_unal_mk_kn_splitk", "bfloat16_lds_splitk", "float64_gen_odd_splitk", "f32_lone_AB", "float32_peeled", "f32_trinary_contraction"]
TWO_STREAMS = ["f32_unal_mk_kn_splitk", "bfloat16_lds_splitk", "float32_peeled"]
CONTROL = "f32_unal_mk_kn_splitk"


def case_of(cid):
    return EXTRA[cid] if cid in EXTRA else xc.BY_ID[cid]


def _contraction_plan(ct, ops, h, case):
    import guarded as gd
    e, m = case.extents, case.modes
    kw = dict(workspace_limit=case.ws_limit)
    if getattr(case, "compute", None):
        kw["compute"] = case.compute
    st = [gd.packed_strides(e(m[i]), case.pad[i]) for i in range(3)]
    conj = [ct.OP_CONJ if c else ct.OP_IDENTITY for c in (case.conjA, case.conjB, case.conjC)]
    return ops.contraction_plan(h, e(m[0]), m[0], e(m[1]), m[1], e(m[2]), m[2], dtype=xc._dt(ct, case.dtype), strideA=st[0], strideB=st[1],
                                strideC=st[2], alignment=case.align or 128, opA=conj[0], opB=conj[1], opC=conj[2], **kw)


def _workspace(plan):
    import torch
    return torch.full((max(plan.required_workspace, 256),), 0xFF, dtype=torch.uint8, device="cuda")


def prepare_contraction(ct, ops, h, case, plan=None):
    own = plan is None
    if own:
        with wc.hook_env(case):
            plan = _contraction_plan(ct, ops, h, case)
    d = wc.describe(ct, plan)
    assert case.expect(d) and case.gpu_expect(d), "%s is off its path: %s" % (case.id, d)
    e, m = case.extents, case.modes
    pa, pb = xc.Placed(e(m[0]), case.dtype, case.pad[0], case.off), xc.Placed(e(m[1]), case.dtype, case.pad[1], case.off)
    pd = xc.Placed(e(m[2]), case.dtype, case.pad[2], case.off)
    pc = None
    if case.beta:
        pc = pd if getattr(case, "inplace", False) else xc.Placed(e(m[2]), case.dtype, case.pad[2], case.off)
    ins = [pa, pb] + ([pc] if pc is not None else [])
    draws = []
    for swap in (False, True):
        A, B, C = xd.make_exact(case, swap)
        xd.check_draw(case, A, B, C, swap)
        want, _ = xd.expected(case, xd.exact_reference(case, A, B, C, device="cuda"))
        draws.append((stage(ins, [A, B, C]), [want]))
    ws = _workspace(plan)
    req = plan.required_workspace

    def launch(stream):
        plan.contract(case.alpha, pa.ptr, pb.ptr, case.beta, pc.ptr if pc is not None else 0, pd.ptr, ws.data_ptr(), req, stream)

    return Prepared("%s %s" % (case.id, d), plan if own else None, ins, [pd], ws, launch, draws)


def prepare_trinary_contraction(ct, ops, h, case, plan=None):
    """the data of exact_cases.run_trinary_case: E[abe] = alpha A[acd] B[cb] C[de] + beta D, every product and partial sum below 2^24"""
    import torch
    own = plan is None
    if own:
        plan = wc.make_plan(ct, ops, h, case)
    d = wc.check_path(ct, case, plan)
    mA, mB, mC, mD = case.modes
    dev = [xc.Placed(case.extents(m), case.dtype) for m in (mA, mB, mC)]
    pe, pd = xc.Placed(case.extents(mD), case.dtype), xc.Placed(case.extents(mD), case.dtype)
    ins = dev + [pe]
    draws = []
    for swap in (False, True):
        rng = np.random.default_rng([77, int(swap)])
        vals = np.array([-3, -2, -1, 1, 2, 3])
        X = [vals[rng.integers(0, 6, size=case.extents(m))] for m in (mA, mB, mC)]
        E = rng.integers(-3, 4, size=case.extents(mD))
        eq = "%s,%s,%s->%s" % (mA, mB, mC, mD)
        bound = np.einsum(eq, *[np.abs(x) for x in X], optimize=True).max()
        assert abs(case.alpha) * bound + 3 * abs(case.beta) < 2.0 ** 24, bound
        ref = case.alpha * np.einsum(eq, *X, optimize=True) + case.beta * E
        want, _ = xd.expected(case, torch.from_numpy(ref.astype(np.float64)))
        draws.append((stage(ins, [torch.from_numpy(x).to(pe.tdt) for x in X + [E]]), [want]))
    ws = _workspace(plan)
    req = plan.required_workspace

    def launch(stream):
        plan.contract_trinary(case.alpha, dev[0].ptr, dev[1].ptr, dev[2].ptr, case.beta, pe.ptr, pd.ptr, ws.data_ptr(), req, stream)

    return Prepared("%s %s" % (case.id, d), plan if own else None, ins, [pd], ws, launch, draws)


def prepare_blocksparse(ct, ops, h, case, plan=None):
    """exact_cases.blocksparse_inputs; every block of A, B, C and D in a Placed buffer of its own"""
    own = plan is None
    if own:
        plan = wc.make_plan(ct, ops, h, case)
    d = wc.check_path(ct, case, plan)
    lay = [wc.BlockLayout(case.ext, m, c) for m, c in zip(case.modes, case.blocks)]
    blocks = [[xc.Placed(shape, case.dtype) for shape in lay[i].shapes] for i in (0, 1, 2, 2)]          # A, B, C, D
    ins = blocks[0] + blocks[1] + blocks[2]
    draws = []
    for swap in (False, True):
        dense, _, A, B, C, _ = xc.blocksparse_inputs(case, swap)
        want, _ = xd.expected(dense, xd.exact_reference(dense, A, B, C))
        hosts = [x[sl] for i, x in enumerate((A, B, C)) for sl in lay[i].slices]
        draws.append((stage(ins, hosts), [want[sl] for sl in lay[2].slices]))
    ws = _workspace(plan)
    req = plan.required_workspace
    arr = [(ctypes.c_void_p * len(b))(*[p.ptr for p in b]) for b in blocks]
    al, be = plan.scalar(case.alpha), plan.scalar(case.beta)

    def launch(stream):
        ct.check(ct.cutensorBlockSparseContract(h.h, plan.plan, ctypes.byref(al), arr[0], arr[1], ctypes.byref(be), arr[2], arr[3],
                                                ws.data_ptr(), req, stream or None))

    return Prepared("%s %s" % (case.id, d), plan if own else None, ins, blocks[3], ws, launch, draws, keep=(arr, al, be))


def prepare(ct, ops, h, cid, plan=None):
    case = case_of(cid)
    return {"contraction": prepare_contraction, "contraction_trinary": prepare_trinary_contraction,
            "blocksparse": prepare_blocksparse}[case.kind](ct, ops, h, case, plan)


# ---- reductions and element-wise ---------------------------------------------------------------------------------------------------------
# (case id, the indices of the case's runs to take; None: every run) — cutensorReduce and its finalize; launch_fill and the permutation;
# the two passes of the trinary form and, where C is D, the single gather launch; a converting permutation; the binary form
EW = [("f32_red_row_split_add", None), ("f32_red_acc64_gen_split_add", None), ("c128_red_col_odd_split_add", None),
      ("f32_tri_two_pass_add_add", None), ("bf16_f32_perm_transpose_pad", None), ("f32_bin_transpose_t64_add", None)]
EW_CAPTURED = [("f32_red_row_split_add", 1), ("f32_tri_two_pass_add_add", 1)]


def ew_case(cid):
    return cc.BY_ID[cid] if cid in cc.BY_ID else ec.BY_ID[cid]


def prepare_ew(ct, ops, h, case, run):
    """one run (scalars, where C lives) of a case of tests/ew_exact_cases.py or tests/convert_cases.py, as their run_case lays it out"""
    convert = isinstance(case, cc.Case)
    plan = cc.make_plan(ct, ops, h, case) if convert else ec.make_plan(ct, ops, h, case)
    desc = wc.describe(ct, plan)
    assert case.expect(desc), "%s is off its path: %s" % (case.id, desc)
    d = {k: v for k, v in desc.pairs}
    placed = (lambda t: cc.placed(case, t)) if convert else (lambda t: ec._placed(case, t))
    host = (lambda t, x: cc.host(x, case.tdtype(t))) if convert else (lambda t, x: ec._host(case, x))
    scal, cmode = run
    names = [t for t in ec.TENSORS[case.kind][:-1] if t != "C"]
    dev = {t: placed(t) for t in names}
    pd = placed("D")
    pc = pd if cmode == "inplace" else placed("C" if "C" in case.modes else "D") if cmode == "separate" else None
    ins = [dev[t] for t in names] + ([pc] if pc is not None else [])
    draws = []
    for draw in range(2):
        x = ec.make_draw(case, draw, d)
        ec.check_draw(case, x, run, d)
        want = ec.expected(case, ec.reference(case, x, run))
        draws.append((stage(ins, [host(t, x[t]) for t in names] + ([host("D", x["C"])] if pc is not None else [])), [want]))
    ws = _workspace(plan) if case.kind == "reduction" else None
    req = plan.required_workspace
    cptr = pc.ptr if pc is not None else pd.ptr

    def launch(stream):
        if case.kind == "permutation":
            plan.permute(scal[0], dev["A"].ptr, pd.ptr, stream)
        elif case.kind == "binary":
            plan.binary(scal[0], dev["A"].ptr, scal[1], cptr, pd.ptr, stream)
        elif case.kind == "trinary":
            plan.trinary(scal[0], dev["A"].ptr, scal[1], dev["B"].ptr, scal[2], cptr, pd.ptr, stream)
        else:
            plan.reduce(scal[0], dev["A"].ptr, scal[1], cptr, pd.ptr, ws.data_ptr(), req, stream)

    return Prepared("%s scalars %s C %s %s" % (case.id, scal, cmode, desc), plan, ins, [pd], ws, launch, draws)


def prepare_padded(ct, ops, h, run=1):
    """convert_cases.PAD_CASE as convert_cases.run_padding lays it out: launch_fill writes the border, the permutation the interior"""
    case = cc.PAD_CASE
    plan = cc.make_plan(ct, ops, h, case, padding=(cc.PAD_LEFT, cc.PAD_RIGHT, cc.PAD_VALUE))
    desc = wc.describe(ct, plan)
    assert case.expect(desc), desc.raw
    pa = cc.placed(case, "A")
    full = [x + l + r for x, l, r in zip(case.extents("D"), cc.PAD_LEFT, cc.PAD_RIGHT)]
    pd = xc.Placed(full, case.dtype)
    scal, _ = case.runs[run]
    draws = []
    for draw in range(2):
        x = ec.make_draw(case, draw, {})
        want = np.full(full, cc.PAD_VALUE, dtype=np.float64)
        want[tuple(slice(l, l + n) for l, n in zip(cc.PAD_LEFT, case.extents("D")))] = ec.reference(case, x, (scal, "none"))
        draws.append((stage([pa], [cc.host(x["A"], case.dtypeA)]), [cc.host(want, "float64")]))

    def launch(stream):
        plan.permute(scal[0], pa.ptr, pd.ptr, stream)

    return Prepared("%s alpha %s %s" % (case.id, scal[0], desc.raw), plan, [pa], [pd], None, launch, draws)


def ew_runs(cid, which=None):
    case = ew_case(cid)
    return [(case, r) for i, r in enumerate(case.runs) if which is None or i == which]


# ---- running ---------------------------------------------------------------------------------------------------------------------------------
def run_contraction_gated(ct, ops, h, cid):
    case = case_of(cid)
    with wc.hook_env(case):
        p = prepare(ct, ops, h, cid)
        try:
            for k in (0, 1):
                gated([(p, k, side_stream(0))])
        finally:
            p.close()


def parse_times(out):
    """the ENQUEUE lines of a child's output into TIMES"""
    for line in out.splitlines():
        if line.startswith("ENQUEUE "):
            f = line.split()
            TIMES[f[1]] = max(TIMES.get(f[1], 0.0), float(f[2]) * 1e-6)
            DELAYS.append(float(line.rsplit("delay ", 1)[1].split()[0]))


if __name__ == "__main__":
    from cudalibrarysamples_amd import cutensor as ct_, ops as ops_
    mode_ = sys.argv[1]
    h_ = ops_.Handle()
    for cid_ in sys.argv[2:]:
        if mode_ == "describe":          # what the planner gives the case on this device (no launch)
            with wc.hook_env(case_of(cid_)):
                pl_ = _contraction_plan(ct_, ops_, h_, case_of(cid_))
            print("DESCRIBE", cid_, wc.describe(ct_, pl_), flush=True)
            pl_.destroy()
        else:
            run_contraction_gated(ct_, ops_, h_, cid_)
        print("ok", cid_, flush=True)
