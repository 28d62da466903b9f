"""Stream order of cutensorMgCopy under the gated-stream harness of tests/stream_cases.py: the source (one cell, owned by handle
entry 0) arrives behind a closed gate on a stream S; the call is made and the gate must still be closed when it returns; S alone
is synchronised, and the snapshot of the destination cells taken on S must be exact.  With the handle [0, 0] each entry launches on
a stream of its own, and S is given to entry 0 (the source owner) or to entry 1 (NOT the owner: the call runs behind everything
enqueued on every stream, whichever of them produced the source): the launch on the other stream has to wait for S (the fork — or
it reads 0xFF bytes at once), and S has to end behind it (the join — or the snapshot on S misses that entry's cells and the
poisoning of the source that follows on S races with its reads).  One rows case and one tile case; and the harness's control:
given the null stream, the call reads the poisoned source at once and the comparison fails."""
import numpy as np
import pytest

import stream_cases as sc
from tests import mg_copy_cases as mc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mg(built):
    import torch
    assert torch.cuda.is_available()
    from cudalibrarysamples_amd import cutensormg
    return cutensormg, torch


class CopyCall:
    """one cutensorMgCopy under the harness's protocol (the interface of stream_cases.Prepared)"""

    def __init__(self, cm, torch, devices, case, dtype="fp32", gated_entry=0):
        self.torch, self.case, self.dtype, self.gated_entry = torch, case, dtype, gated_entry
        self.what = self.name = "mg_copy_%s_%d_gate%d" % (case.id, len(devices), gated_entry)
        S, D, self.want = mc.make_data(case.src, case.dst, dtype, 21)
        as_dev = lambda cells: [torch.from_numpy(x.view(np.uint8).copy()).cuda() for x in cells]     # noqa: E731
        self.staging, self.dst_poison = as_dev(S), as_dev(D)
        self.live = [torch.full_like(t, 0xFF) for t in self.staging]
        self.dst = [t.clone() for t in self.dst_poison]
        self.plan = cm.CopyPlan(devices, case.dst.layout(), case.src.layout(), dtype=mc.DTYPES[dtype][0])
        d = self.plan.describe()
        assert d["srcOwners"] == [0] and sorted(set(d["dstOwners"])) == list(range(len(devices))) and not any(self.plan.ws_sizes), d
        self.snaps = None

    def alloc_snapshots(self):
        self.snaps = [self.torch.empty_like(t) for t in self.dst]

    def load(self, k):
        for l, s in zip(self.live, self.staging):
            l.copy_(s, non_blocking=True)

    def poison_inputs(self):
        for l in self.live:
            l.fill_(0xFF)

    def poison_all(self):
        self.poison_inputs()
        for t, p in zip(self.dst, self.dst_poison):
            t.copy_(p)

    def fill_workspace(self):
        pass

    def launch(self, stream):
        """the gated entry gets the harness's stream, the other entry (if any) the harness's second side stream"""
        streams = [sc.side_stream(1).cuda_stream] * len(self.plan.devices)
        streams[self.gated_entry] = stream
        st = self.plan.run([t.data_ptr() for t in self.dst], [t.data_ptr() for t in self.live], None, streams)
        assert st == 0, st

    def snapshot(self):
        for s, t in zip(self.snaps, self.dst):
            s.copy_(t, non_blocking=True)

    def check(self, k, what=""):
        np_dt = mc.DTYPES[self.dtype][1]
        mc.check([s.cpu().numpy().view(np_dt) for s in self.snaps], self.want, self.dtype, "%s %s" % (self.what, what))

    def has_nan(self):
        """a valid element of the snapshot is all ones: the poison of the live source (NaN in every type)"""
        np_dt = mc.DTYPES[self.dtype][1]
        ones = np.iinfo(np_dt).max
        return any(((s.cpu().numpy().view(np_dt) == ones) & (w != mc.poison(np_dt, mc.DST_POISON))).any() for s, w in zip(self.snaps, self.want))

    def close(self):
        self.plan.close()


@pytest.mark.parametrize("devices,gated_entry", [([0], 0), ([0, 0], 0), ([0, 0], 1)], ids=["one", "two_streams_owner", "two_streams_not_owner"])
@pytest.mark.parametrize("cid", ["scatter_rows", "scatter_tile"])
def test_copy_runs_in_stream_order(mg, cid, devices, gated_entry):
    cm, torch = mg
    call = CopyCall(cm, torch, devices, mc.BY_ID[cid], gated_entry=gated_entry)
    try:
        sc.gated([(call, 0, sc.side_stream(0))], "gated")
    finally:
        torch.cuda.synchronize()
        call.close()


def test_the_harness_can_fail_for_this_call(mg):
    """stream_cases.control: the call is given the null stream while the source arrives late on S — it must read 0xFF"""
    cm, torch = mg
    call = CopyCall(cm, torch, [0], mc.BY_ID["scatter_rows"])
    try:
        sc.control(call)
    finally:
        torch.cuda.synchronize()
        call.close()
