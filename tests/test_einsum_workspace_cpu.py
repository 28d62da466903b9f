"""torch_einsum._get_workspace keeps one growing buffer per (device, stream): two streams that run split-K einsums side by side must not
share their partials, and a buffer that grows on one stream must leave every other stream's buffer alone.  Host-only: _alloc_workspace
is replaced by a fake that hands out numbered buffers, streams are plain integers (a raw stream handle)."""
import pytest


class FakeBuffer:
    def __init__(self, serial, nbytes, device):
        self.serial, self.nbytes, self.device = serial, nbytes, device

    def numel(self):
        return self.nbytes


@pytest.fixture
def tein(built, monkeypatch):
    from cudalibrarysamples_amd import torch_einsum as te
    made = []

    def alloc(nbytes, device):
        made.append(FakeBuffer(len(made), nbytes, device))
        return made[-1]

    monkeypatch.setattr(te, "_alloc_workspace", alloc)
    monkeypatch.setattr(te, "_workspace", {})
    return te, made


S1, S2 = 0x1000, 0x2000


def test_no_workspace_for_a_plan_that_needs_none(tein):
    te, made = tein
    assert te._get_workspace("cuda:0", 0, S1) is None and not made


def test_each_stream_gets_a_buffer_of_its_own(tein):
    te, made = tein
    a = te._get_workspace("cuda:0", 1024, S1)
    b = te._get_workspace("cuda:0", 1024, S2)
    assert a is not b and [x.serial for x in (a, b)] == [0, 1]
    assert a.nbytes == b.nbytes == 1024
    # another device with the same stream handle: its own buffer too
    c = te._get_workspace("cuda:1", 1024, S1)
    assert c is not a and c.device == "cuda:1" and len(made) == 3


def test_a_stream_reuses_its_buffer_when_the_request_fits(tein):
    te, made = tein
    a = te._get_workspace("cuda:0", 1024, S1)
    assert te._get_workspace("cuda:0", 1024, S1) is a
    assert te._get_workspace("cuda:0", 100, S1) is a
    assert len(made) == 1


def test_growth_replaces_one_stream_s_buffer_and_no_other(tein):
    te, made = tein
    a = te._get_workspace("cuda:0", 1024, S1)
    b = te._get_workspace("cuda:0", 2048, S2)
    big = te._get_workspace("cuda:0", 4096, S1)
    assert big is not a and big.nbytes == 4096 and len(made) == 3
    assert te._get_workspace("cuda:0", 2048, S2) is b              # untouched by S1's growth
    assert te._get_workspace("cuda:0", 1024, S1) is big            # the grown buffer serves the smaller request from now on
    assert te._workspace == {("cuda:0", S1): big, ("cuda:0", S2): b}
    assert len(made) == 3


def test_a_failed_allocation_keeps_nothing(tein, monkeypatch):
    """einsum() plans again with the minimum workspace when the allocation fails: the stream must not be left with a stale entry"""
    te, made = tein
    te._get_workspace("cuda:0", 1024, S1)
    b = te._get_workspace("cuda:0", 1024, S2)

    def failing(nbytes, device):
        raise MemoryError("simulated")

    monkeypatch.setattr(te, "_alloc_workspace", failing)
    with pytest.raises(MemoryError):
        te._get_workspace("cuda:0", 4096, S1)
    assert te._workspace == {("cuda:0", S2): b}
