"""The plan cache, its file and the plan memo of a handle (csrc/host/plan_store.cpp) on a handle that needs no device: what
tests/test_gpu_plan_cache.py checks with timed trials, as far as it can be checked by writing a cache file, editing it and reading it back.
The problem is that test's fp32 one, 'mk,kn->mn' at M = 512, N = 384, K = 4096 with m fastest in A and k fastest in B."""
import ctypes

import pytest

M, N, K = 512, 384, 4096
HEADER = "cutensor-amd-plancache 1"


@pytest.fixture(scope="module")
def env(built):
    from cudalibrarysamples_amd import cutensor as ct, ops
    return ct, ops


def _plan(ops, h, **kw):
    return ops.contraction_plan(h, [M, K], "mk", [K, N], "kn", [M, N], "mn", workspace_limit=256 << 20, **kw)


def _choice(ops, h, **kw):
    p = _plan(ops, h, **kw)
    try:
        d = p.describe()
        return (d["kernel"], d["splitK"]), d
    finally:
        p.destroy()


def _read(ct, h, path):
    n = ctypes.c_uint32(77)
    return ct.cutensorHandleReadPlanCacheFromFile(h.h, path.encode(), ctypes.byref(n)), n.value


@pytest.fixture(scope="module")
def flow(env, tmp_path_factory):
    """steps 1-4: the first two ranked candidates, a cache file written by a handle that holds the problem, and the same file with the
    entry rewritten to the second candidate"""
    ct, ops = env
    probe = ops.Handle()
    rank0, _ = _choice(ops, probe, algo=0, cache_mode=ct.CACHE_MODE_NONE)
    rank1, _ = _choice(ops, probe, algo=1, cache_mode=ct.CACHE_MODE_NONE)
    assert rank0 != rank1, (rank0, rank1)
    h = ops.Handle(plan_cache=16)
    assert _choice(ops, h)[0] == rank0 and ct.plan_memo_stats(h.h) == (0, 1, 1)
    # the measured choice: without a device its scratch allocation fails and it keeps the first candidate, with one it times them; either
    # way the cache holds the problem afterwards and the memoised default prototype is gone
    patient, _ = _choice(ops, h, algo=ct.ALGO_DEFAULT_PATIENT)
    assert ct.plan_memo_stats(h.h)[2] == 1                      # (the PATIENT plan itself, memoised after the store dropped the memo)
    assert _choice(ops, h)[0] == patient                        # the default plan is answered from the cache now
    written = str(tmp_path_factory.mktemp("plancache") / "written.txt")
    assert ct.cutensorHandleWritePlanCacheToFile(h.h, written.encode()) == ct.STATUS_SUCCESS
    text = open(written).read()
    lines = text.split("\n")
    assert lines[0] == HEADER and len(lines) == 3 and lines[2] == "", text
    cols = lines[1].split("\t")
    assert len(cols) == 5 and (int(cols[1]), int(cols[2])) == patient and int(cols[3]) == 0 and cols[4] == "0.000", cols
    edited = written.replace("written", "edited")
    with open(edited, "w") as f:
        f.write("\n".join([HEADER, "\t".join([cols[0], str(rank1[0]), str(rank1[1]), cols[3], cols[4]]), ""]))
    return dict(rank0=rank0, rank1=rank1, written=written, edited=edited, key=cols[0])


def test_a_cache_file_decides_the_default_plan_and_drops_the_memo(env, flow, tmp_path):
    ct, ops = env
    rank0, rank1 = flow["rank0"], flow["rank1"]
    streamed = _choice(ops, ops.Handle(plan_cache=16), operands_streamed=True)[0]   # on a handle that holds no entry
    h2 = ops.Handle(plan_cache=16)
    assert _choice(ops, h2)[0] == rank0
    assert ct.plan_memo_stats(h2.h) == (0, 1, 1)
    assert _read(ct, h2, flow["edited"]) == (ct.STATUS_SUCCESS, 1)
    assert ct.plan_memo_stats(h2.h) == (0, 1, 0)               # a memoised prototype must not shadow the file's choice
    c, d = _choice(ops, h2)
    assert c == rank1
    assert ct.plan_memo_stats(h2.h) == (0, 2, 1)
    c2, d2 = _choice(ops, h2)
    assert c2 == rank1 and d2 == d and ct.plan_memo_stats(h2.h) == (1, 2, 1)
    # a named candidate, a plan under the streamed-operands preference and CACHE_MODE_NONE do not ask the cache
    assert _choice(ops, h2, algo=0)[0] == rank0
    assert _choice(ops, h2, operands_streamed=True)[0] == streamed
    assert _choice(ops, h2, cache_mode=ct.CACHE_MODE_NONE)[0] == rank0
    # the handle writes what it read, byte for byte
    again = str(tmp_path / "again.txt")
    assert ct.cutensorHandleWritePlanCacheToFile(h2.h, again.encode()) == ct.STATUS_SUCCESS
    assert open(again, "rb").read() == open(flow["edited"], "rb").read()
    # step 7: a resize to 0 evicts the entry, and it stays evicted
    ct.check(ct.cutensorHandleResizePlanCache(h2.h, 0))
    ct.check(ct.cutensorHandleResizePlanCache(h2.h, 16))
    assert _choice(ops, h2)[0] == rank0


def test_a_cache_of_capacity_zero_reads_nothing(env, flow):
    ct, ops = env
    h3 = ops.Handle()
    ct.check(ct.cutensorHandleResizePlanCache(h3.h, 0))
    assert _read(ct, h3, flow["edited"]) == (ct.STATUS_INSUFFICIENT_WORKSPACE, 0)
    assert _choice(ops, h3)[0] == flow["rank0"] and ct.plan_memo_stats(h3.h) == (0, 0, 0)


def test_read_skips_malformed_lines_overwrites_and_stops_at_the_first_line_that_does_not_fit(env, flow, tmp_path):
    ct, ops = env
    rank0, rank1, key = flow["rank0"], flow["rank1"], flow["key"]
    line = lambda k, c: "\t".join([k, str(c[0]), str(c[1]), "0", "0.000"])   # noqa: E731
    path = str(tmp_path / "many.txt")
    with open(path, "w") as f:
        f.write("\n".join([HEADER, "no tab in this line", key + "\tnot a number", line(key, rank0), line("other|problem", (3, 1)),
                           line(key, rank1), line("third|problem", (4, 2)), ""]))
    h = ops.Handle()
    ct.check(ct.cutensorHandleResizePlanCache(h.h, 2))
    # four well-formed lines: the key, another key, the key again (overwriting always fits), a third key (does not)
    assert _read(ct, h, path) == (ct.STATUS_INSUFFICIENT_WORKSPACE, 3)
    assert _choice(ops, h)[0] == rank1
    out = str(tmp_path / "out.txt")
    assert ct.cutensorHandleWritePlanCacheToFile(h.h, out.encode()) == ct.STATUS_SUCCESS
    assert open(out).read().split("\n") == [HEADER] + sorted([line(key, rank1), line("other|problem", (3, 1))]) + [""]
    # a resize evicts from the smallest key upward
    ct.check(ct.cutensorHandleResizePlanCache(h.h, 1))
    assert ct.cutensorHandleWritePlanCacheToFile(h.h, out.encode()) == ct.STATUS_SUCCESS
    assert open(out).read().split("\n") == [HEADER, max(line(key, rank1), line("other|problem", (3, 1))), ""]
    # not a cache file, no file
    bad = str(tmp_path / "bad.txt")
    open(bad, "w").write("something else 1\n")
    assert _read(ct, h, bad) == (ct.STATUS_IO_ERROR, 0)
    assert _read(ct, h, str(tmp_path / "missing.txt")) == (ct.STATUS_IO_ERROR, 0)


def test_a_resumed_tuning_state_is_written_back(env, flow, tmp_path):
    """tried > 0 resumes incremental autotuning where the writing process stopped: the count and the best time come back out, and a
    plan under the autotune mode is no trial once all candidates were tried"""
    ct, ops = env
    rank1, key = flow["rank1"], flow["key"]
    path = str(tmp_path / "tuned.txt")
    text = "\n".join([HEADER, "\t".join([key, str(rank1[0]), str(rank1[1]), "4", "12.345"]), ""])
    open(path, "w").write(text)
    h = ops.Handle()
    assert _read(ct, h, path) == (ct.STATUS_SUCCESS, 1)
    tune = dict(cache_mode=ct.CACHE_MODE_PEDANTIC, autotune=ct.AUTOTUNE_MODE_INCREMENTAL, incremental_count=4)
    assert _choice(ops, h, **tune)[0] == rank1
    out = str(tmp_path / "out.txt")
    assert ct.cutensorHandleWritePlanCacheToFile(h.h, out.encode()) == ct.STATUS_SUCCESS
    assert open(out).read() == text
