"""cutensorMgCopy plans without a GPU: every case of tests/mg_copy_cases.py plans into its form on plan-only handles with 1, 2, 4
and 8 distinct device ids; the bytes a plan accounts for are the tensor's valid bytes; a device gets at most one launch per form;
every refusal of the descriptor and the plan has its status and its CUTENSOR_LOG_LEVEL line; the workspace query is honoured; the
mode cap is at least 12.  (The refusal of a device pair without peer access needs real devices that lack it: it is not covered.)"""
import ctypes
import json
import os
import subprocess
import sys

import pytest

from tests import mg_copy_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HANDLES = [1, 2, 4, 8]


@pytest.fixture(scope="module")
def cm(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("plan-only handles for device ids 0..7 need a host without that many GPUs")
    from cudalibrarysamples_amd import cutensormg
    return cutensormg


@pytest.mark.parametrize("n", HANDLES)
@pytest.mark.parametrize("case,dtype", mc.RUNS, ids=mc.RUN_IDS)
def test_every_case_plans_into_its_form(cm, case, dtype, n):
    devices = list(range(n))
    with cm.CopyPlan(devices, case.dst.layout(), case.src.layout(), dtype=mc.DTYPES[dtype][0]) as p:
        d = p.describe()
        assert list(p.ws_sizes) == [dev["workspace"] for dev in d["devices"]] and p.host_size.value == 0 == d["hostWorkspace"]
    assert case.expect(d, dtype), d
    item = mc.ELEM(dtype)
    assert d["elementSize"] == item and len(d["devices"]) == n
    assert sum(dev["localBytes"] + dev["remoteBytes"] for dev in d["devices"]) == case.dst.valid_elements() * item, d
    if n == 1:
        assert d["devices"][0]["remoteBytes"] == 0
    seen = []
    for g, dev in enumerate(d["devices"]):
        forms = [L["form"] for L in dev["launches"]]
        assert len(forms) == len(set(forms)) <= 1, dev                    # at most one launch per device and form (one form per plan)
        for L in dev["launches"]:
            assert L["grid"][1] == len(L["cells"]) and all(d["dstOwners"][c] == g for c in L["cells"]), (g, L)
            seen += L["cells"]
        assert g not in dev["readOwners"] and all(0 <= o < n for o in dev["readOwners"])
    assert sorted(seen) == list(range(case.dst.cells))                      # every destination cell is filled exactly once
    # cells are dealt to the handle's devices cyclically (the default owners), a source cell on another device is a remote read
    assert d["dstOwners"] == [c % n for c in range(case.dst.cells)] and d["srcOwners"] == [c % n for c in range(case.src.cells)]
    if case.id == "same_layout":                                            # cell c goes to cell c, on the same device
        assert sum(dev["remoteBytes"] for dev in d["devices"]) == 0
    if case.id == "scatter_rows" and n >= 4:                                # the one source cell is on device 0, three of the four cells elsewhere
        # a: blocks 0 and 2 (64 indices) on grid coordinate 0, block 1 (32) on 1; b: 48 indices on coordinate 0, 32 on 1
        assert [(dev["localBytes"], dev["remoteBytes"]) for dev in d["devices"][:4]] == [(64 * 48 * 4, 0), (0, 32 * 48 * 4), (0, 64 * 32 * 4), (0, 32 * 32 * 4)]
        assert [dev["readOwners"] for dev in d["devices"][:4]] == [[], [0], [0], [0]]


def test_logical_devices_deal_cells_round_robin(cm):
    """a handle that lists one device several times: the k-th cell on that device belongs to entry k mod m"""
    case = mc.BY_ID["scatter_rows"]
    with cm.CopyPlan([0, 0, 0], case.dst.layout(), case.src.layout()) as p:
        d = p.describe()
    assert d["dstOwners"] == [0, 1, 2, 0] and d["srcOwners"] == [0]
    assert [dev["readOwners"] for dev in d["devices"]] == [[], [0], [0]]
    assert sum(dev["remoteBytes"] for dev in d["devices"]) == 0             # one physical device: every read is local


def test_lanes_run_along_the_longest_stride_1_label(cm):
    """packed layouts whose leading blocks hold one element have several modes of element stride 1: the lanes take the one with the
    most local coordinates, and a label that has stride 1 on both sides beats a transposition between two different ones"""
    src = mc.Side("abc", [3, 40, 5], [1, 8, 5], [1, 2, 1])          # a and b have element stride 1
    dst = mc.Side("abc", [3, 40, 5], [1, 16, 1], [1, 1, 2])         # a and b too
    d = mc.run_on_host(cm, [0, 1], None, "fp32", src=src, dst=dst)
    assert mc.form("rows", 4)(d, "fp32") and all(L["along"] == [ord("b"), ord("b")] for L in mc.launches(d)), d
    src = mc.Side("abc", [3, 40, 5], [3, 8, 5], [1, 2, 1])          # a alone
    dst = mc.Side("cab", [5, 3, 40], [1, 1, 8], [1, 1, 2])          # c, a and b: b is the longest, but a is common to both sides
    d = mc.run_on_host(cm, [0, 1], None, "fp32", src=src, dst=dst)
    assert mc.form("rows", 4)(d, "fp32") and all(L["along"] == [ord("a"), ord("a")] for L in mc.launches(d)), d
    d = mc.run_on_host(cm, [0], mc.BY_ID["tile_3d"], "fp32")
    assert all(L["along"] == [ord("c"), ord("a")] for L in mc.launches(d)), d


REFUSALS = {   # name -> (status, a fragment of the log line)
    "label_sets_differ": (7, "label sets differ"),
    "mode_counts_differ": (7, "label sets differ"),
    "extent_differs": (7, "extent of label"),
    "repeated_label": (7, "is repeated"),
    "different_types": (15, "different data types"),
    "too_many_modes": (15, "more than the cap"),
    "foreign_destination_cell": (15, "not in the handle"),
    "small_workspace": (19, "bytes of workspace"),
}


def _refusals_child():
    """runs in a child with CUTENSOR_LOG_LEVEL=1 (the level is read once per process): one JSON line per refusal on stdout"""
    from cudalibrarysamples_amd import cutensormg as cm

    def status(devices, dst, src, **kw):
        try:
            cm.CopyPlan(devices, dst, src, **kw).close()
        except cm.ct.CuTensorError as e:
            return e.status
        return 0

    def t(modes, ext, **kw):
        return dict(modes=modes, extent=ext, **kw)
    out = {}
    sys.stderr.write("REFUSAL label_sets_differ\n")
    out["label_sets_differ"] = status([0], t("ab", [4, 6]), t("ac", [4, 6]))
    sys.stderr.write("REFUSAL mode_counts_differ\n")
    out["mode_counts_differ"] = status([0], t("ab", [4, 6]), t("abc", [4, 6, 2]))
    sys.stderr.write("REFUSAL extent_differs\n")
    out["extent_differs"] = status([0], t("ab", [4, 6]), t("ba", [4, 6]))
    sys.stderr.write("REFUSAL repeated_label\n")
    out["repeated_label"] = status([0], t("aa", [4, 4]), t("ab", [4, 4]))
    sys.stderr.write("REFUSAL different_types\n")
    out["different_types"] = status([0], t("ab", [4, 6]), t("ab", [4, 6]), dtype=0, src_dtype=1)
    sys.stderr.write("REFUSAL too_many_modes\n")
    many = "abcdefghijklmnopq"
    out["too_many_modes"] = status([0], t(many, [1] * 17), t(many, [1] * 17))
    out["sixteen_modes"] = status([0], t(many[:16], [2] * 16), t(many[15::-1], [2] * 16))
    sys.stderr.write("REFUSAL foreign_destination_cell\n")
    out["foreign_destination_cell"] = status([0, 1], t("ab", [4, 6], owners=[5]), t("ab", [4, 6]))
    out["foreign_source_cell"] = status([0, 1], t("ab", [4, 6]), t("ab", [4, 6], owners=[5]))          # source cells may live anywhere
    sys.stderr.write("REFUSAL small_workspace\n")
    case = mc.BY_ID["many_cells"]
    with cm.CopyPlan([0], case.dst.layout(), case.src.layout()) as p:
        small = (ctypes.c_int64 * 1)(p.ws_sizes[0] - 1)
        plan = ctypes.c_void_p()
        out["small_workspace"] = cm.cutensorMgCreateCopyPlan(p.h, ctypes.byref(plan), p.cd, small, 0)
    sys.stderr.write("REFUSAL end\n")
    print(json.dumps(out))


def test_every_refusal_has_its_status_and_its_log_line(cm):
    env = dict(os.environ, CUTENSOR_LOG_LEVEL="1")
    r = subprocess.run([sys.executable, "-c", "from tests.test_mg_copy_plan_cpu import _refusals_child as f; f()"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = json.loads(r.stdout.strip().split("\n")[-1])
    assert got.pop("sixteen_modes") == 0 and got.pop("foreign_source_cell") == 0, got
    assert got == {k: v[0] for k, v in REFUSALS.items()}, got
    # the log: between a refusal's marker and the next one, exactly one line of the library, naming the reason
    blocks, name = {}, None
    for line in r.stderr.split("\n"):
        if line.startswith("REFUSAL "):
            name = line.split()[1]
            blocks[name] = []
        elif name is not None and line.startswith("[cutensor-amd]"):
            blocks[name].append(line)
    for k, (_, fragment) in REFUSALS.items():
        assert len(blocks[k]) == 1 and fragment in blocks[k][0] and "cutensorMgCreateCopy" in blocks[k][0], (k, blocks[k])


def test_workspace_query_is_honoured(cm):
    case = mc.BY_ID["many_cells"]
    for n in HANDLES:
        with cm.CopyPlan(list(range(n)), case.dst.layout(), case.src.layout()) as p:
            d = p.describe()
            assert d["argCells"] == 128 and case.src.cells == case.dst.cells == 144
            per_dev = [len(L["cells"]) for dev in d["devices"] for L in dev["launches"]]
            up = lambda x: -(-x // 256) * 256   # noqa: E731
            # the three tables: source pointers, this device's destination pointers, their cell indices
            assert list(p.ws_sizes) == [up(8 * 144) + up(8 * k) + up(4 * k) for k in per_dev] and p.host_size.value == 0
            # ... written by the table writer, 256 eight-byte words per launch, ahead of the device's copy launch
            assert [dev["tableLaunches"] for dev in d["devices"]] == [-(-s // 2048) for s in p.ws_sizes]
            assert n > 1 or d["devices"][0]["tableLaunches"] == 2
            plan = ctypes.c_void_p()
            for g in range(n):
                sizes = (ctypes.c_int64 * n)(*p.ws_sizes)
                sizes[g] -= 1
                assert cm.cutensorMgCreateCopyPlan(p.h, ctypes.byref(plan), p.cd, sizes, 0) == 19     # INSUFFICIENT_WORKSPACE
            assert cm.cutensorMgCreateCopyPlan(p.h, ctypes.byref(plan), p.cd, None, 0) == 19
            bigger = (ctypes.c_int64 * n)(*[s + 4096 for s in p.ws_sizes])
            assert cm.cutensorMgCreateCopyPlan(p.h, ctypes.byref(plan), p.cd, bigger, 0) == 0
            assert cm.describe_copy_plan(plan) == d                                                      # a larger offer changes nothing
            assert cm.cutensorMgDestroyCopyPlan(plan) == 0
    # all sizes 0: the plan (like the call) accepts a null size array
    case = mc.BY_ID["tile_2d"]
    with cm.CopyPlan([0, 1], case.dst.layout(), case.src.layout()) as p:
        assert list(p.ws_sizes) == [0, 0] and p.host_size.value == 0
        plan = ctypes.c_void_p()
        assert cm.cutensorMgCreateCopyPlan(p.h, ctypes.byref(plan), p.cd, None, 0) == 0
        assert cm.cutensorMgDestroyCopyPlan(plan) == 0
        # a plan-only handle cannot execute
        assert p.run([1] * case.dst.cells, [1] * case.src.cells, None, [0, 0]) != 0


def test_mode_cap_holds_blog_post_tensors(cm):
    """at least 12 modes (blog_post.cu's tensors): a 12-mode transposition plans, and the description names the cap"""
    modes = "abcdefghijkl"
    src = mc.Side(modes, [2] * 12, [2] + [1] * 11, [1, 2, 2] + [1] * 9)          # element stride 1 on a alone
    dst = mc.Side(modes[::-1], [2] * 12, [2] * 12, [1] * 12)
    d = mc.run_on_host(cm, [0, 1, 2, 3], None, "fp32", src=src, dst=dst)
    assert d["modeCap"] >= 12 and mc.form("tile")(d, "fp32")
