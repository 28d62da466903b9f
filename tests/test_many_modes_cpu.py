"""The table of tests/many_mode_cases.py on the CPU planner (no GPU): every case plans onto the kernel it names and every draw of every
run satisfies the data conditions of tests/ew_exact_cases.py, so exactness in D's type is proved before a GPU sees a case.  Beside it:
what stays refused with many modes, the descriptions of every plan that existed before the mode-table route
(tests/golden/many_modes_unchanged_descriptions.json, tools/gen_ew_unchanged_descriptions.py), the description of a 25-mode plan, the
plan memo on a many-mode plan, and the host replay of every case's table (tests/harness/ew_table_layout_harness.cpp on
csrc/kernels/ew_table_layout.h)."""
import ctypes
import json
import os
import struct
import subprocess

import pytest

import ew_exact_cases as ec
import many_mode_cases as mm
import workspace_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KDIR = os.path.join(ROOT, "cudalibrarysamples_amd", "csrc", "kernels")
_DESC = {}


@pytest.fixture(scope="module")
def env(built):
    from cudalibrarysamples_amd import cutensor as ct, ops
    return ct, ops, ops.Handle()


def _describe(env, case):
    if case.id not in _DESC:
        ct, ops, h = env
        _DESC[case.id] = mm.plan_path(ct, ops, h, case)
    return _DESC[case.id]


@pytest.mark.parametrize("case", mm.CASES, ids=[c.id for c in mm.CASES])
def test_case_is_on_its_kernel_and_its_draws_hold(env, case):
    d = _describe(env, case)
    n = mm.check_case(case, d)
    assert 2 <= n <= ec.MAX_DRAWS


def test_the_table_covers_the_three_kernels_and_the_split(env):
    names = {_describe(env, c).get("kname") for c in mm.CASES}
    assert names == {"ew_table_tile_kernel", "ew_table_gather_kernel", "reduce_table_kernel"}
    assert any(_describe(env, c).get("splitR", 1) > 1 for c in mm.CASES)
    d = _describe(env, mm.BY_ID["f32_perm_long_in_a"])
    assert d["tile"][0] % 64 == 0 and 70 % 64 != 0          # the long mode is cut into pieces of 64: its last piece is partial


def _status(ct, f):
    try:
        f().destroy()
    except ct.CuTensorError as e:
        return e.status
    return ct.STATUS_SUCCESS


def test_what_stays_refused_with_many_modes(env):
    """each of these was refused before for its mode count alone; the mode-table kernels take one data type, no padding and no second
    permuted operand"""
    ct, ops, h = env
    e, m = [2] * 8, mm.M8
    rev = m[::-1]
    assert _status(ct, lambda: ops.permutation_plan(h, e, m, e, rev)) == ct.STATUS_SUCCESS
    assert _status(ct, lambda: ops.permutation_plan(h, e, m, e, rev, dtype=ct.R_32F, dtypeB=ct.R_16BF)) == ct.STATUS_NOT_SUPPORTED
    assert _status(ct, lambda: ops.binary_plan(h, e, m, e, rev, dtype=ct.R_16F, dtypeC=ct.R_32F)) == ct.STATUS_NOT_SUPPORTED
    assert _status(ct, lambda: ops.permutation_plan(h, e, m, e, rev, padding=([1] * 8, [0] * 8, 0.0))) == ct.STATUS_NOT_SUPPORTED
    assert _status(ct, lambda: ops.trinary_plan(h, e, m, e, rev, e, rev, e, rev)) == ct.STATUS_NOT_SUPPORTED
    assert _status(ct, lambda: ops.trinary_plan(h, e, m, e, m[1:] + m[0], e, rev, e, rev)) == ct.STATUS_NOT_SUPPORTED
    # 2^31 elements: refused as before ("tensor too large for the tile index space")
    m31 = mm.modes_of(26) + "ABCDE"
    assert _status(ct, lambda: ops.permutation_plan(h, [2] * 31, m31, [2] * 31, m31[::-1])) == ct.STATUS_NOT_SUPPORTED


def test_every_plan_that_existed_before_is_unchanged(env):
    """byte for byte the description the commit before the mode-table route gave (the golden was generated there)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_ew_unchanged_descriptions", os.path.join(ROOT, "tools", "gen_ew_unchanged_descriptions.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(gen.OUT) as f:
        want = json.load(f)
    got = gen.describe_all()
    assert sorted(got) == sorted(want)
    changed = {k: (want[k], got[k]) for k in want if got[k] != want[k]}
    assert not changed, changed
    assert not any("ew_table" in v or "reduce_table" in v for v in got.values())


def test_a_25_mode_plan_describes_its_modes(env):
    """the view's modes are D's modes after fusion: all 25 under a reversal, seven when three single modes move to the front"""
    ct, ops, h = env
    m = mm.modes_of(25)
    for mD, modes in ((m[::-1], 25), (mm.FRONT3_D, 7)):
        plan = ops.permutation_plan(h, [2] * 25, m, [2] * 25, mD)
        try:
            d = wc.describe(ct, plan)
            assert d.get("modes") == modes and mm.tiled(d), d
            assert d.get("tile")[0] * d.get("blocks") == 1 << 25
        finally:
            plan.destroy()


def test_a_many_mode_plan_is_memoised_and_the_switch_stands_aside(env):
    ct, ops, h = env
    case = mm.BY_ID["f32_perm_rev12"]
    h2 = ops.Handle()
    hits0, misses0, _ = ct.plan_memo_stats(h2.h)
    a = mm.make_plan(ct, ops, h2, case)
    b = mm.make_plan(ct, ops, h2, case)
    try:
        assert wc.describe(ct, a).raw == wc.describe(ct, b).raw
        hits1, misses1, _ = ct.plan_memo_stats(h2.h)
        assert (hits1, misses1) == (hits0 + 1, misses0 + 1), (hits0, misses0, hits1, misses1)
    finally:
        a.destroy()
        b.destroy()
    g = mm.make_plan(ct, ops, h2, mm.REV12_GATHER)          # same problem under the switch: planned again, on the other kernel
    try:
        assert mm.gather(wc.describe(ct, g))
    finally:
        g.destroy()
    assert ct.plan_memo_stats(h2.h)[:2] == (hits1, misses1)       # (neither looked up nor stored while the switch is set)
    c = mm.make_plan(ct, ops, h2, case)
    try:
        assert mm.tiled(wc.describe(ct, c))
    finally:
        c.destroy()


# ---- the host replay -------------------------------------------------------------------------------------------------------------------
def _truth(case):
    """the problem as the harness reads it: per mode of D (then per reduced mode of A) extent and strides in A, D, C"""
    m, rows = case.modes, []
    sA, sD = dict(zip(m["A"], case.strides("A"))), dict(zip(m["D"], case.strides("D")))
    uses_c = case.kind == "binary" or case.kind == "reduction"
    sC = dict(zip(m.get("C", m["D"]), case.strides("C" if "C" in m else "D"))) if uses_c else {}
    for c in m["D"]:
        rows.append((case.ext[c], sA.get(c, 0), sD[c], sC.get(c, 0)))
    for c in m["A"]:
        if c not in m["D"]:
            rows.append((case.ext[c], sA[c], -1, 0))
    return rows


def _dump(env, case, path):
    ct, ops, h = env
    plan = mm.make_plan(ct, ops, h, case)
    try:
        buf = ctypes.create_string_buffer(4096)
        ct.lib.ctamdEwTable.restype = ctypes.c_int
        ct.lib.ctamdEwTable.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
        n = ct.lib.ctamdEwTable(plan.plan, buf, 4096)
        assert n > 0, (case.id, n)
        rows = _truth(case)
        with open(path, "wb") as f:
            f.write(struct.pack("<q", len(rows)))
            for r in rows:
                f.write(struct.pack("<4q", *r))
            f.write(buf.raw[:n])
    finally:
        plan.destroy()


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ewt") / "ew_table_layout_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", KDIR,
                           os.path.join(ROOT, "tests", "harness", "ew_table_layout_harness.cpp"), "-o", exe])
    return exe


def test_every_table_produces_every_element_once_from_the_right_offsets(env, harness, tmp_path):
    files = []
    for case in mm.CASES:
        path = str(tmp_path / (case.id + ".ewt"))
        _dump(env, case, path)
        files.append(path)
    r = subprocess.run([harness] + files, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ew table layout ok: %d tables" % len(files) in r.stdout, r.stdout + r.stderr


def test_a_40_digit_table_with_strides_beyond_2_to_the_33(harness):
    r = subprocess.run([harness], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ew table layout ok: synthetic" in r.stdout, r.stdout + r.stderr
