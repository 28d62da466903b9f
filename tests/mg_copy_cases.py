"""The case table of the cutensorMgCopy tests (tests/test_mg_copy_plan_cpu.py plans every case and tests/test_mg_copy_replay_cpu.py
replays it without a GPU, tests/test_gpu_mg_copy_exact.py runs it) — a helper module, not a conftest, in the style of
tests/rc64_cases.py.

A case: id, the modes of the source and of the destination, extents per label, (block sizes; grid) of both sides in each side's own
mode order, optional strides of the source, the element types it runs with, and a predicate on the plan's description
(ctamdMgDescribeCopyPlan) that proves which form ran.

The reference is NumPy alone: the address function `_addresses` of tests/test_mg_replay_cpu.py (imported; `addresses` below adds
non-packed strides and is checked against it on every packed layout), `collect` of the same module, and np.transpose for the
permutation.  Data are random BIT PATTERNS (unsigned integers of the element size: NaN payloads, infinities, -0 and denormals
included) with the two poison patterns excluded; every cell buffer starts full of poison — 0xA5 bytes in source cells, 0x5A bytes
in destination cells — and after the call the WHOLE destination buffers must equal the expectation: valid elements bit for bit,
every other byte still 0x5A, so no padding or gap was written and no source padding (0xA5) reached a valid element."""
import numpy as np

from tests.test_mg_replay_cpu import _addresses, _layout, collect

DTYPES = {"fp32": (0, np.uint32), "fp64": (1, np.uint64), "fp16": (2, np.uint16), "bf16": (14, np.uint16)}     # cudaDataType, bit view
SRC_POISON, DST_POISON = 0xA5, 0x5A


def poison(np_dt, byte):
    return np.frombuffer(bytes([byte]) * np.dtype(np_dt).itemsize, dtype=np_dt)[0]


class Side:
    """one tensor: modes (a string), extents, block sizes and grid in the tensor's own mode order, optional strides"""

    def __init__(self, modes, ext, block, grid, elem_stride=None, block_stride=None):
        self.modes, self.ext, self.block, self.grid = modes, list(ext), list(block), list(grid)
        self.elem_stride, self.block_stride = elem_stride, block_stride
        es, bstr, cstr, self.cells, span = _layout(self.ext, self.block, self.grid)
        self.es = list(elem_stride) if elem_stride else es
        self.bstr = list(block_stride) if block_stride else bstr
        lb = [-(-(-(-e // b)) // d) for e, b, d in zip(self.ext, self.block, self.grid)]
        self.span = 1 + sum((b - 1) * s + (l - 1) * t for b, s, l, t in zip(self.block, self.es, lb, self.bstr))
        self.cstr = cstr
        self.packed = elem_stride is None and block_stride is None
        assert not self.packed or self.span == span

    def layout(self, owners=None):
        """the dict cutensormg.CopyPlan takes"""
        return dict(modes=self.modes, extent=self.ext, block=self.block, grid=self.grid, elem_stride=self.elem_stride,
                    block_stride=self.block_stride, owners=owners)

    def addresses(self):
        """(cell, offset) of every element — _addresses of tests/test_mg_replay_cpu.py with this side's strides"""
        idx = np.indices(self.ext, dtype=np.int64)
        cell = np.zeros(self.ext, dtype=np.int64)
        off = np.zeros(self.ext, dtype=np.int64)
        for i in range(len(self.ext)):
            blk, w = idx[i] // self.block[i], idx[i] % self.block[i]
            cell += (blk % self.grid[i]) * self.cstr[i]
            off += w * self.es[i] + (blk // self.grid[i]) * self.bstr[i]
        if self.packed:
            c0, o0, cells, span = _addresses(self.ext, self.block, self.grid)
            assert (c0 == cell).all() and (o0 == off).all() and cells == self.cells and span == self.span
        return cell, off

    def valid_elements(self):
        n = 1
        for e in self.ext:
            n *= e
        return n


class Case:
    def __init__(self, id, msrc, mdst, ext, src, dst, expect, dtypes=("fp32",), src_strides=(None, None)):
        self.id, self.ext, self.expect, self.dtypes = id, ext, expect, dtypes
        self.src = Side(msrc, [ext[c] for c in msrc], src[0], src[1], *src_strides)
        self.dst = Side(mdst, [ext[c] for c in mdst], dst[0], dst[1])

    def __repr__(self):
        return self.id


def aligned_cells(cells, span, np_dt, fill):
    """`cells` buffers of `span` elements, each starting at a multiple of 64 bytes (16-byte lanes need aligned cells; the host
    replay refuses to fall back quietly), full of the poison byte `fill`"""
    item = np.dtype(np_dt).itemsize
    pitch = -(-span * item // 64) * 64
    raw = np.full(cells * pitch + 64, fill, dtype=np.uint8)
    start = (-raw.ctypes.data) % 64
    return [raw[start + c * pitch: start + c * pitch + span * item].view(np_dt) for c in range(cells)]


def make_data(src, dst, dtype, seed):
    """-> (source cells, destination cells full of poison, expected destination cells) as lists of 64-byte aligned arrays"""
    np_dt = DTYPES[dtype][1]
    rng = np.random.default_rng(seed)
    G = rng.integers(0, np.iinfo(np_dt).max, size=src.ext, dtype=np_dt, endpoint=True)
    for p in (poison(np_dt, SRC_POISON), poison(np_dt, DST_POISON)):
        G[G == p] ^= np_dt(1)                                   # the data never look like poison
    want_global = np.transpose(G, [src.modes.index(m) for m in dst.modes])
    assert list(want_global.shape) == dst.ext
    S = aligned_cells(src.cells, src.span, np_dt, SRC_POISON)
    D = aligned_cells(dst.cells, dst.span, np_dt, DST_POISON)
    W = aligned_cells(dst.cells, dst.span, np_dt, DST_POISON)
    cell, off = src.addresses()
    for c in range(src.cells):
        S[c][off[cell == c]] = G[cell == c]
    cell, off = dst.addresses()
    for c in range(dst.cells):
        W[c][off[cell == c]] = want_global[cell == c]
    if dst.packed:
        assert (collect(W, dst.ext, dst.block, dst.grid) == want_global).all()
    return S, D, W


def check(got, want, dtype, what):
    """the whole destination buffers: valid elements bit for bit, everything else still destination poison; no source poison anywhere"""
    np_dt = DTYPES[dtype][1]
    sp = poison(np_dt, SRC_POISON)
    for c, (g, w) in enumerate(zip(got, want)):
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, "%s: cell %d differs at %d offsets, first %d: got %#x want %#x (%s)" % (
            what, c, bad.size, bad[0], int(g[bad[0]]), int(w[bad[0]]),
            "a byte outside the valid elements was written" if w[bad[0]] == poison(np_dt, DST_POISON) else "a valid element")
        assert not (g == sp).any(), "%s: source padding reached cell %d" % (what, c)


# ---- predicates on the plan description ------------------------------------------------------------------------------------------
def launches(d):
    return [L for dev in d["devices"] for L in dev["launches"]]


def form(name, lane=None):
    def ok(d, dtype):
        ls = launches(d)
        want_lane = lane(dtype) if callable(lane) else lane
        return bool(ls) and all(L["form"] == name and (want_lane is None or L["lane"] == want_lane) for L in ls)
    return ok


def workspace_tables(d, dtype):
    return all((dev["workspace"] > 0) == bool(dev["launches"]) for dev in d["devices"]) and form("rows")(d, dtype)


ELEM = lambda dtype: np.dtype(DTYPES[dtype][1]).itemsize      # noqa: E731   element lanes: the lane is one element

E2 = dict(a=96, b=80)
CASES = [
    # runs cut by both sides' block edges, ragged a; 16-byte lanes in every type (block sizes 16 and 24, every other stride a multiple)
    Case("rows_misaligned", "abc", "abc", dict(a=70, b=9, c=5), ((16, 4, 5), (2, 2, 1)), ((24, 3, 2), (1, 2, 2)), form("rows", 16),
         dtypes=("fp32", "bf16", "fp16", "fp64")),
    Case("rows_odd", "abc", "abc", dict(a=70, b=9, c=5), ((7, 4, 5), (2, 2, 1)), ((24, 3, 2), (1, 2, 2)), form("rows", ELEM)),
    # more than one tile each way, partial tiles, tiles straddling cells
    Case("tile_2d", "ab", "ba", dict(a=130, b=67), ((16, 8), (2, 2)), ((9, 32), (2, 1)), form("tile"), dtypes=("fp32", "fp16", "fp64")),
    Case("tile_3d", "abc", "cab", dict(a=37, b=22, c=9), ((8, 5, 4), (2, 2, 1)), ((4, 16, 6), (1, 3, 2)), form("tile")),     # a middle mode on the move
    Case("scatter_rows", "ab", "ab", E2, ((96, 80), (1, 1)), ((32, 16), (2, 2)), form("rows", 16)),
    Case("gather_rows", "ab", "ab", E2, ((32, 16), (2, 2)), ((96, 80), (1, 1)), form("rows", 16)),
    Case("scatter_tile", "ab", "ba", E2, ((96, 80), (1, 1)), ((32, 16), (2, 2)), form("tile")),
    Case("gather_tile", "ba", "ab", E2, ((32, 16), (2, 2)), ((96, 80), (1, 1)), form("tile")),
    Case("same_layout", "ab", "ab", dict(a=64, b=64), ((32, 32), (2, 2)), ((32, 32), (2, 2)), form("flat")),
    # element stride 2 on a, gaps between the columns and between the blocks: one element per lane, the destination is packed
    Case("strided", "ab", "ab", dict(a=40, b=12), ((8, 4), (2, 1)), ((10, 6), (1, 2)), form("gather"), src_strides=((2, 20), (85, 262))),
    # the mode loop, blocks of extent 1, a block larger than its extent
    Case("many_modes", "abcdef", "fbdace", dict(a=3, b=4, c=2, d=5, e=3, f=2), ((2,) * 6, (2, 1, 2, 1, 1, 1)),
         ((3, 2, 1, 2, 2, 1), (1, 2, 1, 1, 2, 1)), form("tile")),
    # 144 cells on either side, more than the kernel arguments hold: the cell tables go through the device workspace
    Case("many_cells", "abc", "abc", dict(a=16, b=12, c=6), ((1, 1, 1), (8, 6, 3)), ((2, 1, 1), (2, 12, 6)), workspace_tables),
]
BY_ID = {c.id: c for c in CASES}
RUNS = [(c, t) for c in CASES for t in c.dtypes]
RUN_IDS = ["%s-%s" % (c.id, t) for c, t in RUNS]
ROUND_TRIPS = [("scatter_rows", "gather_rows"), ("scatter_tile", "gather_tile")]


def run_on_host(cm, devices, case, dtype, seed=0, src=None, dst=None):
    """plans the case on a handle over `devices`, replays it over host cells with ctamdMgCopyReplayOnHost, checks everything;
    returns the plan description"""
    src, dst = src or case.src, dst or case.dst
    S, D, W = make_data(src, dst, dtype, seed)
    with cm.CopyPlan(devices, dst.layout(), src.layout(), dtype=DTYPES[dtype][0]) as p:
        d = p.describe()
        rc = p.replay_on_host([x.ctypes.data for x in D], [x.ctypes.data for x in S])
    assert rc == 0, rc
    check(D, W, dtype, "%s %s on %s" % (case.id if case else "fuzz", dtype, devices))
    return d


# ---- the fuzz -----------------------------------------------------------------------------------------------------------------------
FUZZ_DRAWS = 50


def fuzz_draw(seed):
    """2-5 modes, extents up to 12, random block sizes (1 .. extent + 2: ragged, and blocks larger than the extent), grids of 1-3 cells per
    mode (more grid coordinates than blocks included), a random permutation, a random type.  No descriptor rule refuses any of these
    (default owners are handle devices, the mode count is below the cap, strides are packed): the refused share is 0 of 50, within
    the cap of 20 % (tests/test_mg_copy_replay_cpu.py counts it)."""
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(2, 6))
    labels = "abcde"[:n]
    ext = {c: int(rng.integers(1, 13)) for c in labels}
    sides = []
    for _ in range(2):
        modes = "".join(rng.permutation(list(labels)))
        block = [int(rng.integers(1, ext[c] + 3)) for c in modes]
        grid = [int(rng.integers(1, 4)) for _ in modes]
        sides.append(Side(modes, [ext[c] for c in modes], block, grid))
    return sides[0], sides[1], str(rng.choice(sorted(DTYPES)))
