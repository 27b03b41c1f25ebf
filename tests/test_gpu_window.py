"""The range pass on its own (k_block_reads + k_window, through the test entry point mm2gb_window_check): every st[i], every
per-block planner word and the input flags against a NumPy restatement of lchain.c:170-173 and of the planner's definitions
(chain_dev.h, DevBatch), on batches built to hit the kernel's edges -- read boundaries inside blocks, empty and one-anchor reads,
windows wider than the stretch a block stages in LDS, windows at max_iter and one either side of it, strand / reference changes
inside a window, runs of equal x, positions near 2^31, batch sizes that are not a multiple of the block."""
import ctypes as C

import numpy as np
import pytest

import orc
import synth_cases as sc

pytestmark = pytest.mark.gpu

mm = pytest.importorskip("mm2gb_amd")

PLAN_BLOCK = 1024
INT32_MAX = 2**31 - 1
FLAG_ANY_SEGID, FLAG_NO_LUT = 1, 2


def run_window(a, off, max_dist_x, max_iter):
    L = mm.lib()
    fn = L.mm2gb_window_check
    fn.argtypes = [C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 6
    a = np.ascontiguousarray(a, dtype=np.uint64)
    off = np.ascontiguousarray(off, dtype=np.int64)
    n, nb = len(a), (len(a) + PLAN_BLOCK - 1) // PLAN_BLOCK
    st = np.empty(n, np.int32)
    cut, pairs, clamped = np.empty(nb, np.int32), np.empty(nb, np.int64), np.empty(nb, np.int32)
    wmax, flags = np.empty(2 * nb, np.int32), np.zeros(1, np.uint32)
    rc = fn(n, len(off) - 1, a.ctypes.data, off.ctypes.data, max_dist_x, max_iter, st.ctypes.data, cut.ctypes.data,
            pairs.ctypes.data, clamped.ctypes.data, wmax.ctypes.data, flags.ctypes.data)
    assert rc == 0, L.mm2gb_last_error()
    return dict(st=st, firstcut=cut, pairs=pairs, clamped=clamped, wmax=wmax, flags=int(flags[0]))


def window_loop(a, off, max_dist_x, max_iter):
    """lchain.c:170-173 as written: the carried start, per read; clamp = the start was cut by max_iter."""
    x = [int(v) for v in a[:, 0]]
    st = np.arange(len(a), dtype=np.int64)
    clamp = np.zeros(len(a), bool)
    for r in range(len(off) - 1):
        s, e = int(off[r]), int(off[r + 1])
        j = s
        for i in range(s, e):
            while j < i and (x[i] >> 32 != x[j] >> 32 or x[i] > x[j] + max_dist_x):
                j += 1
            if i - j > max_iter:
                clamp[i] = max_iter > 0
                j = i - max_iter
            st[i] = j
    return st, clamp


def window_closed(a, off, max_dist_x, max_iter):
    """The same in closed form (reads sorted by x): the first anchor in reach by a lower bound, then the max_iter cut."""
    x = a[:, 0]
    st = np.arange(len(a), dtype=np.int64)
    clamp = np.zeros(len(a), bool)
    for r in range(len(off) - 1):
        s, e = int(off[r]), int(off[r + 1])
        if e <= s:
            continue
        xr = x[s:e]
        assert np.all(xr[1:] >= xr[:-1]), "anchors of a read are sorted by x"
        pos = (xr & np.uint64(0xffffffff)).astype(np.int64)
        thr = (xr & ~np.uint64(0xffffffff)) | np.maximum(pos - max_dist_x, 0).astype(np.uint64)
        first = np.searchsorted(xr, thr, side="left")
        idx = np.arange(e - s)
        lb = np.maximum(idx - max_iter, 0)
        st[s:e] = s + np.where(idx > lb, np.maximum(first, lb), idx)
        clamp[s:e] = (max_iter > 0) & (first < idx - max_iter)
    return st, clamp


def planner_words(a, st, clamp):
    n = len(a)
    i = np.arange(n, dtype=np.int64)
    starts = np.arange(0, n, PLAN_BLOCK)
    blk = i // PLAN_BLOCK
    w = i - st
    cut_at = np.where(st == i, i, INT32_MAX)
    firstcut = np.minimum.reduceat(cut_at, starts)
    before = i < firstcut[blk]
    y = a[:, 1]
    seg = (y >> np.uint64(48)) & np.uint64(0xff)
    span = (y >> np.uint64(32)) & np.uint64(0xff)
    big = ((y & np.uint64(0xffffffff)) >= np.uint64(1 << 22)) | (span == 0)
    return dict(st=st.astype(np.int32), firstcut=firstcut.astype(np.int32), pairs=np.add.reduceat(w, starts),
                clamped=np.maximum.reduceat(clamp.astype(np.int32), starts),
                wmax=np.stack([np.maximum.reduceat(np.where(before, w, 0), starts),
                               np.maximum.reduceat(np.where(before, 0, w), starts)], axis=1).reshape(-1).astype(np.int32),
                flags=(FLAG_ANY_SEGID if np.any(seg != 0) else 0) | (FLAG_NO_LUT if np.any(big) else 0))


def check(a, off, max_dist_x=5000, max_iter=5000, loop=False):
    st, clamp = window_closed(a, off, max_dist_x, max_iter)
    if loop:
        st_l, clamp_l = window_loop(a, off, max_dist_x, max_iter)
        assert np.array_equal(st, st_l) and np.array_equal(clamp, clamp_l)
    want = planner_words(a, st, clamp)
    got = run_window(a, off, max_dist_x, max_iter)
    for k in ("st", "firstcut", "pairs", "clamped", "wmax"):
        bad = np.flatnonzero(got[k] != want[k])
        assert bad.size == 0, f"{k}: {bad.size} differ, first at {bad[0]}: got {got[k][bad[0]]} want {want[k][bad[0]]}"
    assert got["flags"] == want["flags"]
    return want


def batch(reads):
    reads = [np.asarray(r, np.uint64).reshape(-1, 2) for r in reads]
    off = np.zeros(len(reads) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in reads])
    return np.concatenate(reads), off


def steps(n, step, rid=5, rev=0, r0=1_000, qspan=15):
    return sc.pack(np.full(n, rid), np.full(n, rev), r0 + step * np.arange(n), 100 + np.arange(n), qspan=qspan)


def test_read_boundaries_inside_blocks():
    rng = np.random.default_rng(11)
    reads = []
    for k in range(400):
        m = int(rng.choice([0, 0, 1, 1, 2, 3, 31, 64, 700, 1023, 1024, 1025, 2500]))
        reads.append(sc.noise(m, 100 + k, n_rid=2, span=60_000, qlen=5_000) if m else np.zeros((0, 2), np.uint64))
    reads = [np.zeros((0, 2), np.uint64)] + reads + [np.zeros((0, 2), np.uint64)] * 3
    a, off = batch(reads)
    assert len(a) % PLAN_BLOCK
    check(a, off, loop=True)
    check(a, off, max_dist_x=200, max_iter=50, loop=True)


def test_one_anchor_reads():
    a, off = batch([sc.noise(1, k) for k in range(3000)])
    check(a, off, loop=True)


@pytest.mark.parametrize("max_iter", [1, 63, 1000, 1023, 1024, 1025, 3000, 5000, 20_000])
def test_dense_windows_across_blocks(max_iter):
    """Every anchor in reach: windows = max_iter, wider than the staged look-back from 1 024 on; clamped everywhere."""
    a, off = batch([sc.sort_by_x(sc.repeat_block(9_000, 3, xwin=3_000)), sc.sort_by_x(sc.repeat_block(30_000, 4, xwin=4_000)),
                    sc.noise(777, 5, n_rid=1)])
    w = check(a, off, max_iter=max_iter)
    assert w["clamped"].any()


@pytest.mark.parametrize("dist", [1_000, 2_047, 5_000])
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_windows_at_max_iter(dist, delta):
    """x rises by one per anchor: the window reaches dist anchors back, max_iter cuts it one short, exactly, or one beyond."""
    a, off = batch([steps(13_000, 1), steps(4_000, 1, rid=6), steps(2_000, 2, rid=6, r0=5_000_000)])
    w = check(a, off, max_dist_x=dist, max_iter=dist + delta)
    assert bool(w["clamped"].any()) == (delta < 0)


def test_strand_and_reference_changes():
    rng = np.random.default_rng(21)
    reads = []
    for k in range(12):
        n = int(rng.integers(500, 6000))
        rid = rng.integers(0, 3, n)
        rev = rng.integers(0, 2, n)
        reads.append(sc.sort_by_x(sc.pack(rid, rev, rng.integers(0, 30_000, n), rng.integers(15, 9_000, n))))
    a, off = batch(reads)
    check(a, off, loop=True)
    check(a, off, max_dist_x=800, max_iter=700, loop=True)


def test_equal_x_and_positions_near_2_31():
    rng = np.random.default_rng(31)
    top = 2**31 - 1
    runs = sc.sort_by_x(sc.pack(np.full(6000, 2), np.zeros(6000), top - 6000 + rng.integers(0, 40, 6000) * 150, rng.integers(15, 20_000, 6000)))
    ties = sc.grid_ties(nx=50, ny=13, step=3)
    high = sc.sort_by_x(sc.pack(np.full(5000, 1), np.ones(5000), top - rng.integers(0, 9000, 5000), rng.integers(15, 20_000, 5000)))
    a, off = batch([runs, ties, high, runs[:1500]])
    check(a, off, loop=True)
    check(a, off, max_dist_x=2**31 - 2**22, max_iter=4000)


def test_flags():
    a, off = batch([steps(3000, 3, qspan=15), steps(100, 3, rid=9, qspan=0)])
    assert check(a, off)["flags"] == FLAG_NO_LUT
    a, off = batch([sc.two_segments(3000, 5)])
    check(a, off)


@pytest.mark.parametrize("seed", range(12))
def test_fuzz_cases(seed):
    rng = np.random.default_rng(9000 + seed)
    a, off, _ = sc.fuzz_case(rng)
    if len(a) == 0:
        return
    for dist, it in ((5000, 5000), (int(rng.integers(1, 8000)), int(rng.integers(1, 3000)))):
        check(a, off, max_dist_x=dist, max_iter=it, loop=len(a) < 40_000)


def test_multi_read_batch():
    a, off = sc.multi_read_batch(60, 17)
    check(a, off)
    check(a, off, max_dist_x=1500, max_iter=200)


def test_rescue_case():
    a = sc.rescue_case()
    check(a, np.array([0, len(a)], np.int64), loop=True)


def test_synthetic_ultra_long_reads():
    """The bench's generator (100-300 kb ONT-like reads) at a few million anchors, defaults and a narrow max_iter."""
    a, off = mm.synth_reads(2024, 0, 60, 100_000, 300_000)
    prm = orc.default_param()
    w = check(a, off, max_dist_x=prm.max_dist_x, max_iter=prm.max_iter)
    assert w["pairs"].sum() > 0
    check(a, off, max_dist_x=prm.max_dist_x, max_iter=700)
