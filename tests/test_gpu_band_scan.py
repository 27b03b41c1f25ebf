"""The scan of the band pass (chain_kernels.hip, band_group): a group's sources [lo, jl) go by in whole blocks of 64 and one last block of
(jl - lo) % 64, whose other lanes read nothing and cannot hit; the hits of a block -- its mask straight from the compare -- are pushed to
the lanes of a stage after those already there, and a stage's block is staged from one 16-byte load per source, its x extent taken
from lanes 0 and 63 when x does not fall along the stage.

One read per case, built as in test_gpu_band_stage.py: an old run on the targets' diagonal, filler 20 000 off it (bw is 500 and the
targets lie within 40 of the run's diagonal: no group's band test lets a filler in), two slabs of targets, the first starting on a slab
boundary of the read.  New here: the read may begin with anchors more than max_dist_x to the left of everything else, so that every
window starts right after them at lo; the scan of the first slab of targets then covers exactly the anchors the case lays out, block
boundaries where the case puts them, and the slab's lag of filler follows.  The second slab scans a slab more.

Every anchor's f / p is checked against the oracle and against the dense sweep (MM2GB_BAND=0) of the same engine build, on the wave
path, in teams of 4 and in whole-workgroup teams, at slab / lag 128 / 64 and 256 / 128.

A stage never holds sources of two reads, nor of two (reference, strand) stretches of one read: the sources of a group are older than
jl, hence older than every target of the slab, and not older than the window start of the group's oldest target -- which lies in that
target's own stretch.  They are a run of ONE stretch, whose x does not fall.  So no batch of sorted reads takes the reductions that the
staging keeps for a stage whose x falls, and NO TEST HERE RUNS THEM (nor the loop over parts of a scan of more than 2^28 sources):
input that is not sorted is accepted but its values are unspecified, the dense sweep's as much as the band pass's, so there is
nothing to compare them with.  The nearest a sorted batch comes is a stage of anchors that share positions, ordered by query
position, which is a case below (its x does not fall either: the ends of the stage are its extent)."""
import numpy as np
import pytest

import mm2gb_amd  # noqa: F401  (first: a broken build fails here, before an import below could turn it into a skip)
import orc
import synth_cases as sc
from test_gpu_band import TEAMS, batch, engine_with
from test_gpu_parity import check_batch, misc_from

pytestmark = pytest.mark.gpu

SHAPES = [(128, 64), (256, 128)]
PATHS = ["wave", "teams-of-4", "whole-workgroup"]
X0, Y0 = 2_000_000, 60_000
FAR_LEFT = 1_000_000           # the leading anchors' distance from the rest: beyond max_dist_x, inside no window
FILLER_OFF = 20_000            # the filler's distance from the run's diagonal
R, F, E = "run", "filler", "equal-x run"

# what the scan of the first slab of targets sees, from lo on: (length, kind) stretches
LAYOUTS = {}
for L in (1, 63, 64, 65, 127, 128, 129):                          # scan lengths: the last block holds 1, 63, 0, 1, 63, 0, 1 sources
    LAYOUTS[f"scan-{L}"] = [(L // 3, F), (L - L // 3, R)]
# blocks without a hit: the first, three in a row and two in a row between blocks with hits, and the last (39 sources)
LAYOUTS["hit-free-blocks"] = [(64, F), (70, R), (250, F), (10, R), (200, F), (5, R), (80, F)]
for H in (255, 256, 257, 320):                                    # more hits than four stages hold, off the block boundaries
    LAYOUTS[f"hits-{H}"] = [(5, F), (H, R), (3, F)]
# single blocks that deliver 64, 0, 1 and 64 hits, then a last block of 3
LAYOUTS["hits-per-block"] = [(64, R), (64, F), (17, F), (1, R), (46, F), (64, R), (3, R)]
# anchors that share a position two by two, ordered by query position: x does not rise from lane to lane, and does not fall
LAYOUTS["equal-x"] = [(5, F), (150, E), (9, F)]


def read_with_layout(layout, slab, lag, seed=7):
    """(anchors, lo, jl, first target): leading anchors [0, lo), the layout [lo, jl), filler [jl, n0), targets [n0, n0 + 2 * slab)."""
    L = sum(n for n, _ in layout)
    lo = (-(L + lag)) % slab
    if lo + L + lag < 128:                                         # a slab takes the band pass from 128 anchors into its chunk on
        lo += slab
    jl, n0 = lo + L, lo + L + lag
    n = n0 + 2 * slab
    rng = np.random.default_rng(seed + 1000 * L + slab)
    x = X0 + np.arange(n, dtype=np.int64)
    x[:lo] -= FAR_LEFT
    y = x - (X0 - Y0)                                              # the run's diagonal
    y[:lo] = Y0 // 2 + np.arange(lo)
    y[jl:n0] -= FILLER_OFF
    at = lo
    for m, kind in layout:
        if kind == F:
            y[at:at + m] -= FILLER_OFF
        elif kind == E:
            x[at:at + m] = x[at] + np.arange(m) // 2
            y[at:at + m] = x[at:at + m] - (X0 - Y0) + np.arange(m) % 2 * 3
        at += m
    y[n0:] += rng.integers(-40, 41, n - n0)
    return sc.pack(np.full(n, 3), np.zeros(n, np.int64), x, y), lo, jl, n0


def read_with_a_tie(slab, lag):
    """Two old sources A < B with equal scores, 60 off the first target's diagonal on either side (120 from each other: chaining B to A
    does not pay), and 70 sources between them that every group's band test lets in: B is the 72nd hit of the scan, in the second
    stage, A the first hit.  The 70 lie above the first target on the query and descend: they score neither for it nor from each other."""
    lo = 0
    n0 = slab * 2
    jl = n0 - lag
    n = n0 + 2 * slab
    rng = np.random.default_rng(11 + slab)
    x = X0 + np.arange(n, dtype=np.int64)
    y = x - (X0 - Y0)
    y[:n0] -= FILLER_OFF
    y[n0 + 1:] += rng.integers(-40, 41, n - n0 - 1)                # (the first target stays on the diagonal)
    ib = jl - 20                                                   # (at least 15 + 60 before the first target: B's whole span counts)
    ia = ib - 71
    y[ia] = x[ia] - (X0 - Y0) - 60
    y[ib] = x[ib] - (X0 - Y0) + 60
    y[ia + 1:ib] = y[n0] + 100 - np.arange(70)
    return sc.pack(np.full(n, 3), np.zeros(n, np.int64), x, y), lo, jl, n0, ia, ib


@pytest.fixture(scope="module")
def reads():
    """Every case once, with the oracle's f / p: shared by the tests below and left unchanged."""
    prm = orc.default_param()
    out = {}
    for slab, lag in SHAPES:
        for name, layout in LAYOUTS.items():
            a, lo, jl, n0 = read_with_layout(layout, slab, lag)
            xs = a[:, 0].astype(np.int64) & 0xffffffff
            assert jl - lo == sum(m for m, _ in layout) and n0 % slab == 0 and n0 >= 128 and n0 - jl == lag
            assert np.all(np.diff(xs) >= 0) and xs[-1] - xs[lo] < prm.max_dist_x and len(a) < prm.max_iter
            assert lo == 0 or xs[lo] - xs[lo - 1] > prm.max_dist_x
            f, p, _ = orc.chain_fill_many(*batch([a]), prm, threads=1)
            out[(slab, lag, name)] = (a, lo, jl, n0, f, p)
        a, lo, jl, n0, ia, ib = read_with_a_tie(slab, lag)
        f, p, _ = orc.chain_fill_many(*batch([a]), prm, threads=1)
        out[(slab, lag, "tie")] = (a, lo, jl, n0, f, p, ia, ib)
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=["-".join(map(str, s)) for s in SHAPES])
def test_targets_chain_to_the_scanned_sources(reads, shape):
    """Without this a lost block or stage would go unnoticed: in every layout some target's best predecessor is one of the sources the
    first slab's scan covers.  (CPU: the oracle alone; marked gpu with the module, it needs none.)"""
    for name in LAYOUTS:
        a, lo, jl, n0, f, p = reads[shape + (name,)]
        assert np.any((p[n0:] >= lo) & (p[n0:] < jl)), f"{name}: no target chains to a scanned source"


@pytest.mark.parametrize("shape", SHAPES, ids=["-".join(map(str, s)) for s in SHAPES])
def test_the_tie_lies_across_a_stage_boundary(reads, shape):
    """(CPU.)  The first target scores the same from A and from B and takes B, the later one; B is in the stage after A's for every
    group the target can be in: each of the 72 sources from A to B passes every group's band test, and nothing else before jl does."""
    prm = orc.default_param()
    a, lo, jl, n0, f, p, ia, ib = reads[shape + ("tie",)]
    x, y = (a[:, 0].astype(np.int64) & 0xffffffff), (a[:, 1].astype(np.int64) & 0xffffffff)
    d = x - y
    from_a, from_b = f[ia] + orc.pair_score(a[n0], a[ia], prm), f[ib] + orc.pair_score(a[n0], a[ib], prm)
    assert from_a == from_b == f[n0] and p[n0] == ib
    d_lo, d_hi = d[n0:].min(), d[n0:].max()                       # a group's diagonals lie in here, whichever targets it holds
    assert d_hi - d_lo <= 80
    hits = np.arange(ia, ib + 1)
    assert np.all(d[hits] >= d_hi - prm.bw) and np.all(d[hits] <= d_lo + prm.bw)
    others = np.setdiff1d(np.arange(lo, jl), hits)
    assert np.all(np.abs(d[others] - d[n0]) > prm.bw + 80)
    assert ib - ia >= 64


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("shape", SHAPES, ids=["-".join(map(str, s)) for s in SHAPES])
def test_scans_against_the_oracle_and_the_dense_sweep(monkeypatch, reads, shape, path):
    slab, lag = shape
    prm = orc.default_param()
    side = 0 if path == "wave" else 1
    names = list(LAYOUTS) + ["tie"]
    res = {}
    for on in ("1", "0"):
        with engine_with(monkeypatch, dict(TEAMS[path], MM2GB_BAND=on, MM2GB_BAND_SLAB=str(slab), MM2GB_BAND_LAG=str(lag))) as e:
            for name in names:
                a, off = batch([reads[shape + (name,)][0]])
                if on == "1":
                    check_batch(e, a, off, prm, threads=1)          # every anchor's f / p against the oracle
                e.set_misc(misc_from(prm))
                f, p, st = e.score(a, off)
                groups = e.band_groups()
                if on == "0":
                    assert groups == (0, 0)
                else:
                    assert groups[side] > 0, f"{name}: the band pass did not run on the {path} path: {groups}"
                    if path == "wave":
                        assert groups[1] == 0
                res[(on, name)] = (f.copy(), p.copy(), st["n_pairs"])
    for name in names:
        band, dense = res[("1", name)], res[("0", name)]
        assert np.array_equal(band[0], dense[0]) and np.array_equal(band[1], dense[1]) and band[2] == dense[2], f"{name}: band and dense sweep differ"
