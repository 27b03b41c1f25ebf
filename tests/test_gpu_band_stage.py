"""The stage boundary of the band pass's hit compaction (chain_kernels.hip, band_group): the hits of a scan go to the lanes of a stage
of 64, a full stage is swept and the hits that did not fit are carried to the first lanes of the next one; the last, partial stage is
swept in one more trip of the same loop.

One read per case: five filler anchors, so that the run starts off a 64 boundary and a scan block holds hits and misses; a run of H
old sources on one diagonal; then more than a lag of filler anchors -- every filler's diagonal lies 20 000 from the run's (bw is 500
and a slab of targets spans under 100, so no group's band test ever lets one in); then two slabs of targets within 40 of the run's
diagonal, the first of them starting on a slab boundary of the read.  The whole read spans under max_dist_x and holds fewer
than max_iter anchors, so every window reaches back to the run.  For the first slab of targets the band's sources are the run and the
filler: exactly H hits out of scan blocks that the run does not fill evenly (the first holds 59 of them), i.e. hits carried over to the
next stage's first lanes, H // 64 full stages and a last one of H % 64; the second slab adds the targets of the first that are older
than its lag.  The run's scores grow along it, so a target whose band best lies in the run takes the run's LAST anchor -- the one in
the last stage, or carried over a stage boundary -- and a lost or repeated stage changes f and p.

Every anchor's f / p is checked against the oracle and against the dense sweep (MM2GB_BAND=0) of the same engine build, on the wave
path, in teams of 4 and in whole-workgroup teams, at slab / lag 128 / 64 and 256 / 128."""
import numpy as np
import pytest

import mm2gb_amd  # noqa: F401  (first: a broken build fails here, before an import below could turn it into a skip)
import orc
import synth_cases as sc
from test_gpu_band import TEAMS, batch, engine_with
from test_gpu_parity import check_batch, misc_from

pytestmark = pytest.mark.gpu

RUN_LENGTHS = [0, 1, 63, 64, 65, 127, 128, 129, 200]
SHAPES = [(128, 64), (256, 128)]
PATHS = ["wave", "teams-of-4", "whole-workgroup"]
STEP = 3                       # reference distance between consecutive anchors: 1024 * 3 < max_dist_x = 5000
LEAD = 5                       # filler anchors before the run
X0, Y0 = 1_000_000, 60_000
FILLER_OFF = 20_000            # the filler's distance from the run's diagonal


def read_with_run(h, slab, lag, seed=5):
    """(anchors, index of the first target): filler [0, LEAD), run [LEAD, LEAD + h), filler [LEAD + h, n0), targets [n0, n0 + 2 * slab);
    n0 the first slab boundary with more than a lag of filler before it."""
    rng = np.random.default_rng(seed + 1000 * h + slab)
    n0 = slab * ((LEAD + h + lag + 1 + slab - 1) // slab)
    n = n0 + 2 * slab
    x = X0 + STEP * np.arange(n, dtype=np.int64)
    y = x - (X0 - Y0)                                              # the run's diagonal
    y[:LEAD] -= FILLER_OFF                                         # (query positions stay positive: Y0 > FILLER_OFF)
    y[LEAD + h:n0] -= FILLER_OFF
    y[n0:] += rng.integers(-40, 41, n - n0)
    return sc.pack(np.full(n, 3), np.zeros(n, np.int64), x, y), n0


@pytest.fixture(scope="module")
def reads():
    """Every case once, with the oracle's f / p: shared by the tests below and left unchanged."""
    prm = orc.default_param()
    out = {}
    for slab, lag in SHAPES:
        for h in RUN_LENGTHS:
            a, n0 = read_with_run(h, slab, lag)
            assert n0 - LEAD - h > lag and STEP * len(a) < prm.max_dist_x and len(a) < prm.max_iter
            assert np.all(np.diff(a[:, 0].astype(np.int64)) > 0)
            f, p, _ = orc.chain_fill_many(*batch([a]), prm, threads=1)
            out[(slab, lag, h)] = (a, n0, f, p)
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=["-".join(map(str, s)) for s in SHAPES])
def test_a_target_takes_its_predecessor_from_the_run(reads, shape):
    """Without this a lost stage would go unnoticed: for each H > 0 some target's best predecessor is an anchor of the old run -- and,
    the run's scores growing, its last one.  (CPU: the oracle alone; marked gpu with the module, it needs none.)"""
    for h in RUN_LENGTHS[1:]:
        a, n0, f, p = reads[shape + (h,)]
        from_run = np.flatnonzero((p[n0:] >= LEAD) & (p[n0:] < LEAD + h))
        assert from_run.size > 0, f"H = {h}: no target chains to the run"
        assert np.all(p[n0:][from_run] == LEAD + h - 1)
        assert np.all(np.diff(f[LEAD:LEAD + h]) > 0)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("shape", SHAPES, ids=["-".join(map(str, s)) for s in SHAPES])
def test_stage_boundaries_against_the_oracle_and_the_dense_sweep(monkeypatch, reads, shape, path):
    slab, lag = shape
    prm = orc.default_param()
    side = 0 if path == "wave" else 1
    res = {}
    for on in ("1", "0"):
        with engine_with(monkeypatch, dict(TEAMS[path], MM2GB_BAND=on, MM2GB_BAND_SLAB=str(slab), MM2GB_BAND_LAG=str(lag))) as e:
            for h in RUN_LENGTHS:
                a, off = batch([reads[shape + (h,)][0]])
                if on == "1":
                    check_batch(e, a, off, prm, threads=1)          # every anchor's f / p against the oracle
                e.set_misc(misc_from(prm))
                f, p, st = e.score(a, off)
                groups = e.band_groups()
                if on == "0":
                    assert groups == (0, 0)
                elif h > 0:
                    assert groups[side] > 0, f"H = {h}: the band pass did not run on the {path} path: {groups}"
                    if path == "wave":
                        assert groups[1] == 0
                res[(on, h)] = (f.copy(), p.copy(), st["n_pairs"])
    for h in RUN_LENGTHS:
        band, dense = res[("1", h)], res[("0", h)]
        assert np.array_equal(band[0], dense[0]) and np.array_equal(band[1], dense[1]) and band[2] == dense[2], f"H = {h}: band and dense sweep differ"
