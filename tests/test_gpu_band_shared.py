"""The band pass of k_score in the teams and its shape per path (chain_kernels.hip: band_slab_publish, band_slab_part).

In a team ONE wave orders a slab's targets by diagonal and publishes the order and a header (skip / index order / sorted, tagged with the
launch's epoch); the other parts of the slab wait for the header and read their own elements.  Every path has a lag of its own
(MM2GB_BAND_LAG_WAVE, _TEAM4, _TEAM8, _WG; MM2GB_BAND_LAG still sets all four), and the mean window from which a chunk takes the band
pass no longer follows the lag.  Every anchor's f / p is compared with the oracle (check_batch); the oracle's answer for a batch is
computed once and shared by the tests of this file.

Not here: a host-only program for the element -> group arithmetic of the published order.  That arithmetic (element e = 64 r + lane,
empty from the slab's length on) is a few lines inside the device functions, not a header the host could include, so there is nothing
to build under a sanitizer.

The `narrow` case of test_gpu_band.py is not narrow in the sense of the band pass's threshold: its reads' mean windows are 412 and 966
anchors (max_gap 20 and 5 at max_dist_x 5000), both above 256, so its chunks take the band pass at the default shape already (31 groups
on the wave path before this change, 102 with MM2GB_BAND_LAG=0).  "No groups at wave lag 0" cannot hold for it whatever the threshold
is; test_the_threshold_does_not_follow_the_lag checks it against the oracle at wave lag 0 and shows the threshold on reads whose mean
window IS below 256: no groups with the wave lag at 0, groups when MM2GB_BAND_LAG=0 lowers the threshold with it."""
import numpy as np
import pytest

import mm2gb_amd  # noqa: F401  (first: a broken build fails here, before an import below could turn it into a skip)
import orc
import synth_cases as sc
from test_gpu_band import TEAMS, batch, cases, engine_with
from test_gpu_parity import check_batch, misc_from

pytestmark = pytest.mark.gpu

TEAM_PATHS = ["teams-of-4", "teams-of-8", "team4-all", "whole-workgroup"]
# the knob that sets a path's lag, and the path's entry in Engine.band_shape()
LAG_KNOB = {"wave": ("MM2GB_BAND_LAG_WAVE", "lag_wave"), "teams-of-4": ("MM2GB_BAND_LAG_TEAM4", "lag_team4"), "team4-all": ("MM2GB_BAND_LAG_TEAM4", "lag_team4"),
            "teams-of-8": ("MM2GB_BAND_LAG_TEAM8", "lag_team8"), "whole-workgroup": ("MM2GB_BAND_LAG_WG", "lag_wg")}
# what DESIGN 4 states for an engine made with no MM2GB_BAND_* knob set
DEFAULT_SHAPE = {"slab": 512, "lag_wave": 0, "lag_team4": 256, "lag_team8": 512, "lag_wg": 512, "min_window": 256}
MUST_BAND = ("repeats", "equal-x", "rescue")
BAND_KNOBS = ["MM2GB_BAND", "MM2GB_BAND_SLAB", "MM2GB_BAND_LAG", "MM2GB_BAND_LAG_WAVE", "MM2GB_BAND_LAG_TEAM4", "MM2GB_BAND_LAG_TEAM8", "MM2GB_BAND_LAG_WG"]


@pytest.fixture(scope="module")
def batches():
    """Every case once, shared and left unchanged."""
    return cases()


_ORACLE = {}
_FILL = orc.chain_fill_many


@pytest.fixture(autouse=True)
def oracle_once(monkeypatch):
    """check_batch asks the oracle through orc.chain_fill_many: answer a batch it has seen (same anchors, offsets, parameters) from
    the first answer.  The band knobs of the caller's environment are cleared: a test sets the ones it means."""
    def fill(a, off, prm, threads=4):
        key = (a.tobytes(), np.asarray(off).tobytes(), tuple(sorted((k, float(v)) for k, v in orc.param_to_dict(prm).items())))
        if key not in _ORACLE:
            _ORACLE[key] = _FILL(a, off, prm, threads=threads)
        return _ORACLE[key]
    monkeypatch.setattr(orc, "chain_fill_many", fill)
    for k in BAND_KNOBS:
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("slab", ["128", "256", "512"])
@pytest.mark.parametrize("path", TEAM_PATHS)
def test_shared_order_on_every_team_path(monkeypatch, batches, path, slab):
    with engine_with(monkeypatch, dict(TEAMS[path], MM2GB_BAND_SLAB=slab)) as e:
        assert e.band_shape()["slab"] == int(slab)
        for name in ("repeats", "equal-x", "ties", "rescue", "reads"):
            a, off = batches[name]
            for kw in (dict(), dict(max_iter=700)):
                check_batch(e, a, off, orc.default_param(**kw))
                if not kw and name in MUST_BAND:
                    assert e.band_groups()[1] > 0, f"{name}: no team swept a band group"


S = 128


def slab_boundary_reads():
    """Repeat-block reads of S k + r anchors: the last slab partial, with 1, fewer than 64, exactly 64 and just over 64 targets; and two
    reads with a colinear tail of more than two slabs behind a repeat block of whole slabs: a sparse tail, whose windows (about 50
    anchors) never reach a lag before their slab -- the skip exit --, and a dense one, whose windows reach back into the block while
    a slab's diagonals lie within 2 bw -- the index-order exit."""
    reads = [sc.sort_by_x(sc.repeat_block(S * 11 + r, 80 + r)) for r in (1, 63, 64, 65)]
    block = sc.sort_by_x(sc.repeat_block(S * 10, 90))
    x_end = int((block[:, 0] & np.uint64(0xffffffff)).max())
    sparse = sc.colinear(3 * S + 17, 91, r0=x_end + 1, q0=20_000, max_gap=200, indel_p=0.0)
    dense = sc.colinear(3 * S + 17, 92, r0=x_end + 1, q0=20_000, max_gap=4, indel_p=0.0)
    return reads + [np.concatenate([block, sparse]), np.concatenate([block, dense])]


def last_slab(a, lag, max_dist_x=5000):
    """(smallest window start, diagonal range) of the read's last slab of S anchors and the slab's jl, the read being one chunk from 0"""
    x = (a[:, 0] & np.uint64(0xffffffff)).astype(np.int64)
    y = (a[:, 1] & np.uint64(0xffffffff)).astype(np.int64)
    assert np.all(np.diff(x) >= 0)
    st = np.searchsorted(x, x - max_dist_x, side="left")
    s0 = (len(a) - 1) // S * S
    d = (x - y)[s0:]
    return int(st[s0:].min()), int(d.max() - d.min()), s0 - lag


def test_the_boundary_reads_take_the_exits_they_are_meant_to():
    """(CPU: the reads alone; marked gpu with the module, it needs none.)"""
    prm = orc.default_param()
    reads = slab_boundary_reads()
    assert [len(a) % S for a in reads[:4]] == [1, 63, 64, 65]
    for a in reads[:4]:
        st_lo, rng, jl = last_slab(a, S)
        assert st_lo < jl and (rng > 2 * prm.bw or len(a) % S == 1)   # sorted (a single target: index order)
    st_lo, rng, jl = last_slab(reads[4], S)
    assert st_lo >= jl                                                # skip, at the full lag and so at every shorter one too...
    assert last_slab(reads[4], 0)[0] < last_slab(reads[4], 0)[2] and last_slab(reads[4], 0)[1] <= 2 * prm.bw   # ... but index order at lag 0
    st_lo, rng, jl = last_slab(reads[5], S)
    assert st_lo < jl and rng <= 2 * prm.bw                           # index order


@pytest.mark.parametrize("path", ["wave"] + TEAM_PATHS)
def test_slab_boundaries(monkeypatch, path):
    a, off = batch(slab_boundary_reads())
    with engine_with(monkeypatch, dict(TEAMS[path], MM2GB_BAND_SLAB=str(S))) as e:
        check_batch(e, a, off, orc.default_param())
        assert e.band_groups()[0 if path == "wave" else 1] > 0


def permuted(seed):
    """Three reads of fixed lengths, their content from `seed`: batches of equal anchor count and different order in every slab."""
    return batch([sc.sort_by_x(sc.repeat_block(4000, seed)), sc.sort_by_x(np.concatenate([sc.repeat_block(3000, seed + 1), sc.noise(1000, seed + 2)])),
                  sc.sort_by_x(sc.repeat_block(2500, seed + 3, xwin=2500))])


@pytest.mark.parametrize("path", TEAM_PATHS)
def test_no_stale_order(monkeypatch, path):
    """One engine, batches of equal size one after the other: what an earlier launch published at the same addresses -- another
    batch's order, or the same batch's -- must not stand in for this launch's."""
    b1, b2, b3 = permuted(101), permuted(201), permuted(301)
    assert len(b1[0]) == len(b2[0]) == len(b3[0]) and np.array_equal(b1[1], b2[1]) and not np.array_equal(b1[0], b2[0])
    prm = orc.default_param()
    with engine_with(monkeypatch, dict(TEAMS[path], MM2GB_BAND_SLAB="256")) as e:
        for a, off in (b1, b2, b3, b1, b2, b2, b3):
            check_batch(e, a, off, prm)
            assert e.band_groups()[1] > 0


@pytest.mark.parametrize("lag", ["0", "64", "256"])
@pytest.mark.parametrize("path", ["wave"] + TEAM_PATHS)
def test_a_lag_per_path(monkeypatch, batches, path, lag):
    """MM2GB_BAND_LAG unset, the path's own knob at 0, 64 and the slab: the oracle's results, and those of the dense sweep of this build."""
    prm = orc.default_param()
    knob, entry = LAG_KNOB[path]
    # the other paths keep their defaults (cut to the slab), and the threshold its own
    want = {k: min(v, 256) for k, v in DEFAULT_SHAPE.items()}
    want[entry] = int(lag)
    res = {}
    for on in ("1", "0"):
        with engine_with(monkeypatch, {**TEAMS[path], "MM2GB_BAND": on, "MM2GB_BAND_SLAB": "256", knob: lag}) as e:
            if on == "1":
                assert e.band_shape() == want
            else:
                assert e.band_shape()["slab"] == 0
            for name in ("repeats", "rescue"):
                a, off = batches[name]
                if on == "1":
                    check_batch(e, a, off, prm)
                    assert e.band_groups()[0 if path == "wave" else 1] > 0
                e.set_misc(misc_from(prm))
                f, p, st = e.score(a, off)
                res[(on, name)] = (f.copy(), p.copy(), st["n_pairs"])
    for name in ("repeats", "rescue"):
        band, dense = res[("1", name)], res[("0", name)]
        assert np.array_equal(band[0], dense[0]) and np.array_equal(band[1], dense[1]) and band[2] == dense[2]


def test_default_shape(monkeypatch):
    with engine_with(monkeypatch, {}) as e:
        assert e.band_shape() == DEFAULT_SHAPE
    with engine_with(monkeypatch, {"MM2GB_BAND_LAG": "128", "MM2GB_BAND_LAG_WAVE": "0"}) as e:        # MM2GB_BAND_LAG still sets every path
        assert e.band_shape() == {"slab": 512, "lag_wave": 128, "lag_team4": 128, "lag_team8": 128, "lag_wg": 128, "min_window": 64}


def test_the_threshold_does_not_follow_the_lag(monkeypatch, batches):
    """Reads whose mean window is below 256 anchors (about 160 and 100) take no band pass with the wave path's lag at 0; that it is the
    threshold that keeps them out shows with MM2GB_BAND_LAG=0, which lowers the threshold with the lags: then they do.  The `narrow` case
    of test_gpu_band.py (mean windows 412 and 966, see the module's text) is checked against the oracle at wave lag 0."""
    prm = orc.default_param()
    thin = batch([sc.colinear(5000, 63, max_gap=60), sc.colinear(3000, 64, max_gap=100)])
    for a in (thin[0][:5000], thin[0][5000:]):
        x = (a[:, 0] & np.uint64(0xffffffff)).astype(np.int64)
        w = np.arange(len(x)) - np.searchsorted(x, x - prm.max_dist_x, side="left")
        assert 64 < w.mean() < 256
    with engine_with(monkeypatch, dict(TEAMS["wave"], MM2GB_BAND_LAG_WAVE="0")) as e:
        check_batch(e, *thin, prm)
        assert e.band_groups() == (0, 0)
        check_batch(e, *batches["narrow"], prm)
    with engine_with(monkeypatch, dict(TEAMS["wave"], MM2GB_BAND_LAG="0")) as e:
        check_batch(e, *thin, prm)
        assert e.band_groups()[0] > 0
