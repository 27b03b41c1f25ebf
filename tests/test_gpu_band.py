"""The band pass of k_score (chain_kernels.hip, band_slab_part): sources older than a lag before the target's slab are swept by
diagonal band.  Forced on at small slabs and lags, through the wave path, the 4- and 8-wave teams and whole-workgroup teams, every
anchor's f / p against the oracle and against the dense sweep (MM2GB_BAND=0) of the same build; the engine's band counters
(mm2gb_engine_band_groups) say that the band pass ran, and on which path."""
import numpy as np
import pytest

import orc
import synth_cases as sc
from test_gpu_parity import check_batch, misc_from

pytestmark = pytest.mark.gpu

mm = pytest.importorskip("mm2gb_amd")

# (gangs off in the team configurations: a small batch would send its heaviest chunks to gangs, which keep the dense sweep)
TEAMS = {"wave": {"MM2GB_NO_COOP": "1"},
         "teams-of-4": {"MM2GB_LONG_MIN_COST": "1", "MM2GB_LONG_MIN_WINDOW": "1", "MM2GB_WIDE_WINDOW": "100000000", "MM2GB_GANG_MAX": "0"},
         "teams-of-8": {"MM2GB_LONG_MIN_COST": "1", "MM2GB_LONG_MIN_WINDOW": "1", "MM2GB_WIDE_WINDOW": "1", "MM2GB_WHOLE_WG_PCT": "0", "MM2GB_GANG_MAX": "0"},
         "team4-all": {"MM2GB_LONG_MIN_COST": "1", "MM2GB_LONG_MIN_WINDOW": "1", "MM2GB_TEAM4_ALL": "1", "MM2GB_WHOLE_WG_PCT": "0", "MM2GB_GANG_MAX": "0"},
         "whole-workgroup": {"MM2GB_LONG_MIN_COST": "1", "MM2GB_LONG_MIN_WINDOW": "1", "MM2GB_WIDE_WINDOW": "1", "MM2GB_WHOLE_WG_PCT": "1", "MM2GB_GANG_MAX": "0"}}
SHAPES = [("128", "64"), ("128", "128"), ("256", "0"), ("512", "512")]


def batch(parts):
    off = np.zeros(len(parts) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(x) for x in parts])
    return np.concatenate(parts).astype(np.uint64), off


def equal_x_runs(seed):
    rng = np.random.default_rng(seed)
    base = sc.sort_by_x(sc.repeat_block(3000, seed, xwin=2500, ywin=6000))
    xs = [int(base[k, 0] & np.uint64(0xffffffff)) for k in (700, 1500, 2600)]
    dups = [sc.pack(np.full(n, 3), np.zeros(n, np.int64), np.full(n, x), np.sort(rng.integers(5000, 11000, n))) for n, x in zip((3, 90, 600), xs)]
    return sc.sort_by_x(np.concatenate([base] + dups))


def several_reads_one_chunk(seed):
    """reads of other strands and rids inside one planner chunk: short reads joined by the planner, then a heavy one"""
    rs = [sc.colinear(40, seed + k, rid=k % 3, rev=k & 1, max_gap=20) for k in range(12)]
    return rs + [sc.sort_by_x(sc.repeat_block(5000, seed + 50, rid=1, rev=1))]


def cases():
    out = {}
    out["repeats"] = batch([sc.sort_by_x(sc.repeat_block(6000, 11)), sc.sort_by_x(np.concatenate([sc.repeat_block(8000, 12), sc.colinear(900, 13)])),
                            sc.read_like(12000, 14)])
    out["equal-x"] = batch([equal_x_runs(21), equal_x_runs(22)])
    out["ties"] = batch([sc.grid_ties(), sc.sort_by_x(np.concatenate([sc.grid_ties(nx=120, ny=30, step=7), sc.repeat_block(3000, 31, xwin=1200, ywin=1500)]))])
    out["reads"] = batch(several_reads_one_chunk(41))
    out["rescue"] = batch([sc.rescue_case(n_noise=7000, n_chain=60, seed=51), sc.sort_by_x(np.concatenate([sc.repeat_block(7000, 52), sc.noise(2000, 53)]))])
    out["narrow"] = batch([sc.colinear(5000, 61, max_gap=20), sc.colinear(3000, 62, max_gap=5, qspan=15)])
    return out


PARAMS = {"default": dict(), "max_iter": dict(max_iter=700), "dist_y": dict(max_dist_y=300, bw=100), "small_bw": dict(max_dist_y=40, bw=8, max_iter=1500)}
# cases whose chunks reach back beyond the lag of every shape above at the default parameters: the band pass must have run on them
MUST_BAND = ("repeats", "equal-x", "rescue")


def engine_with(monkeypatch, env):
    """An engine whose knobs stay set for its whole life: set_misc configures the score kernel again, and reads them again."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return mm.Engine()


@pytest.mark.parametrize("team", list(TEAMS))
@pytest.mark.parametrize("shape", SHAPES, ids=["-".join(s) for s in SHAPES])
def test_band_against_the_oracle(monkeypatch, team, shape):
    env = dict(TEAMS[team], MM2GB_BAND="1", MM2GB_BAND_SLAB=shape[0], MM2GB_BAND_LAG=shape[1])
    side = 0 if team == "wave" else 1
    swept = 0
    with engine_with(monkeypatch, env) as e:
        for name, (a, off) in cases().items():
            for pname, kw in PARAMS.items():
                check_batch(e, a, off, orc.default_param(**kw))
                groups = e.band_groups()
                if team == "wave":
                    assert groups[1] == 0
                swept += groups[side]
                if pname == "default" and name in MUST_BAND:
                    assert sum(groups) > 0, f"{name}: the band pass did not run"
    # the path under test (the wave path, or a team's) swept band groups itself
    assert swept > 0


@pytest.mark.parametrize("team", ["wave", "teams-of-4", "whole-workgroup"])
def test_band_on_and_off_agree(monkeypatch, team):
    a, off = batch([sc.sort_by_x(sc.repeat_block(9000, 71)), sc.read_like(15000, 72), sc.rescue_case(n_noise=5000, seed=73)])
    prm = orc.default_param()
    res = []
    for on in ("1", "0"):
        with engine_with(monkeypatch, dict(TEAMS[team], MM2GB_BAND=on, MM2GB_BAND_SLAB="256", MM2GB_BAND_LAG="128")) as e:
            e.set_misc(misc_from(prm))
            f, p, st = e.score(a, off)
            res.append((f.copy(), p.copy(), st["n_pairs"], e.band_groups()))
    assert sum(res[0][3]) > 0 and res[1][3] == (0, 0)
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1]) and res[0][2] == res[1][2]
