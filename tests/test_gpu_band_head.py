"""Head stages and short last stages of the band pass (chain_kernels.hip, band_group).

A group of 64 targets scans the sources [smallest window start, jl) and sweeps its hits 64 at a time.  A stage whose first source lies
before the group's LARGEST window start is a head stage: some targets' windows start inside or after it.  A head stage that is left
of every target and within the free span takes the free or FAR form with one test per source, "source index >= this target's window
start"; the others keep the band-edge form.  The last stage of a scan is swept over its own sources only, to the next multiple of 4.

One read per case, at most about 1 500 anchors, windows cut by a small max_iter (st = i - MAX_ITER): filler 20 000 off the targets'
diagonal, old sources on it placed by their distance from the first target's window start, a lag and more of filler, two slabs of
targets from anchor N0 on.  band_model() below applies band_group's own rules to a read on the CPU -- the order of a slab's targets, a
group's hits, its stages and the form each takes -- and every case asserts from it and the oracle alone that it tests what it is for:
those tests need no GPU and are not marked for one.

Every anchor's f / p is checked against the oracle and against the dense sweep (MM2GB_BAND=0) of the same build, on the wave path, in
teams of 4 and in whole-workgroup teams, at slab / lag 128 / 64 and 256 / 128."""
import numpy as np
import pytest

import mm2gb_amd  # noqa: F401  (first: a broken build fails here, before an import below could turn it into a skip)
import orc
import synth_cases as sc
from test_gpu_band import TEAMS, batch, engine_with
from test_gpu_parity import check_batch, misc_from
from test_gpu_sparse_fill import window_starts


SHAPES = [(128, 64), (256, 128)]
PATHS = ["wave", "teams-of-4", "whole-workgroup"]
MAX_ITER = 300
N0 = 512                       # the first target: a slab boundary at either shape, more than MAX_ITER anchors into the read
X0, Y0 = 2_000_000, 60_000
FILLER_OFF = 20_000
SPAN = 15
LAST = (1, 2, 3, 4, 5, 61, 62, 63)


def param(**kw):
    return orc.default_param(max_iter=MAX_ITER, **kw)


# ---- band_group's rules on the CPU ----------------------------------------------------------------------------------------------------

def band_model(a, slab, lag, prm):
    """The stages of every group of every slab of ONE read that is one chunk: dicts with the group's targets, the stage's sources
    (indices, ascending), whether it is a head stage, its form (far / free / no_check / edge) and, for a last, partial stage, its
    number of sources (0: a full stage)."""
    off = np.array([0, len(a)], np.int64)
    st, _ = window_starts(a, off, prm)
    x = (a[:, 0].astype(np.int64) & 0xffffffff)
    y = (a[:, 1].astype(np.int64) & 0xffffffff)
    q = (a[:, 1].astype(np.int64) >> 32) & 0xff
    d = x - y
    bw, dq_lim = prm.bw, min(prm.max_dist_x, prm.max_dist_y)
    free_sweep = dq_lim > 2 * bw
    out = []
    for s0 in range(0, len(a), slab):
        jl = s0 - lag
        tg = np.arange(s0, min(s0 + slab, len(a)))
        if s0 < 128 or st[tg].min() >= jl:
            continue
        dmin = d[tg].min()
        rng_d = d[tg].max() - dmin
        if rng_d <= 2 * bw:
            order = tg
        else:
            sh = int(rng_d >> 22).bit_length()
            order = tg[np.lexsort((tg, (d[tg] - dmin) >> sh))]
        for g in range(0, len(order), 64):
            grp = order[g:g + 64]
            lo_all, hi_st = st[grp].min(), st[grp].max()
            if lo_all >= jl:
                continue
            src = np.arange(lo_all, jl)
            hits = src[(d[src] >= d[grp].min() - bw) & (d[src] <= d[grp].max() + bw)]
            gx_min, gx_max = x[grp].min(), x[grp].max()
            for k in range(0, len(hits), 64):
                s = hits[k:k + 64]
                inside = s[0] >= hi_st
                left = gx_min > x[s].max()
                free = left and free_sweep and gx_max - x[s].min() <= dq_lim - bw
                far = free and np.all(q[s] + bw <= gx_min - x[s])
                form = "far" if far else "free" if free else "no_check" if inside and left else "edge"
                out.append(dict(slab=s0, targets=grp, sources=s, head=not inside, form=form, last=len(s) if len(s) < 64 else 0))
    return out


def stages_with(model, **want):
    return [s for s in model if all(s[k] == v for k, v in want.items())]


# ---- reads ---------------------------------------------------------------------------------------------------------------------------

def lay_out(slab, step, on_diagonal, seed, targets="jitter", off_b=0):
    """Anchors [0, N0) at `step` on the reference, filler but for `on_diagonal`: (first, length[, every[, shift]]) stretches, `first`
    counted from the first target's window start N0 - MAX_ITER, that lie on the targets' diagonal, or `shift` off it (every: only each
    `every`-th anchor of the stretch, the others off_b off it: a second diagonal).  targets:
      "jitter" -- at `step` like the sources, within 40 of the diagonal;
      "two"    -- the same, alternately on the diagonal and off_b off it;
      "level"  -- one base apart, all at ONE query position, so that no target chains to another and every target takes the best
                  old source its window holds; the first target lies on the diagonal."""
    n = N0 + 2 * slab
    rng = np.random.default_rng(seed)
    x = X0 + step * np.arange(n, dtype=np.int64)
    t = np.arange(N0, n)
    if targets == "level":
        x[t] = x[N0 - 1] + step + (t - N0)
    y = x - (X0 - Y0)
    fill = np.ones(N0, bool)
    lo = N0 - MAX_ITER
    for first, length, *more in on_diagonal:
        every, shift = (more + [1, 0][len(more):])[:2]
        k = np.arange(lo + first, lo + first + length)
        other = k[(k - k[0]) % every != 0]
        k = k[(k - k[0]) % every == 0]
        y[other] -= off_b
        fill[other] = False
        fill[k] = False
        y[k] -= shift
    y[:N0][fill] -= FILLER_OFF
    if targets == "level":
        y[t] = y[N0]
    if targets == "two":
        y[t[1::2]] -= off_b
    if targets != "level":
        y[t] += rng.integers(-40, 41, len(t))
    return sc.pack(np.full(n, 3), np.zeros(n, np.int64), x, y, qspan=SPAN)


def read_with_a_tie(slab):
    """test_gpu_band_scan's tie, the first source A in the head stage of the first group: A, 70 sources that every group's band test
    lets in and that score for nobody, then B, which scores the same for the first target -- the 72nd hit, in the stage after A's."""
    n = N0 + 2 * slab
    rng = np.random.default_rng(11 + slab)
    x = X0 + np.arange(n, dtype=np.int64)
    y = x - (X0 - Y0)
    y[:N0] -= FILLER_OFF
    y[N0 + 1:] += rng.integers(-40, 41, n - N0 - 1)
    ia = N0 - MAX_ITER + 5
    ib = ia + 71
    y[ia] = x[ia] - (X0 - Y0) - 60
    y[ib] = x[ib] - (X0 - Y0) + 60
    y[ia + 1:ib] = y[N0] + 100 - np.arange(70)
    return sc.pack(np.full(n, 3), np.zeros(n, np.int64), x, y, qspan=SPAN), ia, ib


def x_reach_read(slab):
    """Window starts set by the reach on the reference (max_iter 5000): sources in clusters of 80 at step 1, 700 between clusters, the
    second cluster (anchors 80 to 159) on the targets' diagonal; targets at step 10, whose window starts cross a cluster one source per ten
    targets and then stay for 60 targets at the next cluster's first source."""
    n = N0 + 2 * slab
    k = np.arange(N0, dtype=np.int64)
    xs = X0 + (k // 80) * 780 + k % 80
    reach = orc.default_param().max_dist_x
    xt = xs[100] + reach + 10 * np.arange(n - N0, dtype=np.int64)
    x = np.concatenate([xs, xt])
    y = x - (X0 - Y0)
    fill = np.ones(N0, bool)
    fill[80:160] = False
    y[:N0][fill] -= FILLER_OFF
    y[N0:] += np.random.default_rng(5 + slab).integers(-40, 41, n - N0)
    return sc.pack(np.full(n, 3), np.zeros(n, np.int64), x, y, qspan=SPAN)


def cases(slab):
    """name -> (anchors, parameters, what the model must find: keyword sets for stages_with, each with at least one stage)"""
    out = {}
    # the first group: a full head stage, whose last source scores highest for the first target, then a last stage of 36 inside every
    # window (two stretches 150 and 400 off the targets' diagonal on either side: the second cannot chain to the first)
    parts = [(5, 64, 1, -150), (69, 36, 1, 400)]
    out["index-free"] = (lay_out(slab, 1, parts, 1), param(), [dict(head=True, form="free", last=0), dict(head=False, form="free", last=36)])
    out["index-far"] = (lay_out(slab, 3, parts, 2), param(), [dict(head=True, form="far", last=0), dict(head=False, form="far", last=36)])
    # a sorted slab: targets alternately on two diagonals 1200 apart, the old stretch one anchor of four on the first and three on the
    # second; a diagonal's group holds targets from all over the slab
    out["sorted"] = (lay_out(slab, 1, [(5, 160, 4)], 3, targets="two", off_b=1200), param(), [dict(head=True, form="free", last=0)])
    out["x-reach"] = (x_reach_read(slab), orc.default_param(), [dict(head=True, form="edge", last=60)])
    # the old stretch ends with the scan's highest score, inside the windows of the group's first targets and before those of the others
    out["adversarial-free"] = (lay_out(slab, 1, [(5, 60)], 5, targets="level"), param(), [dict(head=True, form="free", last=60), dict(head=True, form="free", last=1)])
    out["adversarial-far"] = (lay_out(slab, 4, [(5, 60)], 6, targets="level"), param(), [dict(head=True, form="far", last=60), dict(head=True, form="far", last=1)])
    short_y = param(max_dist_y=2000)                 # a free span of 1500: the second stage of the scan lies beyond it
    for r in LAST:
        out[f"last-{r}-head-free"] = (lay_out(slab, 1, [(5, r)], 10 + r, targets="level"), param(), [dict(head=True, form="free", last=r)])
        out[f"last-{r}-head-far"] = (lay_out(slab, 4, [(5, r)], 20 + r, targets="level"), param(), [dict(head=True, form="far", last=r)])
        out[f"last-{r}-free"] = (lay_out(slab, 1, [(5, 64 + r)], 30 + r, targets="level"), param(), [dict(head=False, form="free", last=r)])
        out[f"last-{r}-far"] = (lay_out(slab, 4, [(5, 64 + r)], 40 + r, targets="level"), param(), [dict(head=False, form="far", last=r)])
        out[f"last-{r}-no-check"] = (lay_out(slab, 7, [(5, 64 + r)], 50 + r, targets="level"), short_y, [dict(head=False, form="no_check", last=r)])
    return out


@pytest.fixture(scope="module")
def reads():
    """Every case once, with the oracle's f / p and the model's stages: shared by the tests below and left unchanged."""
    out = {}
    for slab, lag in SHAPES:
        for name, (a, prm, want) in cases(slab).items():
            xs = a[:, 0].astype(np.int64) & 0xffffffff
            assert np.all(np.diff(xs) >= 0) and len(a) <= 1500
            f, p, _ = orc.chain_fill_many(*batch([a]), prm, threads=1)
            out[(slab, lag, name)] = (a, prm, want, f, p, band_model(a, slab, lag, prm))
        a, ia, ib = read_with_a_tie(slab)
        f, p, _ = orc.chain_fill_many(*batch([a]), param(), threads=1)
        out[(slab, lag, "tie")] = (a, param(), [dict(head=True, form="free", last=0)], f, p, band_model(a, slab, lag, param()), ia, ib)
    return out


# ---- what the cases are for, from the model and the oracle alone (no device) ----------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=["-".join(map(str, s)) for s in SHAPES])
def test_the_cases_hold_the_stages_they_are_for(reads, shape):
    """Under band_group's rules every case has a head stage, the stages of the kinds it names, and a target whose predecessor lies in
    a head stage."""
    for name in list(cases(shape[0])) + ["tie"]:
        a, prm, want, f, p, model = reads[shape + (name,)][:6]
        st, _ = window_starts(a, np.array([0, len(a)], np.int64), prm)
        if name != "x-reach":                                       # every window of a target is cut by max_iter
            assert np.all(st[N0:] == np.arange(N0, len(a)) - MAX_ITER)
        heads = stages_with(model, head=True)
        assert heads, f"{name}: no head stage"
        for kw in want:
            assert stages_with(model, **kw), f"{name}: no stage with {kw}; the model has {[(s['head'], s['form'], s['last']) for s in model]}"
        if name != "tie":                                           # (the tie's winner lies in the stage after the head: its own test)
            assert any(np.isin(p[s["targets"]], s["sources"]).any() for s in heads), f"{name}: no target's predecessor lies in a head stage"


@pytest.mark.parametrize("shape", SHAPES, ids=["-".join(map(str, s)) for s in SHAPES])
def test_the_sorted_slabs_have_heads_of_two_stages(reads, shape):
    a, prm, want, f, p, model = reads[shape + ("sorted",)]
    d = (a[:, 0].astype(np.int64) & 0xffffffff) - (a[:, 1].astype(np.int64) & 0xffffffff)
    firsts = {}
    for s in stages_with(model, head=True):
        firsts.setdefault((s["slab"], int(s["targets"][0])), []).append(s)
    assert any(len(v) >= 2 for v in firsts.values()), "no group with a head of two stages"
    tg = np.arange(N0, N0 + shape[0])
    assert d[tg].max() - d[tg].min() > 2 * prm.bw                  # the slab is sorted by diagonal ...
    wide = [s for s in model if s["slab"] == N0 and np.ptp(s["targets"]) > 64]
    assert wide, "no group holds targets from all over the slab"   # ... and a group's targets are not consecutive


@pytest.mark.parametrize("shape", SHAPES, ids=["-".join(map(str, s)) for s in SHAPES])
def test_the_x_reach_case_has_stages_inside_and_outside_a_window(reads, shape):
    a, prm, want, f, p, model = reads[shape + ("x-reach",)]
    st, _ = window_starts(a, np.array([0, len(a)], np.int64), prm)
    assert np.all(np.arange(len(a)) - st < prm.max_iter)           # no window is cut by max_iter
    tg = np.arange(N0, len(a))
    counts = np.unique(st[tg], return_counts=True)[1]
    assert counts.max() >= 30 and (counts == 1).sum() >= 5         # several targets per start, and starts one target each
    ok = False
    for s in stages_with(model, head=True):
        t_st = st[s["targets"]]
        ok |= bool((t_st <= s["sources"][0]).any() and (t_st > s["sources"][-1]).any())
    assert ok, "no head stage that is wholly inside one target's window and wholly outside another's"


@pytest.mark.parametrize("shape", SHAPES, ids=["-".join(map(str, s)) for s in SHAPES])
@pytest.mark.parametrize("form", ["free", "far"])
def test_the_out_of_window_source_would_have_won(reads, shape, form):
    """The adversarial case: the last anchor S of the old stretch holds the highest score of the scan; some target whose window
    starts right after S would score more from S than it does, and does not take it; another target of the same group takes it."""
    a, prm, want, f, p, model = reads[shape + (f"adversarial-{form}",)]
    st, _ = window_starts(a, np.array([0, len(a)], np.int64), prm)
    s_idx = N0 - MAX_ITER + 5 + 60 - 1
    found = False
    for s in stages_with(model, head=True, form=form):
        if s_idx not in s["sources"]:
            continue
        assert f[s_idx] == f[s["sources"]].max()
        t = s["targets"]
        shut_out = [i for i in t if st[i] > s_idx and st[i] <= s_idx + 2]
        takes = [i for i in t if st[i] <= s_idx and p[i] == s_idx]
        for i in shut_out:
            sc_pair = orc.pair_score(a[i], a[s_idx], prm)
            if sc_pair > -(1 << 30) and f[s_idx] + sc_pair > f[i] and p[i] != s_idx and takes:
                found = True
    assert found, "no target that S would have won for, just outside its window, beside one that takes S"


@pytest.mark.parametrize("shape", SHAPES, ids=["-".join(map(str, s)) for s in SHAPES])
def test_the_tie_lies_across_the_head_stage_boundary(reads, shape):
    a, prm, want, f, p, model, ia, ib = reads[shape + ("tie",)]
    from_a, from_b = f[ia] + orc.pair_score(a[N0], a[ia], prm), f[ib] + orc.pair_score(a[N0], a[ib], prm)
    assert from_a == from_b == f[N0] and p[N0] == ib
    mine = [s for s in model if N0 in s["targets"]]
    with_a = [s for s in mine if ia in s["sources"]]
    with_b = [s for s in mine if ib in s["sources"]]
    assert len(with_a) == 1 and len(with_b) == 1 and with_a[0]["head"] and not with_b[0]["head"]
    assert with_a[0]["sources"][-1] < with_b[0]["sources"][0] and with_a[0]["form"] == "free"


# ---- the device ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("shape", SHAPES, ids=["-".join(map(str, s)) for s in SHAPES])
def test_heads_and_last_stages_against_the_oracle_and_the_dense_sweep(monkeypatch, reads, shape, path):
    slab, lag = shape
    side = 0 if path == "wave" else 1
    names = list(cases(slab)) + ["tie"]
    res = {}
    for on in ("1", "0"):
        with engine_with(monkeypatch, dict(TEAMS[path], MM2GB_BAND=on, MM2GB_BAND_SLAB=str(slab), MM2GB_BAND_LAG=str(lag))) as e:
            for name in names:
                a, prm = reads[shape + (name,)][:2]
                a, off = batch([a])
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
