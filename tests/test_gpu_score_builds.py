"""The per-pair builds of the score kernel -- MODE_FAST (no penalty table: bw + 2 > 5120 entries, or chn_pen_skip != 0) and MODE_GENERAL
(cDNA, several segments, or a segment id found on the device) -- at the shapes the rest of the suite sees under the table build only:
chunk lengths around tile pairs, every team size, windows beyond the LDS ring, the rescue state at read boundaries, thousands of tiny
reads; and what only these builds have: the splice preset (bw = max_dist_x = 200 000 while max_dist_y stays 2 000), the last bw with a
table and the first without, the device's fall-back from a table launch, the post-pass with the X-drop off.

Everything is exact: f, p and n_pairs against the CPU oracle (which tests/test_oracle_vs_ref.py and the vectors under tests/golden/
hold to the reference on these very inputs), chains and compacted anchors against the oracle's mg_lchain_dp.  Every test also asserts
Engine.last_score_mode(), so that a parameter set that no longer reaches the build it names fails instead of passing on the table."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import orc
import synth_cases as sc
from test_gpu_parity import fuzz_seed, misc_from, rel, soak_sparse_chunks

pytestmark = pytest.mark.gpu

mm = pytest.importorskip("mm2gb_amd")

LUT, FAST, GENERAL = 0, 1, 2
SPLICE = dict(is_cdna=1, bw=200000, max_dist_x=200000, max_dist_y=2000)
# the per-pair builds by the three ways the host reaches them (the fourth way, the device's own fall-back, has a test of its own)
BUILDS = {"splice": (SPLICE, GENERAL, False), "two-segments": (dict(n_seg=2), GENERAL, True), "bw-5119": (dict(bw=5119), FAST, False)}
TEAM_ENVS = {"planner": {},
             "teams-of-8": {"MM2GB_LONG_MIN_COST": "1", "MM2GB_LONG_MIN_WINDOW": "1", "MM2GB_WIDE_WINDOW": "1", "MM2GB_WHOLE_WG_PCT": "0"},
             "whole-workgroup": {"MM2GB_LONG_MIN_COST": "1", "MM2GB_LONG_MIN_WINDOW": "1", "MM2GB_WIDE_WINDOW": "1", "MM2GB_WHOLE_WG_PCT": "1"},
             "teams-of-4": {"MM2GB_LONG_MIN_COST": "1", "MM2GB_LONG_MIN_WINDOW": "1", "MM2GB_WIDE_WINDOW": "100000000"}}


def offsets(reads):
    off = np.zeros(len(reads) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(r) for r in reads])
    return off


def batch(reads):
    return (np.concatenate(reads) if len(reads) and sum(len(r) for r in reads) else np.zeros((0, 2), np.uint64)), offsets(reads)


def oracle(a, off, prm, threads=4):
    """(f, p as the distance back, n_pairs) of a batch: computed once where several engines score the same batch."""
    fo, po, pairs = orc.chain_fill_many(a, off, prm, threads=threads)
    po_rel = np.concatenate([rel(po[off[r]:off[r + 1]]) for r in range(len(off) - 1)]) if len(a) else np.zeros(0, np.int32)
    return fo, po_rel, pairs


def check(engine, a, off, prm, mode, want=None):
    """One scoring call: every anchor's f and p and the pair count against the oracle, and the build that did the work."""
    fo, po_rel, pairs = want if want is not None else oracle(a, off, prm)
    engine.set_misc(misc_from(prm))
    f, p, st = engine.score(a, off)
    bad = np.flatnonzero((f != fo) | (p != po_rel))
    assert bad.size == 0, f"{bad.size} anchors differ, first at {bad[:5]}: gpu f/p {f[bad[:5]]}/{p[bad[:5]]} oracle {fo[bad[:5]]}/{po_rel[bad[:5]]}"
    assert st["n_pairs"] == pairs
    assert engine.last_score_mode() == mode
    return st


def links(a, p):
    """(dr, dq) of every accepted link i <- p[i] of one read (p absolute, -1 none)."""
    i = np.flatnonzero(p >= 0)
    j = p[i]
    pos = lambda col, k: (a[k, col] & np.uint64(0xffffffff)).astype(np.int64)
    return pos(0, i) - pos(0, j), pos(1, i) - pos(1, j)


def heavy_block(n, seed, exons=30):
    """A dense block inside one splice-sized window (200 000 x 2 000) with a spliced read running through it: every window is cut by
    max_iter alone, and the chain's links span the block."""
    return sc.sort_by_x(np.concatenate([sc.repeat_block(n, seed, xwin=150_000, ywin=1800), sc.spliced(exons, seed + 1, r0=1_900_000, q0=4_000)]))


@pytest.fixture(scope="module")
def engine():
    with mm.Engine() as e:
        yield e


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("env", list(TEAM_ENVS))
def test_chunk_lengths_around_tile_pairs(monkeypatch, env, build):
    """test_gpu_parity's lengths (a chunk ends inside the first tile of a pair, between the two, inside the second, one anchor into the
    next pair), dense and sparse, under its four planner settings -- through the generic sweep_block / in_tile / coop_chunk of each
    per-pair build, plain (max_iter 5000) and tracked (100, 40: the rescue state crosses the tile boundaries)."""
    kw, mode, ids = BUILDS[build]
    for k, v in TEAM_ENVS[env].items():
        monkeypatch.setenv(k, v)
    lengths = [1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 320]
    dense = [sc.sort_by_x(sc.repeat_block(n, 100 + n, xwin=300, ywin=400)) for n in lengths]
    sparse = [sc.colinear(n, 200 + n, max_gap=30) for n in lengths]
    if ids:                                    # (with_segments adds a few anchors: cut back to the length the case is about)
        dense = [sc.with_segments(r, 2, 300 + len(r))[:len(r)] for r in dense]
        sparse = [sc.with_segments(r, 2, 400 + len(r))[:len(r)] for r in sparse]
    a, off = batch(dense + sparse)
    with mm.Engine() as e:
        for max_iter in (5000, 100, 40):
            st = check(e, a, off, orc.default_param(max_iter=max_iter, **kw), mode)
            assert st["n_tracked_chunks"] >= 1 or max_iter == 5000
        # the planner joins short reads into one chunk; alone in its batch a read IS the chunk, so the lengths above are chunk lengths
        prm = orc.default_param(max_iter=100, **kw)
        for r in dense:
            check(e, r, np.array([0, len(r)], np.int64), prm, mode)


TEAM_BATCH = {}


def team_batch(build):
    """Heavy chunks for the team modes and their oracle results at three window limits, made once per build."""
    if build not in TEAM_BATCH:
        kw = BUILDS[build][0] if build == "splice" else dict(bw=9000, max_dist_x=200000, max_dist_y=2000)
        a, off = batch([heavy_block(5000, 51), heavy_block(7000, 53), heavy_block(6000, 55, exons=12), sc.rescue_case(n_noise=6000, n_chain=50, seed=9)])
        prms = {it: orc.default_param(max_iter=it, **kw) for it in (5000, 3000, 160)}
        TEAM_BATCH[build] = (a, off, prms, {it: oracle(a, off, p, threads=8) for it, p in prms.items()})
    return TEAM_BATCH[build]


@pytest.mark.parametrize("build,mode", [("splice", GENERAL), ("bw-9000", FAST)])
@pytest.mark.parametrize("teams", ["planner", "whole-workgroup", "teams-of-8", "teams-of-16", "teams-of-4", "team4-all", "one-wave"])
def test_team_modes(monkeypatch, teams, build, mode):
    """Heavy chunks of the per-pair builds through every team size coop_chunk<MODE, TRACK> is built for, with windows of 5 000 (plain),
    3 000 and 160 anchors (tracked: the rescue state is handed from wave to wave), and with the teams switched off.  The chunk lists are
    asserted, so no case passes without its teams.  What the planner does with a per-pair build (plan_finish): a heavy chunk whose windows
    are narrow against its cost, or all of them under the `teams-of-4` thresholds, goes to a 4-wave team if its widest window fits a
    quarter of the LDS ring (about 3 900 scores without a table in LDS); every other heavy chunk whose window fits a big team's share goes
    to the big-team list.  MM2GB_TEAM4_ALL moves wide-window chunks to 4-wave teams for the table build only (its teams fetch the scores
    their ring share no longer holds from global memory; the per-pair teams do not), so under it these chunks stay on 8-wave teams."""
    env = {"planner": {}, "whole-workgroup": {"MM2GB_WHOLE_WG_PCT": "1"}, "teams-of-8": {"MM2GB_WHOLE_WG_PCT": "0"}, "teams-of-16": {"MM2GB_BIG_TEAM": "16"},
           "teams-of-4": TEAM_ENVS["teams-of-4"],
           "team4-all": {"MM2GB_LONG_MIN_COST": "1", "MM2GB_LONG_MIN_WINDOW": "1", "MM2GB_TEAM4_ALL": "1", "MM2GB_WHOLE_WG_PCT": "0"},
           "one-wave": {"MM2GB_NO_COOP": "1"}}[teams]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    a, off, prms, want = team_batch(build)
    with mm.Engine() as e:
        st = {it: check(e, a, off, prms[it], mode, want[it]) for it in (5000, 3000, 160)}
    # every read of the batch is one chunk, heavy at each of the three limits, its windows cut by max_iter
    assert all(s["n_chunks"] == 4 and s["n_tracked_chunks"] == 4 for s in st.values()), st
    lists = {it: (s["n_long_chunks"], s["n_mid_chunks"]) for it, s in st.items()}
    if teams == "one-wave":
        assert lists == {5000: (0, 0), 3000: (0, 0), 160: (0, 0)}, lists
    elif teams == "teams-of-4":
        assert lists == {5000: (4, 0), 3000: (0, 4), 160: (0, 4)}, lists      # windows of 5 000 do not fit a quarter of the ring
    else:
        assert lists == {5000: (4, 0), 3000: (4, 0), 160: (0, 4)}, lists      # narrow windows: the planner's own choice of 4-wave teams


@pytest.mark.parametrize("max_iter", [9000, 40000, orc.INT32_MAX])
def test_max_iter_beyond_the_lds_ring(engine, max_iter):
    """Without a table in LDS the score ring is larger than under the table build (252 slots of 64 scores against 164), so the sizes at
    which a chunk's widest window stops fitting a team's share lie elsewhere: an 8-wave team has 126 slots, one of them for the tile
    being written, so a window of 8 000 predecessors is the last that fits.  Dense blocks inside one splice-sized window, where max_iter
    and the block alone set the window: 8 001 anchors (widest window 8 000: big-team list) and 8 002 (8 001: one wave), and a block of
    9 000 and one of 3 500 with a spliced read through each."""
    edge = [sc.sort_by_x(sc.repeat_block(n, 80 + n, xwin=150_000, ywin=1800)) for n in (8001, 8002)]
    a, off = batch(edge + [heavy_block(9000, 81), heavy_block(3500, 87)])
    prm = orc.default_param(max_iter=max_iter, **SPLICE)
    st = check(engine, a, off, prm, GENERAL, oracle(a, off, prm, threads=8))
    assert (st["n_chunks"], st["n_long_chunks"], st["n_mid_chunks"]) == (4, 2, 0), st


@pytest.mark.parametrize("kw,ids", [(dict(is_cdna=1), False), (dict(n_seg=2), True)], ids=["cdna", "two-segments"])
def test_rescue_state_restarts_at_every_read(engine, kw, ids):
    """Copies and slices of one repeat-rich read back to back (test_gpu_parity's second construction) with max_dist_x = 200 000: the
    previous read's remembered best anchor (max_ii) is within reach of every anchor of the next read, on the same strand and reference,
    so a rescue state that survives a read boundary in the generic in_tile / run_chunk changes scores."""
    one = sc.sort_by_x(np.concatenate([sc.repeat_block(500, 61, xwin=300, ywin=400), sc.colinear(120, 62, max_gap=20)]))
    if ids:
        one = sc.with_segments(one, 2, 63)
    a, off = batch([one, one[: len(one) // 2], one, one[len(one) // 3:]])
    for max_iter in (7, 63, 200):
        st = check(engine, a, off, orc.default_param(max_iter=max_iter, max_dist_x=200000, bw=100, **kw), GENERAL)
        assert st["n_tracked_chunks"] >= 1


def test_many_tiny_reads(engine):
    """5 000 reads of 0-40 anchors in one micro-batch (test_gpu_parity's, a tenth of the reads): read boundaries every few anchors,
    several per tile, under the splice preset and with segment ids at n_seg = 2."""
    rng = np.random.default_rng(99)
    sizes = rng.integers(0, 41, 5_000)
    off = np.zeros(len(sizes) + 1, dtype=np.int64)
    off[1:] = np.cumsum(sizes)
    n = int(off[-1])
    rid = rng.integers(0, 2, n)
    read_of = np.repeat(np.arange(len(sizes)), sizes)
    pos_in_read = np.arange(n) - off[read_of]
    x = 10_000 + pos_in_read * rng.integers(5, 30, n) + rng.integers(0, 3, n)
    y = 100 + pos_in_read * 17 + rng.integers(0, 9, n)
    sid = rng.integers(0, 2, n)
    for seg, kw in ((np.zeros(n, np.int64), SPLICE), (sid, dict(n_seg=2))):
        a = sc.pack(rid, np.zeros(n, np.int64), x, y, sid=seg)
        a = a[np.lexsort((a[:, 0], read_of))]
        st = check(engine, a, off, orc.default_param(min_cnt=2, min_sc=20, **kw), GENERAL, oracle(a, off, orc.default_param(min_cnt=2, min_sc=20, **kw), threads=8))
        assert st["n_reads"] == 5_000


@pytest.mark.parametrize("clamp", [False, True], ids=["unclamped", "clamped-table"])
@pytest.mark.parametrize("bw", [5117, 5118, 5119, 5120])
def test_table_boundary(monkeypatch, bw, clamp):
    """bw = 5118 is the last parameter set with a penalty table (bw + 2 = LUT_ENTRIES entries: the table starts exactly where ring, scratch
    and team records must have ended), 5119 the first on the per-pair float build.  jump_chain joins blocks by jumps of exactly 5116 ..
    5121 bases, so the links the oracle accepts reach dd == bw and stop there: a table one entry short, a rejecting entry one too early
    or `dd < bw` in the float build loses the last link.  A dense block beside it sends a heavy chunk through the team modes, whose ring
    is what the largest table abuts."""
    if clamp:
        monkeypatch.setenv("MM2GB_LUT_CLAMP", "1")
    jumps = sc.jump_chain([5116, 5117, 5118, 5119, 5120, 5121], 9)
    prm = orc.default_param(bw=bw, max_dist_x=8000, max_dist_y=8000)
    _, p, _ = orc.chain_fill(jumps, prm)
    dr, dq = links(jumps, p)
    dd = np.abs(dr - dq)
    assert dd.max() == bw and sorted(set(dd[dd > 100].tolist())) == list(range(5116, bw + 1))      # the input is decisive
    a, off = batch([jumps, sc.sort_by_x(np.concatenate([sc.repeat_block(5200, 61), sc.colinear(700, 62)]))])
    with mm.Engine() as e:
        st = check(e, a, off, prm, LUT if bw <= 5118 else FAST)
        assert st["n_long_chunks"] + st["n_mid_chunks"] >= 1, st
        check(e, jumps, np.array([0, len(jumps)], np.int64), prm, LUT if bw <= 5118 else FAST)
        # blocks of 400 put the jumps inside tiles and, the fourth, between two; blocks of 6 tiles put every jump between two tiles, so the
        # last link is taken by the in-tile pass in one read and by the sweep of an earlier block in the other
        tiled = sc.jump_chain([5116, 5117, 5118, 5119, 5120, 5121], 10, n=384)
        check(e, tiled, np.array([0, len(tiled)], np.int64), prm, LUT if bw <= 5118 else FAST)


def test_max_dist_y_is_not_raised_to_bw_under_cdna(engine):
    """lchain.c:161 raises max_dist_y to bw unless is_cdna; the splice preset depends on it staying 2 000 under bw = 200 000.  Blocks on
    one diagonal, 2 500 - 150 000 bases apart on both axes (dd == 0): rejected at the splice preset, accepted with is_cdna = 0."""
    rng = np.random.default_rng(17)
    xs, x = [], 1_000_000
    for g in (2500, 2001, 9000, 40_000, 150_000, 3000, 199_000, 2600):
        step = rng.integers(5, 30, 25)
        xs.append(x + np.cumsum(step))
        x = int(xs[-1][-1]) + g
    xs = np.concatenate(xs)
    a = sc.pack(np.full(len(xs), 3), np.zeros(len(xs), np.int64), xs, xs - 999_000)
    off = np.array([0, len(a)], np.int64)
    cdna, genomic = orc.default_param(**SPLICE), orc.default_param(**dict(SPLICE, is_cdna=0, n_seg=2))
    pc, pg = orc.chain_fill(a, cdna)[1], orc.chain_fill(a, genomic)[1]
    assert links(a, pc)[1].max() <= 2000 < links(a, pg)[1].max() and not np.array_equal(pc, pg)      # the two rules differ on this input
    check(engine, a, off, cdna, GENERAL)
    check(engine, a, off, genomic, GENERAL)


def test_device_fallback_from_a_table_launch():
    """The host chose the table build (n_seg = 1, default bw); one late read of a batch with heavy chunks carries segment ids, or a query
    position the table sweep is not exact for.  k_window raises the flag, the table instance of k_score exits, the planner has planned
    without tile pairs and gangs, and the GENERAL (or FAST) instance scores every read with the n_seg = 1 parameters and the table
    launch's smaller ring.  The flag word belongs to one micro-batch: the same engine is back on the table for the next one."""
    heavy = [sc.sort_by_x(sc.repeat_block(6000, 51)), sc.sort_by_x(np.concatenate([sc.repeat_block(7000, 52), sc.colinear(900, 53)])),
             sc.read_like(9000, 54), sc.rescue_case(n_noise=6000, n_chain=50, seed=9)]
    late = sc.read_like(4000, 55)
    far = late.copy()
    far[:, 1] += np.uint64((1 << 27) + 12345)
    plain, with_ids, with_far = batch(heavy + [late]), batch(heavy + [sc.with_segments(late, 2, 56, share=0.05)]), batch(heavy + [far])
    with mm.Engine() as e:
        for max_iter in (5000, 160):
            prm = orc.default_param(max_iter=max_iter)
            want = oracle(*plain, prm)
            for (a, off), mode in ((with_ids, GENERAL), (plain, LUT), (with_far, FAST), (plain, LUT)):
                st = check(e, a, off, prm, mode, want if a is plain[0] else None)
                assert st["n_long_chunks"] + st["n_mid_chunks"] >= 3 and st["n_tracked_chunks"] >= 2, (mode, st)


def chains_against_oracle(res, a, off, prm):
    for r in range(len(off) - 1):
        o = orc.lchain_dp(a[off[r]:off[r + 1]], prm, want_fp=False)
        assert np.array_equal(res[r][0], o["u"]), f"read {r}: chains differ ({len(res[r][0])} vs {len(o['u'])})"
        assert np.array_equal(res[r][1], o["a_out"]), f"read {r}: compacted anchors differ"


def test_device_post_pass_with_the_x_drop_off(engine):
    """is_cdna lifts mg_chain_backtrack's max_drop from bw to INT32_MAX.  qins_chain's chains lose more than bw on their way through runs
    of query insertions: the same f / p give other chains with the X-drop on (asserted), so a post-pass that takes bw under is_cdna
    fails here.  Device post-pass against the oracle and against the host post-pass on the same scores; also the spliced read."""
    q = sc.qins_chain(150, 7)
    kw = dict(bw=100, pen_gap=np.float32(1.0), min_cnt=2, min_sc=15)
    o = orc.lchain_dp(q, orc.default_param(is_cdna=1, **kw))
    u_on, _ = orc.backtrack_compact(q, o["f"], o["p"], orc.default_param(is_cdna=0, **kw))
    assert len(u_on) != len(o["u"]) and len(o["u"]) >= 1
    spl = sc.spliced(60, 5, noise_n=3000)
    for reads, prm in (([q, sc.qins_chain(40, 8), q[:300]], orc.default_param(is_cdna=1, **kw)), ([spl, q, heavy_block(2000, 91)], orc.default_param(**SPLICE))):
        a, off = batch(reads)
        check(engine, a, off, prm, GENERAL)
        dev, _ = engine.chain_gpu(a, off)
        assert engine.last_score_mode() == GENERAL
        host, _ = engine.chain(a, off, threads=4)
        chains_against_oracle(dev, a, off, prm)
        chains_against_oracle(host, a, off, prm)


@pytest.mark.parametrize("max_skip", [25, 0])
def test_skip_limited_walk_at_the_splice_preset(max_skip):
    """Engine(chain_skip=True): mg_lchain_dp's results at a finite max_skip, at the splice preset (the walk calls pair_score with every
    cDNA branch, over windows of up to 5 000 candidates)."""
    a, off = batch([sc.spliced(60, 5, noise_n=3000), heavy_block(3000, 93), sc.spliced(25, 94, qins_p=0.5)])
    prm = orc.default_param(max_skip=max_skip, **SPLICE)
    misc = misc_from(prm)
    misc.max_skip = max_skip
    fo, po_rel, pairs = oracle(a, off, prm)
    with mm.Engine(misc=misc, chain_skip=True) as e:
        f, p, st = e.score(a, off)
        assert e.last_score_form() == 1 and e.last_score_mode() == GENERAL
        assert np.array_equal(f, fo) and np.array_equal(p, po_rel) and st["n_pairs"] == pairs
        for res, _ in (e.chain(a, off, threads=2), e.chain_gpu(a, off)):
            chains_against_oracle(res, a, off, prm)
    unlimited = oracle(a, off, orc.default_param(**SPLICE))
    assert not (np.array_equal(unlimited[0], fo) and np.array_equal(unlimited[1], po_rel))      # the limit matters on this input


def test_fuzz_general(engine, tmp_path):
    """28 batches of synth_cases.fuzz_case_general, four of each parameter class (the class is cycled by the iteration, so all seven
    occur whatever the seed): scores against the oracle; one batch in every seven -- a different class each time -- also takes the device
    post-pass against the oracle.  Class e (segment ids under a table launch) is followed by the same batch without ids on the same
    engine, which must be back on the table: the three builds all occur.  A failing batch is written in tests/fuzz_soak.py's format (anchors, offsets,
    GPU f / p, parameters) to the test's temporary directory, whose path is printed."""
    seed = fuzz_seed() ^ 0x9e4
    print(f"fuzz seed {seed} (hash of mm2-gb_amd/csrc xor 0x9e4; MM2GB_FUZZ_SEED overrides)")
    rng = np.random.default_rng(seed)
    want_mode = dict(a=GENERAL, b=GENERAL, c=GENERAL, d=GENERAL, e=GENERAL, f=FAST, g=FAST)
    seen = set()
    for it in range(28):
        a, off, kw = sc.fuzz_case_general(rng, it)
        cls = sc.GENERAL_CLASSES[it % 7]
        prm = orc.default_param(**kw)
        try:
            check(engine, a, off, prm, want_mode[cls])        # (an empty batch runs nothing: the host's choice, which is the same build)
            seen.add(engine.last_score_mode())
            if it % 7 == it // 7 and off[-1]:
                dev, _ = engine.chain_gpu(a, off)
                chains_against_oracle(dev, a, off, prm)
            if cls == "e":
                bare = a.copy()
                bare[:, 1] &= ~sc.SEG_MASK
                check(engine, bare, off, prm, LUT)
                seen.add(engine.last_score_mode())
        except AssertionError:
            engine.set_misc(misc_from(prm))
            f, p, _ = engine.score(a, off)
            plain = {k: float(v) for k, v in kw.items()}
            dump = tmp_path / f"fuzz_fail_general_{seed}_{it}.npz"
            np.savez(dump, a=a, off=off, f=f, p=p, kw=json.dumps(plain))
            print("iteration", it, "class", cls, "parameters", plain, "batch written to", dump)
            raise
    assert seen == {LUT, FAST, GENERAL}


def test_fuzz_soak_general_eight_engine_configurations():
    """tests/fuzz_soak.py --general in a child process: 28 batches of fuzz_case_general under the eight engine configurations of --teams
    (default planner, every chunk on 8-wave, whole-workgroup and 4-wave teams, 4-wave teams with wide windows, gangs, the large-batch
    form at the default thresholds and with heavy chunks), each against the oracle on every anchor, the default engine's device post-pass
    against the host post-pass.  The per-pair builds run through the sparse list with run_chunk: both engines of the large-batch form
    must have scored chunks of it."""
    here = os.path.dirname(os.path.abspath(__file__))
    seed = fuzz_seed() ^ 0x6e4
    r = subprocess.run([sys.executable, os.path.join(here, "fuzz_soak.py"), str(seed), "--general", "--teams", "--post", "--iters", "28"],
                       capture_output=True, text=True, timeout=600)
    print(r.stdout[-1500:])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert f"seed {seed} clean over 28 batches" in r.stdout
    scored = soak_sparse_chunks(r.stdout)
    assert set(scored) == {"large", "large-teams"} and min(scored.values()) > 0, scored
