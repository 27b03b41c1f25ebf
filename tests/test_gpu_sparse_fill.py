"""The planner's sparse list and its lean scorer (chain_kernels.hip: plan_finish, sparse_chunk, sparse_take): stretches of isolated
anchors -- no window wider than MM2GB_SPARSE_MAX_WINDOW -- are scored by a function of their own in the score kernel's last phase,
claimed eight at a time.  Every anchor's f / p against the oracle; Engine.sparse_chunks() says that the path under test ran: it is
the length of the list, which a numpy model of the planner's rule (expected_sparse) gives independently of the device."""
import numpy as np
import pytest

import orc
import synth_cases as sc
from test_gpu_band import PARAMS, TEAMS, batch
from test_gpu_parity import check_batch, misc_from

pytestmark = pytest.mark.gpu

mm = pytest.importorskip("mm2gb_amd")

BLOCK = 1024          # anchors per planning block
SPARSE_W = 63         # the default MM2GB_SPARSE_MAX_WINDOW
GAP = 10_000          # reference distance between isolated anchors: beyond every max_dist_x in use (5000)
# The team configurations of test_gpu_band make EVERY chunk heavy (MM2GB_LONG_MIN_WINDOW=1), and a heavy chunk is never sparse.  A sparse
# chunk costs at most (63 + 16) per anchor, so a threshold of 80 keeps every chunk with a mean window of 64 or more heavy -- the
# repeat blocks and reads below -- and no chunk that could be sparse.
# MM2GB_SPARSE_MIN_ANCHORS=0: the list is for large micro-batches by default (250 M anchors); here every batch gets it.
LIST_ON = {"MM2GB_SPARSE_MIN_ANCHORS": "0"}
TEAM_ENVS = {k: dict(v, MM2GB_LONG_MIN_WINDOW="80", **LIST_ON) for k, v in TEAMS.items() if k != "wave"}
SPARSE_PARAMS = {"default": PARAMS["default"], "small_bw": PARAMS["small_bw"]}


def stretch(n, runs=(), equal_x=(), rid=5, rev=0, r0=1000, seed=0):
    """n anchors of one read, isolated (GAP apart, query positions at random) except for `runs`: (position, length[, dx[, dy]]) makes the
    `length` anchors from `position` on follow their predecessor at dx bases on the reference and dy on the query (20 and 20: a chain
    whose last anchor has a window of `length`; 2000: windows of 2 however long the run).  Positions in `equal_x` repeat their
    predecessor's reference position, 20 further on the query."""
    rng = np.random.default_rng(seed)
    dx = np.full(n, GAP, np.int64)
    y = rng.integers(1000, 50_000, n)
    follow = {}
    for pos, length, *d in runs:
        for k in range(pos, pos + length):
            follow[k] = (d[0] if len(d) > 0 else 20, d[1] if len(d) > 1 else 20)
    for pos in equal_x:
        follow[pos] = (0, 20)
    for k in sorted(follow):
        dx[k] = follow[k][0]
        y[k] = y[k - 1] + follow[k][1]
    return sc.pack(np.full(n, rid), np.full(n, rev), r0 + np.cumsum(dx), y)


def window_starts(a, off, prm):
    """lchain.c:172-173 per read, as k_window computes it: (st, clamped) per anchor."""
    x = a[:, 0].astype(np.uint64)
    n = len(x)
    st = np.zeros(n, np.int64)
    clamped = np.zeros(n, bool)
    for r in range(len(off) - 1):
        lo, hi = int(off[r]), int(off[r + 1])
        xs = x[lo:hi]
        head = xs & np.uint64(0xffffffff00000000)
        lim = np.maximum(head, np.where(xs - head > np.uint64(prm.max_dist_x), xs - np.uint64(prm.max_dist_x), head))
        first = lo + np.searchsorted(xs, lim, side="left")
        i = np.arange(lo, hi)
        lb = np.maximum(lo, i - prm.max_iter)
        st[lo:hi] = np.maximum(first, lb)
        clamped[lo:hi] = (lb == i - prm.max_iter) & (lb > lo) & (first < lb)
    return st, clamped


def heavy_rule(env):
    """(least cost, least mean window + 16) of a heavy chunk as an engine made under `env` has them (Engine::init)"""
    c = mm.default_config()
    cost = max(1, c.score_kernel.mid_seg_cutoff) * max(64, c.range_kernel.blockdim) * 1024
    return int(env.get("MM2GB_LONG_MIN_COST", cost)), int(env.get("MM2GB_LONG_MIN_WINDOW", 128))


def expected_sparse(a, off, prm, max_window=SPARSE_W, heavy=(1, 80)):
    """Chunks the planner sends to the sparse list (plan_finish): a chunk starts at the first anchor of a planning block whose window is
    empty; it is sparse if it is not heavy, no block from its own to the next chunk's holds a clamped window (the rescue build's flag)
    and its widest window is at most max_window.  The planner takes a chunk's pairs by whole blocks, from its first block to the next
    chunk's: a short chunk that starts in the last block of a dense one looks heavy to it."""
    st, clamped = window_starts(a, off, prm)
    n = len(st)
    i = np.arange(n)
    nb = (n + BLOCK - 1) // BLOCK
    cuts = [(k, int(c[0]) + k * BLOCK) for k in range(nb) for c in [np.flatnonzero(st[k * BLOCK:(k + 1) * BLOCK] == i[k * BLOCK:(k + 1) * BLOCK])] if c.size]
    blk_clamped = [bool(clamped[k * BLOCK:(k + 1) * BLOCK].any()) for k in range(nb)]
    blk_pairs = [int((i[k * BLOCK:(k + 1) * BLOCK] - st[k * BLOCK:(k + 1) * BLOCK]).sum()) for k in range(nb)]
    count = 0
    if max_window <= 0:
        return 0
    for c, (blk, start) in enumerate(cuts):
        last = c + 1 == len(cuts)
        end = n if last else cuts[c + 1][1]
        blk_to = nb - 1 if last else cuts[c + 1][0]
        track = any(blk_clamped[blk:blk_to + 1])
        cost = sum(blk_pairs[blk:nb if last else blk_to]) + 16 * (end - start)
        is_heavy = cost >= heavy[0] and (end - start) * heavy[1] <= cost
        count += (not is_heavy) and (not track) and int((i[start:end] - st[start:end]).max()) <= max_window
    return count


def pad_to_block(parts, seed):
    """a noise read that brings the batch to a multiple of the planning block, so that the next part's tiles are where the test wants them"""
    n = sum(len(p) for p in parts)
    fill = (-n) % BLOCK
    return parts + ([sc.noise(fill, seed)] if fill else [])


def shaped_stretches(tail_len):
    """Reads whose sparse chunks have the shapes sparse_chunk can go wrong at.  The first begins on a planning block: its chunks' tiles
    are the 64-anchor groups of the read."""
    runs = [(62, 3),        # windows 1..3 across lanes 63 -> 64: the second tile reaches into its predecessor, which is the first tile of the same pair
            (126, 3),       # across 127 -> 128: the predecessor tile belongs to the previous pair
            (191, 2), (200, 1), (300, 3), (320, 40, 2000, 2000), (380, 30, 2000),
            (500, SPARSE_W),                          # a window of exactly the bound, across tiles
            (BLOCK + 300, 10),                        # (a chunk whose widest window is 10)
            # no cut at the next block's start: the chunk runs 1, 63, 64, 65, 128 and 129 anchors past the block boundary (windows of 1 and 2),
            # chains across its last, partly filled tile included
            (2 * BLOCK - 1, 1 + 1, 2000), (3 * BLOCK - 1, 1 + 63, 2000, 2000), (4 * BLOCK - 1, 1 + 64, 2000), (4 * BLOCK + 61, 3),
            (5 * BLOCK - 1, 1 + 65, 2000, 2000), (6 * BLOCK - 1, 1 + 128, 2000), (6 * BLOCK + 126, 2), (7 * BLOCK - 1, 1 + 129, 2000, 2000)]
    a = stretch(8 * BLOCK, runs=runs, equal_x=(10, 63, 64, 700, 701, 4 * BLOCK + 70), seed=3)
    wide = stretch(2 * BLOCK, runs=[(100, SPARSE_W + 1)], rid=6, seed=4)                      # one window of bound + 1
    short = [stretch(40 + 7 * k, runs=[(5, 2), (20 + k, 3)], rid=k % 4, rev=k & 1, seed=10 + k) for k in range(30)]   # several reads per chunk
    empty = stretch(3 * BLOCK + tail_len, rid=9, seed=5)                                      # all windows empty; the batch's last chunk has tail_len anchors
    return [a, wide] + short, empty


def sparse_batch(n_heavy, seed, tail_len=65, noise_blocks=4):
    heavy = [sc.sort_by_x(sc.repeat_block(5000 + 1500 * k, seed + k)) if k != 1 else sc.read_like(12000, seed + k) for k in range(n_heavy)]
    shaped, empty = shaped_stretches(tail_len)
    parts = pad_to_block([sc.noise(noise_blocks * BLOCK, seed + 20)] + heavy[:1], seed + 21) + shaped
    parts = pad_to_block(parts + heavy[1:], seed + 22) + [sc.noise((noise_blocks + 1) * BLOCK, seed + 23)]
    return batch(pad_to_block(parts, seed + 24) + [empty])


def engine_of(monkeypatch, env, one_workgroup=False):
    """An engine under `env`.  one_workgroup: its score kernel runs as ONE workgroup, whose waves come to the sparse list one team after
    the other; at the full grid of a small batch the teams that find no heavy chunk have scored it before the first heavy chunk is done."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = mm.default_config()
    if one_workgroup:
        c.score_kernel.short_griddim = 4
    return mm.Engine(config=c)


def check_sparse(e, a, off, prm, env, max_window=SPARSE_W, mode=0):
    """the batch against the oracle, the build that scored it (0: the table build, whose sparse chunks go through sparse_chunk), and the
    list's length"""
    check_batch(e, a, off, prm)
    assert e.last_score_mode() == mode
    got, want = e.sparse_chunks(), expected_sparse(a, off, prm, max_window, heavy_rule(env))
    assert got == want, f"sparse chunks scored: {got}, the planner's rule gives {want}"
    return want


@pytest.fixture(scope="module")
def batches():
    return {n: sparse_batch(n, 100 * n, tail_len=t) for n, t in ((1, 1), (2, 63), (3, 129))}


@pytest.mark.parametrize("team", list(TEAM_ENVS))
@pytest.mark.parametrize("one_workgroup", [True, False], ids=["one-workgroup", "full-grid"])
def test_sparse_chunks_beside_teams(monkeypatch, batches, team, one_workgroup):
    env = TEAM_ENVS[team]
    with engine_of(monkeypatch, env, one_workgroup) as e:
        for n, (a, off) in batches.items():
            for kw in SPARSE_PARAMS.values():
                assert check_sparse(e, a, off, orc.default_param(**kw), env) > 20


NO_GANGS = dict(LIST_ON, MM2GB_GANG_MAX="0")


@pytest.mark.parametrize("tail_len", [1, 63, 64, 65, 128, 129])
def test_the_default_planner_thresholds(monkeypatch, tail_len):
    """heavy chunks as the planner finds them without any knob (big teams, 4-wave teams); the batch's last chunk is tail_len anchors long"""
    a, off = sparse_batch(2, 7, tail_len=tail_len)
    with engine_of(monkeypatch, NO_GANGS) as e:
        for kw in SPARSE_PARAMS.values():
            assert check_sparse(e, a, off, orc.default_param(**kw), NO_GANGS) > 20


def test_a_launch_with_gangs_makes_no_list(monkeypatch):
    """a small batch gets the gang kernel, whose last phase knows the wave list only"""
    a, off = sparse_batch(2, 7)
    with engine_of(monkeypatch, LIST_ON) as e:
        for kw in SPARSE_PARAMS.values():
            check_batch(e, a, off, orc.default_param(**kw))
            assert e.sparse_chunks() == 0


def test_small_batches_get_no_list_by_default(monkeypatch):
    a, off = sparse_batch(2, 7)
    monkeypatch.delenv("MM2GB_SPARSE_MIN_ANCHORS", raising=False)
    with mm.Engine() as e:
        check_batch(e, a, off, orc.default_param())
        assert e.sparse_chunks() == 0
    with engine_of(monkeypatch, {"MM2GB_SPARSE_MIN_ANCHORS": str(len(a)), "MM2GB_GANG_MAX": "0"}) as e:
        assert check_sparse(e, a, off, orc.default_param(), {}) > 20
    with engine_of(monkeypatch, {"MM2GB_SPARSE_MIN_ANCHORS": str(len(a) + 1), "MM2GB_GANG_MAX": "0"}) as e:
        check_batch(e, a, off, orc.default_param())
        assert e.sparse_chunks() == 0


def test_the_bound_of_the_list(monkeypatch, batches):
    a, off = batches[2]
    prm = orc.default_param()
    counts = {}
    for w in ("63", "62", "3", "0", "1000"):
        env = dict(TEAM_ENVS["teams-of-4"], MM2GB_SPARSE_MAX_WINDOW=w)
        with engine_of(monkeypatch, env, one_workgroup=True) as e:
            counts[w] = check_sparse(e, a, off, prm, env, max_window=min(int(w), SPARSE_W))
    # the chunk with a window of exactly 63 is on the list at 63 and not at 62; at 0 there is no list; the bound never exceeds 63
    assert counts["1000"] == counts["63"] == counts["62"] + 1 and counts["62"] > counts["3"] > counts["0"] == 0
    shaped, _ = shaped_stretches(1)
    a1, off1 = batch([shaped[1]])                     # the read with one window of 64: its first chunk is not sparse at 63
    assert expected_sparse(a1, off1, prm) == 1 and expected_sparse(a1, off1, prm, 64) == 2
    env = dict(TEAM_ENVS["teams-of-4"], MM2GB_SPARSE_MAX_WINDOW="63")
    with engine_of(monkeypatch, env) as e:
        assert check_sparse(e, a1, off1, prm, env) == 1


def test_only_sparse_chunks(monkeypatch):
    shaped, empty = shaped_stretches(64)
    a, off = batch([sc.noise(6 * BLOCK, 1)] + shaped[:1] + shaped[2:] + [empty])
    env = TEAM_ENVS["teams-of-4"]
    for one in (True, False):
        with engine_of(monkeypatch, env, one) as e:
            for kw in SPARSE_PARAMS.values():
                assert check_sparse(e, a, off, orc.default_param(**kw), env) > 10


def test_only_heavy_chunks(monkeypatch):
    a, off = batch([sc.sort_by_x(sc.repeat_block(6000, 11)), sc.sort_by_x(sc.repeat_block(8000, 12)), sc.sort_by_x(sc.repeat_block(5000, 13))])
    env = TEAM_ENVS["teams-of-4"]
    for one in (True, False):
        with engine_of(monkeypatch, env, one) as e:
            check_batch(e, a, off, orc.default_param())
            assert e.sparse_chunks() == 0 and expected_sparse(a, off, orc.default_param()) == 0


@pytest.mark.parametrize("one_workgroup", [True, False], ids=["one-workgroup", "full-grid"])
@pytest.mark.parametrize("noise_blocks", [300, 1], ids=["many", "few"])
def test_many_and_few_sparse_chunks(monkeypatch, noise_blocks, one_workgroup):
    """far more sparse chunks than there are waves, and fewer than one claim holds: the list runs out while other waves are still claiming"""
    if noise_blocks > 1:
        a, off = sparse_batch(3, 31, noise_blocks=noise_blocks)
    else:
        a, off = batch(pad_to_block([sc.sort_by_x(sc.repeat_block(5000 + 1000 * k, 40 + k)) for k in range(3)], 44) + [sc.noise(3 * BLOCK, 45)])
    env = TEAM_ENVS["teams-of-4"]
    with engine_of(monkeypatch, env, one_workgroup) as e:
        want = check_sparse(e, a, off, orc.default_param(), env)
        assert want > 600 if noise_blocks > 1 else 0 < want < 8


def test_per_pair_builds_keep_the_four_lists(monkeypatch, batches):
    """MODE_FAST (no table at bw 5119) and MODE_GENERAL (a segment id): the planner makes the list, phase 2 scores it with run_chunk"""
    a, off = batches[2]
    env = TEAM_ENVS["teams-of-4"]
    with engine_of(monkeypatch, env, one_workgroup=True) as e:
        check_sparse(e, a, off, orc.default_param(bw=5119), env, mode=1)
        seg = a.copy()
        seg[[5, 4 * BLOCK + 70, len(a) - 3], 1] |= np.uint64(1) << np.uint64(48)
        check_sparse(e, seg, off, orc.default_param(), env, mode=2)


def test_twice_on_one_engine(monkeypatch, batches):
    """cursors and counters are reset per launch"""
    a, off = batches[3]
    prm = orc.default_param()
    env = TEAM_ENVS["teams-of-8"]
    with engine_of(monkeypatch, env, one_workgroup=True) as e:
        e.set_misc(misc_from(prm))
        f1, p1, st1 = e.score(a, off)
        f1, p1, c1 = f1.copy(), p1.copy(), e.sparse_chunks()
        f2, p2, st2 = e.score(a, off)
        c2 = e.sparse_chunks()
    assert np.array_equal(f1, f2) and np.array_equal(p1, p2) and st1["n_pairs"] == st2["n_pairs"]
    assert c1 == c2 == expected_sparse(a, off, prm, heavy=heavy_rule(env)) > 0
