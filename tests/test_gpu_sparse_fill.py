"""The planner's sparse list and its lean scorer (chain_kernels.hip: plan_finish, sparse_chunk, sparse_take): stretches of isolated
anchors -- no window wider than MM2GB_SPARSE_MAX_WINDOW -- are scored by a function of their own in the score kernel's last phase,
claimed eight at a time.  Every anchor's f / p against the oracle; Engine.sparse_chunks() says that the path under test ran: it is
the length of the list, which a numpy model of the planner's rule (expected_sparse) gives independently of the device."""
import numpy as np
import pytest

import orc
import synth_cases as sc
from test_gpu_band import PARAMS, TEAMS, batch
from test_gpu_parity import check_batch, misc_from, rel

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
SPARSE_PARAMS = {k: PARAMS[k] for k in ("default", "small_bw", "max_iter", "dist_y")}
# The large-batch form: what a batch of 250 M anchors and more gets from Engine::enqueue at the default planner thresholds -- the list, the
# 4-wave share rule, no gangs -- at any size.
LARGE = {"MM2GB_SPARSE_MIN_ANCHORS": "0", "MM2GB_TEAM4_MIN_ANCHORS": "0", "MM2GB_GANG_MAX_ANCHORS": "0"}


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
    dist_x = np.uint64(max(prm.max_dist_x, prm.bw))                  # lchain.c:160
    for r in range(len(off) - 1):
        lo, hi = int(off[r]), int(off[r + 1])
        xs = x[lo:hi]
        head = xs & np.uint64(0xffffffff00000000)
        lim = np.maximum(head, np.where(xs - head > dist_x, xs - dist_x, head))
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


def expected_sparse(a, off, prm, max_window=SPARSE_W, heavy=(1, 80), own_block_only=False):
    """Chunks the planner sends to the sparse list (plan_finish): a chunk starts at the first anchor of a planning block whose window is
    empty; it is sparse if it is not heavy, no block from its own to the next chunk's holds a clamped window (the rescue build's flag)
    and its widest window is at most max_window.  The planner takes a chunk's pairs by whole blocks, from its first block to the next
    chunk's: a short chunk that starts in the last block of a dense one looks heavy to it.
    own_block_only: NOT the planner's rule -- clamps counted in the chunk's first block alone, which misses the windows of a chunk's end
    in the next chunk's block; a case in which the two counts agree does not test the inclusive count."""
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
        track = any(blk_clamped[blk:blk + 1 if own_block_only else blk_to + 1])
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


# ---- clamped windows beside sparse chunks ------------------------------------------------------------------------------------------
# sparse_chunk is the plain build: it has no max_ii rescue (lchain.c:190-201).  plan_finish keeps a chunk off the list when a planning
# block from the chunk's own to the next chunk's holds a window clamped by max_iter.  At max_iter <= 63 a clamped window is no wider than
# the list's bound: there only that flag stands between sparse_chunk and a read that needs the rescue.

CLAMP_CASES = [(1, 8), (7, 20), (20, 40), (62, 70), (63, 64), (64, 70)]      # (max_iter, n_noise); every batch also runs at max_iter 5000
N_CHAIN = 27                                                                 # anchors of a rescue read's chain, and of its continuation
RUN_E = 40                                                                   # part (e): the last anchor's window


def isolated(n, rid, seed, singles=()):
    """a stretch in which no window holds more than one anchor (at `singles`): nothing in it is clamped at any max_iter"""
    return stretch(n, runs=[(k, 1) for k in singles], rid=rid, seed=seed)


def clamp_batch(n_noise, seed=50):
    """Twelve planning blocks and a tail; (anchors, offsets, indices of the rescue reads).  A rescue read is sc.rescue_case scaled down: a
    chain of N_CHAIN anchors, n_noise anchors packed behind its end, the chain's continuation -- at max_iter < n_noise the continuation's
    first anchor reaches the chain's end through max_ii alone.  Isolated anchors each start a window of their own, so every block has a
    cut at or near its start and a chunk is about one block.
      blocks 0-2   (d) isolated anchors: no clamp in any block these chunks are judged by (their own and the next)
      block 3      (c) isolated anchors, 300 more of the stretch in block 4: the chunk of block 3 holds no clamped window, the block in
                   which its stretch ends does
      block 4      (a) two rescue reads behind the 300, (b) a stretch with short runs between them and isolated anchors behind them
      block 5      (d) isolated anchors: judged by blocks 5 and 6, neither of which holds a clamp
      block 6      isolated anchors and the first TWO anchors of a third rescue read, whose other anchors -- every clamped one, at any
                   max_iter -- lie in block 7 before that block's first cut: the chunk of block 6 ends with the read, and only the count's
                   last, inclusive block knows of its clamps
      block 7      (b) behind the read a stretch with a run, isolated anchors
      block 8      (e) a run at 20 / 20 whose last window holds RUN_E anchors: clamped at max_iter < RUN_E, every link inside its window
      blocks 9-11  (d) isolated anchors and a tail of 65"""
    parts, rescue_reads = [], []

    def add(part, rescue=False):
        if rescue:
            rescue_reads.append(len(parts))
        parts.append(part)

    def fill(rid, sd):
        k = -sum(len(p) for p in parts) % BLOCK
        if k:
            add(isolated(k, rid, sd))

    rescue = lambda k: sc.rescue_case(n_noise=n_noise, seed=seed + k, n_chain=N_CHAIN)
    add(isolated(3 * BLOCK, 5, seed, singles=(100, 1500, 2500)))
    add(isolated(BLOCK + 300, 6, seed + 1, singles=(50, BLOCK + 100)))
    add(rescue(10), True)
    add(stretch(200, runs=[(20, 3), (100, 5), (150, 2, 2000)], rid=7, seed=seed + 2))
    add(rescue(20), True)
    fill(8, seed + 3)
    add(isolated(2 * BLOCK - 2, 9, seed + 4, singles=(700,)))
    add(rescue(30), True)
    add(stretch(150, runs=[(30, 4)], rid=10, seed=seed + 5))
    fill(11, seed + 6)
    add(stretch(BLOCK, runs=[(500, RUN_E)], rid=12, seed=seed + 7))
    add(isolated(3 * BLOCK + 65, 13, seed + 8, singles=(10, 2000)))
    a, off = batch(parts)
    assert len(a) == 12 * BLOCK + 65 and off[rescue_reads[2]] == 7 * BLOCK - 2
    return a, off, rescue_reads


def clamp_conditions(a, off, rescue_reads, max_iter, n_noise, heavy):
    """What makes clamp_batch a test of the planner's flag, from the model alone (no device): the list's length at max_iter and at 5000."""
    prm = orc.default_param(max_iter=max_iter)
    st, clamped = window_starts(a, off, prm)
    width = np.arange(len(a)) - st
    for r in rescue_reads:
        lo, hi = off[r], off[r + 1]
        assert hi - lo == 2 * N_CHAIN + n_noise
        if max_iter <= SPARSE_W:              # only the clamp, not the width, keeps the read off the list
            assert width[lo:hi].max() <= SPARSE_W
        assert clamped[lo:hi].any() == (max_iter < hi - lo - 1)
    assert not clamped[5 * BLOCK:7 * BLOCK].any()                # the third read's clamped windows are all in the block after its first
    want = expected_sparse(a, off, prm, heavy=heavy)
    at_5000 = expected_sparse(a, off, orc.default_param(), heavy=heavy)
    assert 0 < want < at_5000, (want, at_5000)
    # the inclusive count matters: counted by their own block alone, more chunks would be on the list
    # (the chunk of block 3, and that of block 6 while the read at its end is narrow enough for the list)
    assert expected_sparse(a, off, prm, heavy=heavy, own_block_only=True) >= want + (2 if max_iter <= SPARSE_W else 1)
    return want, at_5000


@pytest.fixture(scope="module")
def clamp_batches():
    return {(max_iter, n_noise): clamp_batch(n_noise) for max_iter, n_noise in CLAMP_CASES}


@pytest.mark.parametrize("engine", ["default-thresholds", "teams-of-4"])
def test_clamped_windows_beside_sparse_chunks(monkeypatch, clamp_batches, engine):
    """Reads that need the max_ii rescue at a max_iter below the list's bound, in and next to chunks of isolated anchors: every anchor
    against the oracle, the list's length against the model.  The list must lose the chunks with a clamped window in any block they are
    judged by and keep the others; a planner that drops the flag, or counts clamps short of the next chunk's block, hands the read that
    ends the chunk of block 6 to sparse_chunk, which scores its continuation as a new chain (tried on scratch builds: 81 and 27 anchors
    of the (1, 8) batch differ)."""
    env, one_workgroup = (NO_GANGS, False) if engine == "default-thresholds" else (TEAM_ENVS["teams-of-4"], True)
    monkeypatch.delenv("MM2GB_BAND", raising=False)
    with engine_of(monkeypatch, env, one_workgroup) as e:
        for (max_iter, n_noise), (a, off, rescue_reads) in clamp_batches.items():
            print(f"max_iter {max_iter}, n_noise {n_noise}")
            prm = orc.default_param(max_iter=max_iter)
            want, at_5000 = clamp_conditions(a, off, rescue_reads, max_iter, n_noise, heavy_rule(env))
            _, po, _ = orc.chain_fill_many(a, off, prm, threads=2)
            for r in rescue_reads:            # a link only max_ii can make: without one the read tests nothing
                assert max_iter >= n_noise or rel(po[off[r]:off[r + 1]]).max() > max_iter, f"read {r} needs no rescue"
            assert check_sparse(e, a, off, prm, env) == want
            assert check_sparse(e, a, off, orc.default_param(), env) == at_5000


# ---- the lean scorer's parameters ----------------------------------------------------------------------------------------------------
# sparse_chunk hands bw, dq_lim and the table's bounds to the edge sweep and the in-tile steps.  max_dist_x and max_dist_y are raised to
# bw (lchain.c:160-161), so the rows that are to reject a run's step of 20 come with bw 8 as well as with the default.
LEAN_PARAMS = {"bw-0": dict(bw=0), "bw-1": dict(bw=1), "bw-5118": dict(bw=5118),           # 5118: the last width with a table
               **{f"dist_y-{v}": dict(max_dist_y=v, bw=8) for v in (10, 19, 20, 21)},
               **{f"dist_y-{v}-bw-500": dict(max_dist_y=v) for v in (10, 19, 20, 21)},
               **{f"dist_x-{v}": dict(max_dist_x=v, bw=8) for v in (19, 20, 2000)},
               **{f"dist_x-{v}-bw-500": dict(max_dist_x=v) for v in (19, 20, 2000)}}


def twin(read, bit):
    """the read again, one step of a run further on both axes, on another reference sequence (bit 32) or strand (bit 63)"""
    t = read.copy()
    t[:, 0] = (t[:, 0] ^ (np.uint64(1) << np.uint64(bit))) + np.uint64(20)
    t[:, 1] += np.uint64(20)
    return t


@pytest.fixture(scope="module")
def lean_batches():
    shaped, empty = shaped_stretches(65)
    parts = [sc.noise(BLOCK, 61)] + shaped + [empty]
    a, off = batch(parts)
    # query spans of 9 .. 39 (T.q = tag & 0xff), set as sc.variable_span sets them
    spans = a.copy()
    span = np.random.default_rng(62).integers(9, 40, len(a)).astype(np.uint64)
    spans[:, 1] = (spans[:, 1] & ~(np.uint64(0xff) << np.uint64(32))) | (span << np.uint64(32))
    # adjacent short reads of one chunk on the same reference positions: another rid, another strand, and the very same positions
    twins = list(parts)
    first_short = 3
    assert len(twins[first_short]) == 40 and sum(len(p) for p in twins[:first_short]) % BLOCK == 0
    twins[first_short + 1] = twin(twins[first_short], 32)
    twins[first_short + 3] = twin(twins[first_short + 2], 63)
    same = twins[first_short + 4].copy()
    same[:, 0] ^= np.uint64(1) << np.uint64(32)
    twins[first_short + 5] = same
    assert sum(len(p) for p in twins[first_short:first_short + 6]) < BLOCK
    return {"plain": (a, off), "spans": (spans, off), "twins": batch(twins)}


@pytest.mark.parametrize("one_workgroup", [True, False], ids=["one-workgroup", "full-grid"])
def test_parameters_of_the_lean_scorer(monkeypatch, lean_batches, one_workgroup):
    """band widths 0, 1 and the table's last, distance limits on either side of a run's step, spans other than 15, reads that differ
    in rid or strand alone: the shaped stretches under the table build in the large-batch form"""
    with engine_of(monkeypatch, LARGE, one_workgroup) as e:
        for name, kw in LEAN_PARAMS.items():
            print(name)
            assert check_sparse(e, *lean_batches["plain"], orc.default_param(**kw), LARGE) > 10
        for which in ("spans", "twins"):
            for name in ("default", "small_bw", "dist_y"):
                print(which, name)
                assert check_sparse(e, *lean_batches[which], orc.default_param(**SPARSE_PARAMS[name]), LARGE) > 10


# ---- the skip-limited walk with the list made ---------------------------------------------------------------------------------------

def test_the_skip_walk_scores_both_lists(monkeypatch):
    """With the skip limit kept, the planner still makes the sparse list and k_skip_fill scores it as the end of `order`, behind the
    wave list: no chunk of either may go unscored.  The engine's f / p buffers are its own (two sets, used in turn), so before each
    walk two calls on a chain of the batch's length leave scores in both that no isolated anchor has."""
    import test_gpu_chain_skip as walk
    a, off = sparse_batch(2, 7)
    other = batch([sc.colinear(len(a), 71, indel_p=0.0)])
    with engine_of(monkeypatch, NO_GANGS) as e:
        def the_walk(prm):
            e.set_chain_skip(True)
            for _ in range(2):
                f, p, _ = e.score(*other)
                assert (f[1:] > 15).all() and (p[1:] > 0).all()
            walk.check_against_oracle(e, a, off, prm)
            assert e.last_score_form() == 1 and e.sparse_chunks() == 0          # k_score did not run

        for max_skip in (0, 1, 25):
            print(f"max_skip {max_skip}")
            prm = orc.default_param(max_skip=max_skip, max_iter=5000)
            the_walk(prm)
            e.set_chain_skip(False)
            assert check_sparse(e, a, off, orc.default_param(), NO_GANGS) > 20 and e.last_score_form() == 0
            the_walk(prm)


# ---- batches on either side of MM2GB_SPARSE_MIN_ANCHORS on one engine ------------------------------------------------------------------

def cut(a, off, n):
    """the batch's first n anchors"""
    return a[:n], np.minimum(off, n)


def test_either_side_of_the_floor_on_one_engine(monkeypatch):
    """CNT_NSPARSE and `order` stay in a work set's buffers between launches: a launch without a list behind one with a list must not
    serve the old one, and the reverse.  Small batches take the engine's two work sets in turn, so the issue's five sizes put every launch
    with a list on one set and every launch without on the other; the four that follow change sides on both."""
    a, off = sparse_batch(2, 7)
    n_all = len(a)
    env = {"MM2GB_SPARSE_MIN_ANCHORS": str(n_all), "MM2GB_GANG_MAX": "0"}
    prm = orc.default_param()
    with engine_of(monkeypatch, env) as e:
        for n in (n_all, n_all - 1, n_all, n_all - BLOCK, n_all) + (n_all, n_all - 1, n_all - 1, n_all):
            print(n - n_all)
            part = cut(a, off, n)
            if n >= n_all:
                assert check_sparse(e, *part, prm, env) > 20
            else:
                check_batch(e, *part, prm)
                assert e.sparse_chunks() == 0 and expected_sparse(*part, prm, heavy=heavy_rule(env)) > 20


def slices_of(off, slice_anchors):
    """first reads of the slices mm2gb_chain_gpu cuts a batch into (Engine::chain_gpu_sliced): at read boundaries, a slice once it holds
    slice_anchors, a short last one"""
    n_reads, n, tail = len(off) - 1, int(off[-1]), slice_anchors // 4
    first, acc, tail_cut = [0], 0, False
    for r in range(n_reads - 1):
        acc += int(off[r + 1] - off[r])
        left = n - int(off[r + 1])
        if tail_cut:
            continue
        if left <= tail and acc > tail:
            first.append(r + 1); acc = 0; tail_cut = True
        elif acc >= slice_anchors and left > tail + slice_anchors // 4:
            first.append(r + 1); acc = 0
    return first + [n_reads]


def test_slices_on_either_side_of_the_floor(monkeypatch):
    """mm2gb_chain_gpu on a batch that goes in in slices, all on one work set, with the floor between the slices' sizes: launches with
    and without a list follow each other within one call.  Chains and compacted anchors against the host post-pass of the whole batch."""
    a, off = sparse_batch(2, 7)
    slice_anchors = 6000
    prm = orc.default_param()
    first = slices_of(off, slice_anchors)
    sizes = [int(off[first[k + 1]] - off[first[k]]) for k in range(len(first) - 1)]
    floor = sorted(sizes)[len(sizes) // 2]
    listed = [s >= floor for s in sizes]
    steps = set(zip(listed, listed[1:]))
    assert len(a) > slice_anchors + slice_anchors // 2 and len(sizes) >= 4 and (True, False) in steps and (False, True) in steps, sizes
    env = {"MM2GB_SPARSE_MIN_ANCHORS": str(floor), "MM2GB_GANG_MAX": "0"}
    want = 0
    for k in range(len(sizes)):
        if listed[k]:
            part = a[off[first[k]]:off[first[k + 1]]], off[first[k]:first[k + 1] + 1] - off[first[k]]
            want += expected_sparse(*part, prm, heavy=heavy_rule(env))
    whole = expected_sparse(a, off, prm, heavy=heavy_rule(env))
    assert 0 < want < whole
    monkeypatch.setenv("MM2GB_CHAIN_SLICE_ANCHORS", str(slice_anchors))
    with engine_of(monkeypatch, env) as e:
        assert check_sparse(e, a, off, prm, env) == whole            # (host buffers: one launch)
        host, _ = e.chain(a, off, threads=4)
        for again in range(2):
            dev, st = e.chain_gpu(a, off)
            assert e.sparse_chunks() == want and st["n_anchors"] == len(a)
            assert len(dev) == len(host) == len(off) - 1
            for r in range(len(off) - 1):
                assert np.array_equal(dev[r][0], host[r][0]) and np.array_equal(dev[r][1], host[r][1]), f"chains of read {r} differ"
