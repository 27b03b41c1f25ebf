"""The per-read kernels on batches larger than their grids (tests/scale_cases.py; DESIGN: "Batches beyond one pass of a capped grid").  With W = 32 x the engine's
compute units and N = max(2 W, 16384) + 37 tiny reads, every kernel that gives a read to a wave and lets the wave stride on runs a full second pass and a short third
on data that is then compared, exactly: the seed collection in sorted and in heap order against the oracle, the host form and the plain-Python heap; the seed sort and
mm_gen_regs on crafted anchors and chains against the oracle; the match selection against the host form with more than 8192 thinned streaks; the short-read and the
long-read mapper on the short-read fixture's 209 reads c times over against the reference program's text c times over.  The kernel-level tests also run the batch's
first W reads (the grid exactly full) and first W + 1 (one wave with a second read).  A failure names the read relative to W."""
import numpy as np
import pytest

import scale_cases as sx
import sr_cases as sc
from test_gpu_resident import traced
from test_gpu_seeding import same_matches

pytestmark = pytest.mark.gpu

mm = pytest.importorskip("mm2gb_amd")


@pytest.fixture(scope="module")
def engine():
    with mm.Engine() as e:
        yield e


@pytest.fixture(scope="module")
def dims(engine):
    cu = engine.cu_count()
    assert cu >= 1
    w, n = sx.sizes(cu)
    assert n > 2 * w and n > sx.REP_LEN_GRID and w + 1 < n
    print(f"{cu} compute units: W = {w}, N = {n}, the mappers' batches hold {sx.copies(n)} copies of the 209 reads")
    return w, n


def three_sizes(dims):
    w, n = dims
    return (n, w, w + 1)


# ---------------------------------------------------------------- 1. k_seed_compact, k_seed_offsets, k_seed_pack, k_sort_x behind Engine.collect_seeds
@pytest.fixture(scope="module")
def seed_data(dims):
    b = sx.seed_batch(*dims)
    b["want"] = {}
    return b


def seed_want(b, name):
    if name not in b["want"]:
        b["want"][name] = sx.seed_want(b, sx.SEED_FLAGS[name])
    return b["want"][name]


@pytest.mark.parametrize("name", list(sx.SEED_FLAGS))
def test_collect_seeds_beyond_the_grid(engine, dims, seed_data, name):
    """Reads of 0-6 seeds with 0-5 hits; 65 hits and 40 hits of one x at W - 1, W, 2 W - 1, 2 W and N - 1; an empty read and one that loses every hit at 0, W + 1,
    N - 2.  Every read's anchors and anchor_off (k_seed_offsets' carry through ceil(N / 1024) rounds) equal the oracle's."""
    w, n = dims
    b, want = seed_data, seed_want(seed_data, name)
    flag = sx.SEED_FLAGS[name]
    hard, blank, dropped = sx.special(w, n)
    kept = np.asarray([len(a) for a in want])
    n_hits = np.asarray([len(rd["hits"]) for rd in b["reads"]])
    assert (kept[blank] == 0).all() and (n_hits[dropped] > 0).all() and (n_hits[hard] >= 40).all()
    # a read's length differs from that of the read W before it (the wave's previous read): a length read at the wrong index shows
    qlen = np.asarray([rd["qlen"] for rd in b["reads"]])
    assert [int(qlen[r]) for r in hard] == [3_000, 5_000, 4_000, 9_000, 3_000] and all(qlen[r] != qlen[r - w] for r in hard if r >= w)
    assert np.bincount(np.searchsorted(sx.SEED_QLENS, qlen)).min() > n // 8 and (qlen[w:] != qlen[:n - w]).mean() > 0.6
    if flag:
        assert (kept[b["lost"]] == 0).all() and (kept[dropped] == 0).all() and ((kept == 0) & (n_hits > 0)).sum() >= n // 5
    else:
        assert (kept == n_hits).all() and [int(kept[r]) for r in hard] == [65, 40, 65, 40, 65]
    for m in three_sizes(dims):
        a_off, out = sx.collect_seeds_raw(engine, flag, b["reads"][:m], b["ref_len"], b["ref_rank"])
        want_off, rows = sx.lay(want[:m])
        bad = sx.first_difference(a_off, out, want_off, rows, w, f"{name}, {m} reads")
        assert bad is None, bad


# ---------------------------------------------------------------- 2. k_heap_sort_wave, rocPRIM's segmented sort and scan, k_heap_emit, k_heap_pack
@pytest.fixture(scope="module")
def heap_data(dims):
    b = sx.heap_batch(*dims)
    b["host"], b["literal"] = {}, {}
    return b


def heap_host(b, name):
    if name not in b["host"]:
        b["host"][name] = mm.collect_seeds_heap_host(sx.HEAP_FLAGS[name], b["reads"])
        b["literal"][name] = [sc.heap_literal(rd, sx.HEAP_FLAGS[name]) for rd in b["reads"]]
    return b["host"][name]


@pytest.mark.parametrize("name", list(sx.HEAP_FLAGS))
def test_collect_seeds_heap_beyond_the_grid(engine, dims, heap_data, name):
    """The same small reads with ascending lists, about 200 reads of 1025-1400 hits between them (as many segments for the library's sort), wave_exact, wave_plus_1 and
    odd_65 at the special indices: every read equals the host form and the plain-Python heap.  Between 1 % and 10 % of the reads are tied (done again by the host
    form, so their device order is not what is compared); none of the special reads is."""
    w, n = dims
    b = heap_data
    flag = sx.HEAP_FLAGS[name]
    host, host_tied = heap_host(b, name)
    hard, blank, dropped = sx.special(w, n)
    assert host_tied == int(b["tied"].sum()) and n // 100 <= host_tied <= n // 10 and not b["tied"][hard + blank + dropped].any()
    assert len(b["long"]) >= 190 and int(b["tied"][b["long"]].sum()) == sx.N_LONG_TIED
    assert [len(b["reads"][r]["hits"]) for r in hard] == [sc.WAVE_HITS, sc.WAVE_HITS + 1, 65, 65, sc.WAVE_HITS + 1]
    assert all(len(host[r]) == 0 for r in blank) and all(len(b["reads"][r]["hits"]) > 0 for r in dropped)
    if flag:
        assert all(len(host[r]) == 0 for r in dropped)
    want_off, rows = sx.lay(host)
    lit_off, lit = sx.lay(b["literal"][name])
    bad = sx.first_difference(want_off, rows, lit_off, lit, w, f"{name}: the host form against the plain-Python heap")
    assert bad is None, bad
    for m in three_sizes(dims):
        got, n_tied = engine.collect_seeds_heap(flag, b["reads"][:m])
        got_off, got_rows = sx.lay(got)
        want_off, rows = sx.lay(host[:m])
        bad = sx.first_difference(got_off, got_rows, want_off, rows, w, f"{name}, {m} reads")
        assert bad is None, bad
        assert n_tied == int(b["tied"][:m].sum())


# ---------------------------------------------------------------- 3. k_sort_x and k_gen_regs on crafted input
@pytest.fixture(scope="module")
def sort_data(dims):
    a, off = sx.sort_batch(*dims)
    return a, off, sx.sort_want(a, off)


def test_sort_seeds_beyond_the_grid(engine, dims, sort_data):
    """Reads of 0-40 anchors on a dozen positions; 65, 5000, 40 of one x, 64 and 65 anchors at the special indices: radix_sort_128x's order, equal x included."""
    w, n = dims
    a, off, want = sort_data
    hard, blank, _ = sx.special(w, n)
    cnt = np.diff(off)
    assert [int(cnt[r]) for r in hard] == [65, 5_000, 40, 64, 65] and (cnt[blank] == 0).all()
    x = a[off[hard[2]]:off[hard[2] + 1], 0]
    assert (x == x[0]).all()
    for m in three_sizes(dims):
        got = engine.sort_seeds(a[:off[m]], off[:m + 1])                                    # (sorted in place: the rows in are the rows out)
        assert got.shape == (off[m], 2)
        bad = sx.first_difference(off[:m + 1], got, off[:m + 1], want[:off[m]], w, f"{m} reads")
        assert bad is None, bad


@pytest.fixture(scope="module")
def chain_data(dims):
    b = sx.chain_batch(*dims)
    b["want"] = {q: sx.regs_want(b, q) for q in (0, 1)}
    return b


@pytest.mark.parametrize("is_qstrand", [0, 1])
def test_gen_regs_beyond_the_grid(engine, dims, chain_data, is_qstrand):
    """Chains handed over as they are: 0-5 a read, 65 and 64 and five of one score at the special indices, spans of 5-28 mixed inside a chain with steps above and below
    them, chains that begin in the reference's first bases, both strands, scores of 40-42: every record equals the oracle's mm_gen_regs."""
    w, n = dims
    b, want = chain_data, chain_data["want"][is_qstrand]
    hard, blank, _ = sx.special(w, n)
    n_ch = np.diff(b["u_off"])
    assert [int(n_ch[r]) for r in hard] == [65, 64, 5, 64, 65] and (n_ch[blank] == 0).all()
    inner = (b["dx"] > 0)
    both = inner & (b["dx"] > b["span"]) & (b["dy"] > b["span"])
    assert both.sum() > 1_000 and (inner & ~both).sum() > 1_000                                   # either branch of the matching length
    assert (want["rs"] == 0).sum() > 100 and (want["flags"] & (1 << 10) != 0).sum() > 1_000 and (want["flags"] == 0).sum() > 1_000
    score = (b["u"] >> np.uint64(32)).astype(np.int64)
    assert len(np.unique(score[b["u_off"][hard[2]]:b["u_off"][hard[2] + 1]])) == 1
    for m in three_sizes(dims):
        regs = engine.gen_regs(b["chains"][:m], b["qlen"][:m], b["hashes"][:m], is_qstrand)
        assert len(regs) == m
        got_off, got = sx.lay(regs, shape=(0,), dt=mm.REG_DTYPE)
        bad = sx.first_difference(got_off, got, b["u_off"][:m + 1], want[:b["u_off"][m]], w, f"is_qstrand {is_qstrand}, {m} reads")
        assert bad is None, bad


# ---------------------------------------------------------------- 4. the match selection: k_m_select, k_m_rep_len, the library's scans and segmented sort
@pytest.fixture(scope="module")
def match_data(dims):
    reads = sx.match_reads(*dims)
    return dict(reads=reads, streaks=sx.thinned_streaks(sx.host_matches(reads, mid_occ=1 << 30, q_occ_frac=0.0), 2, 50))


@pytest.mark.parametrize("name", list(sx.MATCH_OPTS))
def test_collect_matches_beyond_the_grids(engine, dims, match_data, name):
    """N reads of 80-150 bases, two thirds from the tandem array: more than 8192 streaks are thinned (k_m_select takes a second step) and reads beyond index 16384
    have dropped minimizers (k_m_rep_len's second step is compared); with q_occ_frac > 0 the library sorts N segments.  Every read equals the host form."""
    w, n = dims
    reads, kw = match_data["reads"], sx.MATCH_OPTS[name]
    want = sx.host_matches(reads, **kw)
    print(f"{match_data['streaks']} thinned streaks (one step of k_m_select: {sx.SELECT_GRID})")
    assert match_data["streaks"] >= 9_000 > sx.SELECT_GRID
    rep = np.asarray([m["rep_len"] for m in want])
    assert (rep[sx.REP_LEN_GRID:] > 0).sum() >= 10 and (rep[:sx.REP_LEN_GRID] > 0).sum() >= 9_000
    _, blank, dropped = sx.special(w, n)
    assert all(len(want[r]["seeds"]) == 0 for r in blank + dropped) and sorted(len(reads[r]) for r in blank) == [0, 15, 120]
    for m in three_sizes(dims) if name == "q0" else (n,):
        same_matches(engine.collect_matches(sc.index(), reads[:m], **kw), want[:m], f"{name}, {m} reads, W = {w}:")


# ---------------------------------------------------------------- 5. the short-read mapper on the fixture's reads c times over
SR_FORMS = {
    "sr-seed_host": ("sr", dict(seeding_on_device=0)),
    "sr-seed_device": ("sr", dict(seeding_on_device=1)),
    "sr.f4_50-seed_device": ("sr.f4_50", dict(seeding_on_device=1)),
    "sr.c-align_device": ("sr.c", dict(seeding_on_device=1, align_on_device=1, text_on_device=1)),
    "sr.c-align_host": ("sr.c", dict(seeding_on_device=1, align_on_device=-1, text_on_device=-1)),
}


@pytest.mark.parametrize("form", list(SR_FORMS))
def test_short_read_mapper_beyond_the_grid(engine, dims, form):
    """One read's lines do not depend on its batch: the 209 reads c = ceil(N / 209) times over print the recorded text c times over; the counts are c times one copy's."""
    w, n = dims
    run, kw = SR_FORMS[form]
    c = sx.copies(n)
    _, one = sx.map_sr(engine, run, sc.reads(), **kw)
    text, st = sx.map_sr(engine, run, sc.reads() * c, **kw)
    bad = sx.paf_difference(text, sc.golden_paf(run), c, w, f"{form}, {c} copies")
    assert bad is None, bad
    assert st["n_reads"] == 209 * c and st["n_mapped"] == one["n_mapped"] * c
    assert st["sr_counts"] == {k: v * c for k, v in one["sr_counts"].items()} and st["n_rescued"] == one["n_rescued"] * c
    if run in ("sr", "sr.c"):
        assert st["n_tied_reads"] == 9 * c
    if run == "sr.c":
        assert st["sr_counts"]["fill_ungapped"] >= 200 * c


# ---------------------------------------------------------------- 6. the long-read mapper on the same reads
LONG_FORMS = {"host_seeding": dict(seeds_on_device=-1), "seeds_on_device": dict(seeds_on_device=1), "seeding_on_device": dict(seeding_on_device=1)}


@pytest.mark.parametrize("form", list(LONG_FORMS))
@pytest.mark.parametrize("run", ["ont", "pb"])
def test_long_read_mapper_beyond_the_grid(engine, dims, run, form):
    """The defaults (k = 15, w = 10) and map-pb (k = 19, w = 10, compressed) with the long join on: k_seed_*, k_sort_x and k_gen_regs inside the mapper at N reads, seeded
    on host threads with the anchors made on the host and on the device, and seeded on the device."""
    w, n = dims
    c = sx.copies(n)
    text, st = sx.map_long(engine, run, sc.reads() * c, **LONG_FORMS[form])
    bad = sx.paf_difference(text, sx.long_paf(run), c, w, f"{run} {form}, {c} copies")
    assert bad is None, bad
    assert st["n_reads"] == 209 * c and st["n_mapped"] == len({ln.split("\t")[0] for ln in sx.long_paf(run).splitlines()}) * c


@pytest.mark.parametrize("run", ["ont.nolj", "pb.nolj"])
def test_resident_mapper_beyond_the_grid(engine, dims, capfd, monkeypatch, run):
    """--no-long-join with seeding_on_device = 2: the batch stays on the resident path (its anchors are far below one chaining micro-batch)."""
    w, n = dims
    c = sx.copies(n)
    (text, st), lines = traced(capfd, monkeypatch, lambda: sx.map_long(engine, run, sc.reads() * c, seeding_on_device=mm.SEEDING_RESIDENT))
    assert [ln["path"] for ln in lines] == ["resident"], lines
    bad = sx.paf_difference(text, sx.long_paf(run), c, w, f"{run} resident, {c} copies")
    assert bad is None, bad
    assert st["n_reads"] == 209 * c and lines[0]["anchors"] == st["n_anchors"]


# ---------------------------------------------------------------- 7. arenas: a large batch, a batch of three, the large one again
def test_arenas_after_a_small_batch(engine, dims, heap_data, seed_data):
    w, n = dims
    few = [n - 1, 0, w]
    first, t1 = engine.collect_seeds_heap(0, heap_data["reads"])
    small, _ = engine.collect_seeds_heap(0, [heap_data["reads"][r] for r in few])
    again, t2 = engine.collect_seeds_heap(0, heap_data["reads"])
    host, host_tied = heap_host(heap_data, "none")
    assert t1 == t2 == host_tied
    for what, got in (("first", first), ("again", again)):
        bad = sx.first_difference(*sx.lay(got), *sx.lay(host), w, f"heap order, {what}")
        assert bad is None, bad
    assert all(np.array_equal(small[k], host[r]) for k, r in enumerate(few))
    flag, b = sx.SEED_FLAGS["no_diag_no_dual"], seed_data
    want = seed_want(b, "no_diag_no_dual")
    first = sx.collect_seeds_raw(engine, flag, b["reads"], b["ref_len"], b["ref_rank"])
    small = engine.collect_seeds(flag, [b["reads"][r] for r in few], ref_len=b["ref_len"], ref_rank=b["ref_rank"])
    again = sx.collect_seeds_raw(engine, flag, b["reads"], b["ref_len"], b["ref_rank"])
    for what, got in (("first", first), ("again", again)):
        bad = sx.first_difference(*got, *sx.lay(want), w, f"sorted order, {what}")
        assert bad is None, bad
    assert all(np.array_equal(small[k], want[r]) for k, r in enumerate(few))
