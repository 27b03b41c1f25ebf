"""The batches of tests/scale_cases.py without a device, sized for 256 compute units (W = 8192, N = 16421): what each batch is built to hold (the hard reads at the
seams of a wave's passes, the share of reads that lose every hit, the share of tied reads, the number of thinned streaks), the host forms on them against the oracle
and the plain-Python heap, the recorded long-read texts, and -- where the reference is built -- the oracle's mm_gen_regs against the reference's on the crafted chains
and the recording against the reference program.  tests/test_gpu_scale.py runs the same batches on the device."""
import io
import json
import os

import numpy as np
import pytest

import orc
import scale_cases as sx
import sr_cases as sc

mm = pytest.importorskip("mm2gb_amd")
W, N = sx.sizes(sx.CU_CPU)


def test_sizes_and_special_indices():
    assert (W, N) == (8_192, 16_421) and sx.sizes(4) == (128, 16_421) and sx.sizes(304) == (9_728, 19_493)
    assert sx.special(W, N) == ([W - 1, W, 2 * W - 1, 2 * W, N - 1], [0, W + 1, N - 2], [1, W + 2, N - 3])
    assert sx.special(W, W) == ([W - 1], [0, W - 2], [1, W - 3]) and sx.special(W, W + 1) == ([W - 1, W], [0], [1])
    for cu in (1, 4, 256, 304):                                   # a full second pass and a short third, whatever the device
        w, n = sx.sizes(cu)
        assert n == max(2 * w, 16_384) + 37 and n > sx.REP_LEN_GRID and n > 2 * sx.SELECT_GRID
    assert sx.where(W + 5, W) == f"read {W + 5} (= 1 W + 5; W = {W})"


def test_first_difference_names_the_read():
    off = np.asarray([0, 2, 2, 5])
    rows = np.arange(10, dtype=np.uint64).reshape(5, 2)
    assert sx.first_difference(off, rows, off, rows, 2, "x") is None
    other = rows.copy(); other[3, 1] = 0
    assert "read 2 (= 1 W + 0; W = 2)" in sx.first_difference(off, other, off, rows, 2, "x")
    assert "read 1 " in sx.first_difference(np.asarray([0, 2, 3, 5]), rows, off, rows, 2, "x")


def test_paf_difference_names_the_line_and_the_read():
    names = [n for n, _ in sc.reads()]
    one = f"{names[0]}\tp\n{names[5]}\tq\n{names[5]}\tr\n"            # three lines a copy: the set's first read and two of its sixth
    assert sx.paf_difference(one * 3, one, 3, 100, "x") is None
    lines = (one * 3).splitlines()
    lines[5] = f"{names[5]}\tother"                                  # the second copy's third line: read 209 + 5 of the batch
    msg = sx.paf_difference("\n".join(lines) + "\n", one, 3, 100, "x")
    assert "line 5 of 9 (expected 9), read 214 (mod 209: 5, mod W: 14; W = 100)" in msg and f"got  {names[5]}\tother" in msg and f"want {names[5]}\tr" in msg
    msg = sx.paf_difference("\n".join(lines[:5] + lines[6:]) + "\n", one, 3, 100, "x")      # that line missing: the next one stands in its place
    assert "line 5 of 8 (expected 9), read 214 " in msg and f"got  {names[0]}\tp" in msg
    msg = sx.paf_difference(one * 2 + f"{names[0]}\tp\n", one, 3, 100, "x")                   # the text ends early, in the third copy
    assert "line 7 of 7 (expected 9), read 423 (mod 209: 5, mod W: 23; W = 100)" in msg and "got  (none)" in msg


@pytest.fixture(scope="module")
def seed_data():
    return sx.seed_batch(W, N)


@pytest.mark.parametrize("name", list(sx.SEED_FLAGS))
def test_seed_batch_on_the_host_form(seed_data, name):
    b, flag = seed_data, sx.SEED_FLAGS[name]
    want = sx.seed_want(b, flag)
    got = mm.collect_seeds_host(flag, b["reads"], ref_len=b["ref_len"], ref_rank=b["ref_rank"])
    bad = sx.first_difference(*sx.lay(got), *sx.lay(want), W, name)
    assert bad is None, bad
    hard, blank, dropped = sx.special(W, N)
    kept, n_hits = np.asarray([len(a) for a in want]), np.asarray([len(rd["hits"]) for rd in b["reads"]])
    n_seeds = np.asarray([len(rd["seeds"]) for rd in b["reads"]])
    assert np.bincount(n_seeds)[:7].min() > N // 10 and (n_seeds > 6).sum() <= len(hard + dropped) and (n_hits[blank] == 0).all() and (n_hits[dropped] == 7).all()
    if flag:
        assert (kept[b["lost"]] == 0).all() and ((kept == 0) & (n_hits > 0)).sum() >= N // 5 and 0 < kept.sum() < n_hits.sum()
    else:
        assert [int(kept[r]) for r in hard] == [65, 40, 65, 40, 65]
    qlen = np.asarray([rd["qlen"] for rd in b["reads"]])
    assert [int(qlen[r]) for r in hard] == list(sx.HARD_QLENS) and all(qlen[r] != qlen[r - W] for r in hard if r >= W)
    assert np.bincount(np.searchsorted(sx.SEED_QLENS, qlen)).min() > N // 8 and (qlen[W:] != qlen[:N - W]).mean() > 0.6
    if name == "no_diag_no_dual":                                  # the bits do something beside the lost reads: a hit on the diagonal dropped, MM_SEED_SELF set
        rows = np.concatenate(want)
        assert (rows[:, 1] >> np.uint64(43) & np.uint64(1)).sum() > 100 and kept[~b["lost"]].sum() < n_hits[~b["lost"]].sum()
        for length in sx.SEED_QLENS:                                 # ... in reads of every length
            assert sum(int((want[r][:, 1] >> np.uint64(43) & np.uint64(1)).sum()) for r in np.flatnonzero(qlen == length)) > 20, length


@pytest.mark.parametrize("name", ["none", "no_diag_no_dual"])
def test_a_length_taken_from_the_waves_previous_read_shows(seed_data, name):
    """Why the reads' lengths vary: with the length of the read W before it -- what a wave that kept its previous read's scalar would use -- most reads of the second
    and third pass that keep a reverse-strand anchor get other anchors, the hard reads at W, 2 W - 1, 2 W and N - 1 among them; under MM_F_NO_DIAG the number kept changes too."""
    b, flag = seed_data, sx.SEED_FLAGS[name]
    hard, _, _ = sx.special(W, N)
    want = sx.seed_want(b, flag)
    stale = dict(b, reads=[dict(rd, qlen=b["reads"][r - W]["qlen"]) if r >= W else rd for r, rd in enumerate(b["reads"])])
    other = sx.seed_want(stale, flag)
    differs = np.asarray([a.shape != o.shape or not np.array_equal(a, o) for a, o in zip(want, other)])
    has_rev = np.asarray([bool((a[:, 0] >> np.uint64(63)).any()) for a in want])
    assert not differs[:W].any() and differs[W:].sum() > 0.6 * has_rev[W:].sum() > 1_000 and all(differs[r] for r in hard if r >= W)
    if flag:
        assert sum(len(a) != len(o) for a, o in zip(want, other)) > 20


@pytest.fixture(scope="module")
def heap_data():
    return sx.heap_batch(W, N)


@pytest.mark.parametrize("name", list(sx.HEAP_FLAGS))
def test_heap_batch_on_the_host_form(heap_data, name):
    b, flag = heap_data, sx.HEAP_FLAGS[name]
    got, host_tied = mm.collect_seeds_heap_host(flag, b["reads"])
    want = [sc.heap_literal(rd, flag) for rd in b["reads"]]
    bad = sx.first_difference(*sx.lay(got), *sx.lay(want), W, name)
    assert bad is None, bad
    hard, blank, dropped = sx.special(W, N)
    assert host_tied == int(b["tied"].sum()) and N // 100 <= host_tied <= N // 10 and not b["tied"][hard + blank + dropped].any()
    print(f"{host_tied} of {N} reads tied ({100 * host_tied / N:.2f} %), {len(b['long'])} long reads, {sum(len(rd['hits']) for rd in b['reads'])} hits")
    n_hits = np.asarray([len(rd["hits"]) for rd in b["reads"]])
    assert len(b["long"]) >= 190 and (n_hits[b["long"]] > sc.WAVE_HITS).all() and int(b["tied"][b["long"]].sum()) == sx.N_LONG_TIED
    assert (n_hits > sc.WAVE_HITS).sum() == len(b["long"]) + 2 and [int(n_hits[r]) for r in hard] == [sc.WAVE_HITS, sc.WAVE_HITS + 1, 65, 65, sc.WAVE_HITS + 1]
    for rd in (b["reads"][r] for r in (2, W + 5, N - 7)):            # a seed's list is ascending and distinct, as an index's
        cut = np.cumsum(rd["seeds"][:, 0].astype(int))[:-1]
        assert all((np.diff(l.astype(np.int64)) > 0).all() for l in np.split(rd["hits"], cut))
    if flag:
        assert all(len(got[r]) == 0 and n_hits[r] > 0 for r in dropped)


def test_builders_hold_their_conditions_at_other_device_sizes():
    for cu in (4, 304):
        w, n = sx.sizes(cu)
        hard, blank, dropped = sx.special(w, n)
        h = sx.heap_batch(w, n)
        assert n // 100 <= int(h["tied"].sum()) <= n // 10 and not h["tied"][hard + blank + dropped].any() and int(h["tied"][h["long"]].sum()) == sx.N_LONG_TIED
        s = sx.seed_batch(w, n)
        n_hits = np.asarray([len(rd["hits"]) for rd in s["reads"]])
        assert (s["lost"] & (n_hits > 0)).sum() >= n // 5 and (n_hits[hard] >= 40).all()
        a, off = sx.sort_batch(w, n)
        assert [int(np.diff(off)[r]) for r in hard] == [65, 5_000, 40, 64, 65]
        assert [int(np.diff(sx.chain_batch(w, n)["u_off"])[r]) for r in hard] == [65, 64, 5, 64, 65]


def test_sort_and_chain_batches():
    a, off = sx.sort_batch(W, N)
    hard, blank, _ = sx.special(W, N)
    cnt = np.diff(off)
    assert [int(cnt[r]) for r in hard] == [65, 5_000, 40, 64, 65] and (cnt[blank] == 0).all() and cnt.max() == 5_000 and len(a) == off[-1]
    assert len(np.unique(a[:off[W - 1], 0])) <= 24                   # a dozen positions on two strands: equal x in nearly every read
    want = sx.sort_want(a, off)
    big = want[off[hard[1]]:off[hard[1] + 1], 0]
    assert len(want) == len(a) and not np.array_equal(want, a) and (big[1:] >= big[:-1]).all() and len(np.unique(big)) <= 600
    b = sx.chain_batch(W, N)
    inner = b["dx"] > 0
    both = inner & (b["dx"] > b["span"]) & (b["dy"] > b["span"])
    assert both.sum() > 1_000 and (inner & ~both).sum() > 1_000 and 0.2 < b["near"].mean() < 0.3
    regs = sx.regs_want(b, 0)
    assert len(regs) == b["u_off"][-1] and (regs["rs"] == 0).sum() > 100 and (regs["qs"] >= 0).all() and (regs["qe"] <= np.repeat(b["qlen"], np.diff(b["u_off"]))).all()
    rq = sx.regs_want(b, 1)
    rev = regs["flags"] & (1 << 10) != 0
    assert rev.sum() > 1_000 and (~rev).sum() > 1_000 and (regs["qs"][rev] != rq["qs"][rev]).any() and np.array_equal(regs["qs"][~rev], rq["qs"][~rev])
    # equal scores inside a read: the hash decides, and another hash decides otherwise
    r = hard[2]
    u, ch = b["chains"][r]
    one, other = orc.gen_regs(u, ch, int(b["qlen"][r]), 1), orc.gen_regs(u, ch, int(b["qlen"][r]), 2)
    assert len(set(one["score"].tolist())) == 1 and one["as_"].tolist() != other["as_"].tolist()


@pytest.mark.skipif(not orc.ref_available(), reason="the reference library is built only where its checkout exists")
def test_crafted_chains_through_the_references_mm_gen_regs():
    b = sx.chain_batch(W, N)
    hard, _, _ = sx.special(W, N)
    for r in hard + list(range(2, 400)):
        u, a = b["chains"][r]
        for is_q in (0, 1):
            assert np.array_equal(orc.gen_regs(u, a, int(b["qlen"][r]), int(b["hashes"][r]), is_q), orc.ref_gen_regs(u, a, int(b["qlen"][r]), int(b["hashes"][r]), is_q)), sx.where(r, W)


def test_match_reads_thin_more_streaks_than_one_step_selects():
    reads = sx.match_reads(W, N)
    _, blank, dropped = sx.special(W, N)
    assert len(reads) == N and sorted(len(reads[r]) for r in blank) == [0, 15, 120] and all(80 <= len(s) <= 150 for r, s in enumerate(reads) if r not in blank + dropped)
    unfiltered = sx.host_matches(reads, mid_occ=1 << 30, q_occ_frac=0.0)
    streaks = sx.thinned_streaks(unfiltered, 2, 50)
    print(f"{streaks} thinned streaks in {N} reads")
    assert streaks >= 9_000 > sx.SELECT_GRID
    # the count on a small example: a run of three matches above mid_occ between two below it, 100 bases apart -> keep 2 of 3; a read of one match does not count
    m = lambda occ, q, qlen: dict(seeds=np.asarray([[o, p << 1, 21, 0] for o, p in zip(occ, q)], np.uint32).reshape(-1, 4), qlen=qlen)
    assert sx.thinned_streaks([m([1, 9, 9, 9, 1], [30, 50, 70, 90, 130], 200), m([9], [40], 100), m([], [], 50)], 2, 50) == 1
    assert sx.thinned_streaks([m([9, 9, 9], [30, 50, 70], 120)], 2, 50) == 1 and sx.thinned_streaks([m([9, 9], [30, 50], 120)], 2, 50) == 0
    for name, kw in sx.MATCH_OPTS.items():
        want = sx.host_matches(reads, **kw)
        rep = np.asarray([x["rep_len"] for x in want])
        assert (rep[sx.REP_LEN_GRID:] > 0).sum() >= 10 and (rep[:sx.REP_LEN_GRID] > 0).sum() >= 9_000, name
        assert all(len(want[r]["seeds"]) == 0 for r in blank + dropped)
        kept, was = sum(len(x["seeds"]) for x in want), sum(len(x["seeds"]) for x in unfiltered)
        assert 0 < kept < was


def test_recorded_long_read_texts():
    assert os.path.getsize(os.path.join(sx.GOLD, "scale.npz")) < 64 * 1024
    lines = {run: sx.long_paf(run).splitlines() for run in sx.LONG_RUNS}
    assert {run: len(v) for run, v in lines.items()} == {"ont": 370, "pb": 344, "ont.nolj": 370, "pb.nolj": 344}
    names = {n for n, _ in sc.reads()}
    for run, v in lines.items():
        mapped = {ln.split("\t")[0] for ln in v}
        assert mapped < names and len(mapped) == (205 if run.startswith("ont") else 199) and sum("tp:A:S" in ln for ln in v) >= 100
    assert sx.copies(N) == 79 and sx.copies(209) == 1 and sx.copies(210) == 2


@pytest.mark.skipif(not os.path.exists(sx.REF_EXE), reason="the reference program is built only where its checkout exists")
def test_the_reference_program_prints_the_recorded_texts():
    doc = sx.record_long()
    assert doc == {run: sx.long_paf(run) for run in sx.LONG_RUNS}
    # the file's member, uncompressed, is the document as the tool serialises it (the compressed bytes depend on the deflate library and are not compared)
    again = np.load(io.BytesIO(sx.long_doc_bytes(doc)))["doc"].tobytes()
    assert again == np.load(os.path.join(sx.GOLD, "scale.npz"))["doc"].tobytes() == json.dumps(doc, sort_keys=True).encode("utf-8")
