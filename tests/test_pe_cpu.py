"""Paired-end short reads on the host: fragment formation, the fragment entry of the host seeding against the reference program's SD / RS lines (tests/golden/pe), and
mm_select_sub_multi and mm_seg_gen as batched host calls against what the built reference's exported functions returned on the fixture (recorded by
tests/tools/gen_golden_pe.py) and against plain-Python restatements on crafted records and anchors.  Every comparison is exact.  The mapper itself needs a device:
tests/test_gpu_pe.py."""
import numpy as np
import pytest

import pe_cases as pc

mm = pytest.importorskip("mm2gb_amd")


# ---------------------------------------------------------------- fragments
def test_fragment_formation():
    names = ["a/1", "a/2", "lone", "b/1", "b/2", "plain", "plain", "x1", "x2", "c/1", "d/2", "e/12", "e/13", "/1", "/2", "ab/1", "abc/2"]
    #         a         lone    b             plain            x1    x2    c      d      e/12    e/13    "/1" "/2": shorter than three, the whole name    ab   abc
    assert mm.frag_offsets(names).tolist() == [0, 2, 3, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17]
    assert mm.frag_offsets([]).tolist() == [0] and mm.frag_offsets(["r"]).tolist() == [0, 1]
    assert mm.frag_offsets(["t/1", "t/2", "t/3"]).tolist() == [0, 3]                 # a run of three is one fragment here; the mapping calls refuse it by name
    r1, r2 = [("p/1", b"AC"), ("q/1", b"GT")], [("p/2", b"CA"), ("q/2", b"TG")]
    assert mm.interleave(r1, r2) == [r1[0], r2[0], r1[1], r2[1]]
    with pytest.raises(mm.Mm2gbError, match="differ in length"):
        mm.interleave(r1, r2[:1])


def test_the_fixture_is_worth_having():
    g = pc.gold()
    worth = pc.worth_having(g["pafs"], g["se"])
    assert all(worth.values()), worth
    frags = pc.fragments()
    assert len(frags) == len(g["seeds"]) >= 100 and sorted({len(f) for f in frags}) == [1, 2]
    assert len({sum(len(s) for _, s in f) for f in frags if len(f) == 2}) >= 4
    names = [f[0][0] for f in frags]
    for tag in ("fam0_", "fam1_", "overlap", "far", "cross", "stray", "tiny", "withn", "lone", "plain"):
        assert any(n.startswith(tag) for n in names), tag
    i = names.index("lone")
    assert len(frags[i]) == 1 and len(frags[i - 1]) == len(frags[i + 1]) == 2
    plain = [n for n, _ in next(f for f in frags if f[0][0].startswith("plain"))]
    assert len(plain) == 2 and plain[0] == plain[1] and "/" not in plain[0]
    assert set(pc.RUNS) == set(g["pafs"]) and g["options"]["max_chain_skip"] == 2**31 - 1


def test_new_symbols_are_exported():
    for name in ("mm2gb_collect_matches_frag", "mm2gb_collect_matches_frag_gpu", "mm2gb_frag_offsets", "mm2gb_map_frags_sr", "mm2gb_map_frags_stream_sr",
                 "mm2gb_select_sub_multi_host", "mm2gb_seg_gen_host", "mm2gb_seg_out_free"):
        assert hasattr(mm.lib(), name) and name in mm.CORE_SYMBOLS, name


# ---------------------------------------------------------------- seeding a fragment
def test_matches_frag_gives_the_recorded_anchors_and_rep_len():
    frags = pc.fragments()
    m = pc.matches_frag(frags)
    got, _ = mm.collect_seeds_heap_host(mm.map_opt_sr().flag, m)
    rec = pc.gold()["seeds"]
    n_both = 0
    for f, a, x, want in zip(frags, got, m, rec):
        assert x["qlen"] == sum(len(s) for _, s in f)
        assert pc.sd_rows(a) == want["sd"] and x["rep_len"] == want["rep_len"], f[0][0]
        n_both += len({int(y) >> 48 & 0xff for y in np.asarray(a, np.uint64).reshape(-1, 2)[:, 1]}) == 2
    assert n_both >= 80                                 # anchors of both mates in one list: the segment ids travel


def test_a_fragment_of_one_read_is_the_read():
    o = mm.map_opt_sr()
    for _, s in pc.reads()[:12]:
        a, b = pc.index().matches_frag([s], o.mid_occ), pc.index().matches(s, o.mid_occ)
        assert all(np.array_equal(a[k], b[k]) for k in ("seeds", "hits", "mini_pos")) and (a["rep_len"], a["qlen"]) == (b["rep_len"], b["qlen"])
    with pytest.raises(mm.Mm2gbError, match="one or two segments"):
        pc.index().matches_frag([b"ACGT"] * 3, o.mid_occ)


def test_the_second_mate_lies_behind_the_first():
    """A fragment's seeds are the first mate's own followed by the second mate's with the first's length added and segment id 1 -- where no filter and no streak sees the
    other mate (mid_occ above every occurrence count)."""
    f = pc.fragments()[0]
    s0, s1 = pc.oriented(f)
    ix, big = pc.index(), 1 << 30
    both, m0, m1 = ix.matches_frag([s0, s1], big, q_occ_frac=0.0), ix.matches(s0, big, q_occ_frac=0.0), ix.matches(s1, big, q_occ_frac=0.0)
    assert len(m0["seeds"]) > 0 and len(m1["seeds"]) > 0
    moved = m1["seeds"].copy()
    moved[:, 1] += np.uint32(len(s0) << 1)
    moved[:, 3] |= 1
    assert np.array_equal(both["seeds"], np.concatenate([m0["seeds"], moved]))
    assert np.array_equal(both["hits"], np.concatenate([m0["hits"], m1["hits"]]))
    assert np.array_equal(both["mini_pos"], np.concatenate([m0["mini_pos"], m1["mini_pos"] + np.uint64(len(s0))]))


def test_crafted_fragments_are_what_they_are_named():
    """The host form on the crafted fragments of tests/test_gpu_pe.py shows what each is for (so that the device comparison there is about that)."""
    g, cases = pc.crafted_frags()
    with mm.SeedIndex([g], threads=4, **mm.preset_sr()) as ix:
        _crafted_checks(cases, ix)


def _crafted_checks(cases, ix):
    host = {n: ix.matches_frag(mates, **kw) for n, (mates, kw) in cases.items()}
    alone = {n: [ix.matches(s, **kw) for s in mates] for n, (mates, kw) in cases.items()}
    assert len(host["first_mate_below_k"]["seeds"]) > 0 and (host["first_mate_below_k"]["seeds"][:, 3] & 1).all()
    assert len(host["second_mate_below_k"]["seeds"]) > 0 and not (host["second_mate_below_k"]["seeds"][:, 3] & 1).any()
    assert len(host["both_below_k"]["seeds"]) == 0
    tw, (t0, t1) = host["twin_across_boundary"]["seeds"], alone["twin_across_boundary"]
    assert not (t0["seeds"][:, 3] >> 31).any() and not (t1["seeds"][:, 3] >> 31).any()
    assert (tw[:, 3] >> 31).tolist() == [0] * (len(t0["seeds"]) - 1) + [1, 1] + [0] * (len(t1["seeds"]) - 1)          # MM_SEED_TANDEM on the two neighbours only
    for n in ("streak_across_boundary", "streak_fills_both"):
        h, (a0, a1) = host[n], alone[n]
        assert h["rep_len"] > 0 and a0["rep_len"] > 0 and a1["rep_len"] > 0
        # the streak's length and count are the fragment's: what survives is not the mates' own survivors side by side
        moved = a1["seeds"][:, 1].astype(np.int64) + (len(cases[n][0][0]) << 1)
        assert h["seeds"][:, 1].tolist() != a0["seeds"][:, 1].tolist() + moved.tolist() or h["rep_len"] != a0["rep_len"] + a1["rep_len"]
    (m0, m1), kw = cases["q_filter_joint_only"]
    unfiltered = [ix.matches(s, **dict(kw, q_occ_frac=0.0)) for s in (m0, m1)]
    assert all(np.array_equal(u["seeds"], a["seeds"]) for u, a in zip(unfiltered, alone["q_filter_joint_only"]))             # neither mate's own list is thinned
    joint_unfiltered = ix.matches_frag([m0, m1], **dict(kw, q_occ_frac=0.0))
    joint = host["q_filter_joint_only"]
    assert not (np.array_equal(joint["seeds"], joint_unfiltered["seeds"]) and joint["rep_len"] == joint_unfiltered["rep_len"])     # the joint one is


# ---------------------------------------------------------------- mm_select_sub_multi
def _select(regs, qlens, max_gap_ref, **kw):
    return mm.select_sub_multi_host([regs], [qlens], [max_gap_ref], **kw)[0]


def test_select_sub_multi_on_the_fixture():
    gp = pc.golden_post()
    o, sr = mm.map_opt_sr(), mm.map_sr()
    kept = mm.select_sub_multi_host([p["regs_in"] for p in gp], [p["qlens"] for p in gp], [pc.max_dist_x(o, sr, sum(p["qlens"])) for p in gp], pri_ratio=o.pri_ratio,
                                    min_diff=2 * pc.K, best_n=o.best_n)
    assert sum(len(p["regs_in"]) - len(p["regs_kept"]) for p in gp) >= 100          # the step drops records on this set
    for f, (k, p) in enumerate(zip(kept, gp)):
        assert np.array_equal(k, p["regs_kept"]), f


SELECT_KW = dict(pri_ratio=0.5, pri1=0.2, pri2=0.7, min_diff=42)


def crafted_select():
    """qlens (100, 100), max_gap_ref 600 (max_dist 800).  Record 0: a primary of score 200 across the mates' boundary; record 9: a primary inside mate 0."""
    r = [pc.reg(0, 0, 200, 0, False, 1_000, 1_300, 20, 180),
         pc.reg(1, 0, 158, 1, True, 5_000, 5_100, 0, 90),        # within min_diff (158 + 42 >= 200): stays whatever else holds
         pc.reg(2, 0, 40, 0, False, 1_400, 1_500, 0, 90),        # close on the reference: pri1 (40 >= 200 * 0.2)
         pc.reg(3, 0, 39, 0, False, 1_400, 1_500, 0, 90),        # ... one below: goes
         pc.reg(4, 0, 100, 0, False, 1_800, 1_900, 50, 150),     # q.re - p.rs = 900 >= 800: not close; the child spans the boundary: pri_ratio (100 >= 100)
         pc.reg(5, 0, 99, 0, True, 1_400, 1_500, 50, 150),       # the other strand: not close; spans; one below: goes
         pc.reg(6, 0, 140, 1, False, 1_400, 1_500, 0, 90),       # another sequence; the parent spans and the child does not: pri2 (140 >= 140)
         pc.reg(7, 0, 139, 1, False, 1_400, 1_500, 0, 90),       # ... one below: goes
         pc.reg(8, 8, 120, 1, False, 9_000, 9_090, 0, 90),       # a primary inside mate 0
         pc.reg(9, 8, 60, 0, False, 100, 190, 10, 80),           # neither spans: pri_ratio (60 >= 60)
         pc.reg(10, 8, 59, 0, False, 100, 190, 10, 80)]          # ... one below: goes
    return np.concatenate(r)


def test_select_sub_multi_branches():
    r = crafted_select()
    got = _select(r, [100, 100], 600, best_n=20, **SELECT_KW)
    want = pc.select_literal(r, [100, 100], 600, best_n=20, **SELECT_KW)
    assert want == [0, 1, 2, 4, 6, 8, 9]
    assert [int(x) for x in got["hash"]] == [1000 - i for i in want]            # (hash names the source record)
    assert got["id"].tolist() == list(range(7)) and got["parent"].tolist() == [0, 0, 0, 0, 0, 5, 5]
    # best_n exceeded: the third secondary that would stay is the last one
    got = _select(r, [100, 100], 600, best_n=3, **SELECT_KW)
    assert [1000 - int(x) for x in got["hash"]] == pc.select_literal(r, [100, 100], 600, best_n=3, **SELECT_KW) == [0, 1, 2, 4, 8]
    # one segment: max_dist 0 (nothing is close), nothing spans: pri_ratio throughout
    got = _select(r, [200], 600, best_n=20, **SELECT_KW)
    assert [1000 - int(x) for x in got["hash"]] == pc.select_literal(r, [200], 600, best_n=20, **SELECT_KW) == [0, 1, 4, 6, 7, 8, 9]
    # nothing dropped: the records come back as they went in; pri_ratio 0: the step does not run
    keep_all = np.concatenate([r[:3], r[8:10]])
    keep_all["parent"][3:], keep_all["id"][3:] = 3, [3, 4]
    assert np.array_equal(_select(keep_all, [100, 100], 600, best_n=20, **SELECT_KW), keep_all)
    assert np.array_equal(_select(r, [100, 100], 600, best_n=20, **dict(SELECT_KW, pri_ratio=0.0)), r)
    assert len(_select(r[:0], [100, 100], 600)) == 0


def test_select_sub_multi_random_against_the_restatement():
    rng = np.random.default_rng(3)
    for trial in range(200):
        n = int(rng.integers(1, 14))
        regs, prim = [], []
        for i in range(n):
            if not prim or rng.random() < 0.3:
                prim.append(i)
                parent = i
            else:
                parent = prim[int(rng.integers(0, len(prim)))]
            qs = int(rng.integers(0, 150))
            rs = int(rng.integers(0, 3_000))
            regs.append(pc.reg(i, parent, int(rng.integers(20, 260)), int(rng.integers(0, 2)), bool(rng.integers(0, 2)), rs, rs + int(rng.integers(30, 300)), qs,
                               qs + int(rng.integers(20, 100))))
        r = np.concatenate(regs)
        best_n = int(rng.integers(1, 6))
        got = _select(r, [100, 120], 500, best_n=best_n, **SELECT_KW)
        assert [1000 - int(x) for x in got["hash"]] == pc.select_literal(r, [100, 120], 500, best_n=best_n, **SELECT_KW), trial


def test_select_sub_multi_refusals():
    r = crafted_select()
    with pytest.raises(mm.Mm2gbError, match="one or two segments"):
        _select(r, [50, 50, 50], 600)
    bad = r.copy()
    bad["parent"][2] = 5
    with pytest.raises(mm.Mm2gbError, match="parent"):
        _select(bad, [100, 100], 600)


# ---------------------------------------------------------------- mm_seg_gen
def test_seg_gen_on_the_fixture():
    gp = pc.golden_post()
    ids = [f for f, fr in enumerate(pc.fragments()) if len(fr) == 2]
    got = mm.seg_gen_host([p["regs_kept"] for p in gp], [p["anchors"] for p in gp], [p["qlens"] for p in gp], [pc.frag_hash(i) for i in ids])
    n_one, n_rev = 0, 0
    for f, (g, p) in enumerate(zip(got, gp)):
        for s in range(2):
            assert np.array_equal(g[s][0], p["seg"][s][0]) and np.array_equal(g[s][1], p["seg"][s][1]), (f, s)
            n_one += int((g[s][0]["cnt"] == 1).sum())
            n_rev += int((g[s][0]["flags"] >> 10 & 1).sum())
    assert n_one >= 1 and n_rev >= 20                  # a per-mate hit of one anchor (the cm:i:1 line), reverse-strand hits


def _chain(score, anchors, as_):
    a = np.asarray(anchors, np.uint64).reshape(-1, 2)
    rev = bool(int(a[0][0]) >> 63)
    r = pc.reg(0, 0, score, 0, rev, 0, 0, 0, 0, cnt=len(a), as_=as_)
    return r


def crafted_seg():
    """Four records on a fragment of 100 + 80 bases: all in mate 0; all in mate 1; strictly alternating on the reverse strand; one anchor per mate."""
    A = pc.anchor
    chains = [(90, [A(1_000 + 30 * i, 30 + 15 * i, 0) for i in range(4)]),
              (80, [A(5_000 + 20 * i, 100 + 25 + 12 * i, 1) for i in range(3)]),
              (70, [A(9_000, 30, 1, rev=True), A(9_040, 100, 0, rev=True), A(9_080, 50, 1, rev=True), A(9_120, 140, 0, rev=True)]),   # reverse strand: positions below 80 are mate 1's
              (60, [A(12_000, 50, 0), A(12_300, 150, 1)])]
    regs, anchors, at = [], [], 0
    for i, (score, a) in enumerate(chains):
        r = _chain(score, a, at)
        r["id"] = r["parent"] = i
        regs.append(r)
        anchors += a
        at += len(a)
    return np.concatenate(regs), np.asarray(anchors, np.uint64)


def test_seg_gen_crafted():
    regs, anchors = crafted_seg()
    qlens = [100, 80]
    (got,) = mm.seg_gen_host([regs], [anchors], [qlens], [77])
    lit = pc.seg_literal(regs, anchors, qlens)
    for s in range(2):
        r, a = got[s]
        u, sa = lit[s]
        assert np.array_equal(a, sa)
        assert sorted((int(x["score"]) << 32 | int(x["cnt"])) for x in r) == sorted(u) and r["score"].tolist() == sorted(r["score"].tolist(), reverse=True)
        assert (r["flags"] >> 15 & 1).all() and (r["flags"] >> 16 & 0xff == s).all() and r["id"].tolist() == list(range(len(r))) and (r["parent"] == -1).all()
        assert sum(int(x["cnt"]) for x in r) == len(a) and (a[:, 1] >> np.uint64(48) & np.uint64(0xff) == s).all()
        assert ((a[:, 1] & np.uint64(0xffffffff)).astype(np.int64) < qlens[s]).all()
    # mate 0: the chain all its own (4 anchors), two of the alternating one, one of the last; mate 1 likewise
    assert sorted(got[0][0]["cnt"].tolist()) == [1, 2, 4] and sorted(got[1][0]["cnt"].tolist()) == [1, 2, 3]
    # coordinates in the mate's own frame.  Forward, mate 1: y - 100 (125, 137, 149 -> 25, 37, 49)
    box = lambda x: tuple(int(x[k]) for k in ("qs", "qe", "rs", "re"))
    assert box(got[1][0][got[1][0]["score"] == 80][0]) == (25 + 1 - 21, 49 + 1, 5_000 + 1 - 21, 5_040 + 1)
    # reverse: mate 1 lies first in the fragment's reversed frame, so its y stays (30, 50) and mate 0's drops by 80 (100, 140 -> 20, 60); qs / qe count from the mate's own end
    rv0, rv1 = got[0][0][got[0][0]["score"] == 70][0], got[1][0][got[1][0]["score"] == 70][0]
    assert int(rv0["flags"]) >> 10 & 1 and int(rv1["flags"]) >> 10 & 1
    assert box(rv1) == (80 - (50 + 1), 80 - (30 + 1 - 21), 9_000 + 1 - 21, 9_080 + 1)
    assert box(rv0) == (100 - (60 + 1), 100 - (20 + 1 - 21), 9_040 + 1 - 21, 9_120 + 1)
    # a fragment without a record, and one of a single segment (the record comes back as mm_gen_regs makes it, seg_id 0)
    none = mm.seg_gen_host([regs[:0]], [anchors[:0]], [qlens], [5])[0]
    assert all(len(r) == 0 and len(a) == 0 for r, a in none)
    (single,) = mm.seg_gen_host([regs[:1]], [anchors[:4]], [[100]], [5])
    assert len(single) == 1 and single[0][0]["cnt"].tolist() == [4] and np.array_equal(single[0][1], anchors[:4].reshape(-1, 2))


def test_seg_gen_refusals():
    regs, anchors = crafted_seg()
    with pytest.raises(mm.Mm2gbError, match="segment id is not below n_segs"):
        mm.seg_gen_host([regs], [anchors], [[180]], [1])
    bad = regs.copy()
    bad["cnt"][3] = 9
    with pytest.raises(mm.Mm2gbError, match="outside its fragment"):
        mm.seg_gen_host([bad], [anchors], [[100, 80]], [1])
