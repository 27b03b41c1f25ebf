"""Paired-end short reads on the device.  Seeding a fragment (Engine.collect_matches_frag: the sketch, one kernel that moves the second mates behind the first and
re-labels minimizers with their fragment, the match kernels on per-fragment offsets) against the host form record for record, on the fixture, on crafted fragments -- a
mate shorter than k, equal minimizers on either side of the mates' boundary, a dropped streak across it, a joint list that the q-occurrence filter thins where neither
mate's own is, single reads among pairs -- and on a batch with more fragments than the capped grids.  The mapper (mm2gb_map_frags_sr / _stream_sr) against every PAF the
reference program printed for tests/golden/pe, byte for byte, seeded on the host and on the device, whole and as a stream; the refusals; batches without fragments."""
import numpy as np
import pytest

import pe_cases as pc
import scale_cases as sx
import sr_cases as sc

pytestmark = pytest.mark.gpu

mm = pytest.importorskip("mm2gb_amd")


@pytest.fixture(scope="module")
def engine():
    with mm.Engine() as e:
        yield e


def same(got, want, names):
    assert len(got) == len(want) == len(names)
    for n, a, b in zip(names, got, want):
        for k in ("seeds", "hits", "mini_pos"):
            assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (n, k)
        assert (a["rep_len"], a["qlen"]) == (b["rep_len"], b["qlen"]), n


# ---------------------------------------------------------------- seeding a fragment
@pytest.mark.parametrize("mid_occ", [None, 4], ids=["preset", "f4"])
def test_collect_matches_frag_on_the_fixture(engine, mid_occ):
    frags = pc.fragments()
    o = mm.map_opt_sr()
    want = pc.matches_frag(frags, mid_occ=mid_occ)
    got = engine.collect_matches_frag(pc.index(), [pc.oriented(f) for f in frags], o.mid_occ if mid_occ is None else mid_occ, o.max_max_occ, o.occ_dist, o.q_occ_frac)
    same(got, want, [f[0][0] for f in frags])
    assert sum((m["seeds"][:, 3] & 1).any() and not (m["seeds"][:, 3] & 1).all() for m in got) >= 80       # seeds of both mates in one fragment
    if mid_occ == 4:
        assert sum(m["rep_len"] > 0 for m in got) >= 10


@pytest.fixture(scope="module")
def crafted():
    g, cases = pc.crafted_frags()
    with mm.SeedIndex([g], threads=4, **mm.preset_sr()) as ix:
        yield g, cases, ix


def test_collect_matches_frag_crafted(engine, crafted):
    g, cases, ix = crafted
    by_opt = {}
    for n, (mates, kw) in cases.items():
        by_opt.setdefault(tuple(sorted(kw.items())), []).append(n)
    for key, names in by_opt.items():
        kw = dict(key)
        # single reads and two-mate fragments mixed in one batch, in both orders; then every fragment as a batch of its own
        for order in (names, names[::-1]):
            frags = [cases[n][0] for n in order]
            same(engine.collect_matches_frag(ix, frags, **kw), [ix.matches_frag(f, **kw) for f in frags], order)
        for n in names:
            same(engine.collect_matches_frag(ix, [cases[n][0]], **kw), [ix.matches_frag(cases[n][0], **kw)], [n])
    # a batch of single reads through the fragment call is the read call's
    seqs = [m for n in cases for m in cases[n][0]]
    kw = cases["single"][1]
    same(engine.collect_matches_frag(ix, [[s] for s in seqs], **kw), engine.collect_matches(ix, seqs, **kw), [str(i) for i in range(len(seqs))])
    with pytest.raises(mm.Mm2gbError, match="one or two sequences"):
        engine.collect_matches_frag(ix, [[seqs[0], seqs[1], seqs[2]]], **kw)


def test_collect_matches_frag_beyond_the_grids(engine):
    """More fragments than k_m_rep_len's 16384 blocks and more thinned streaks than k_m_select's 8192: every kernel that strides over fragments takes a second step on
    data that is compared.  Two mates of 80-150 bases each, two thirds from the short-read fixture's tandem array; every seventh fragment a single read."""
    n_frag = sx.REP_LEN_GRID + 37
    reads = sx.match_reads(8_192, 2 * n_frag)
    frags = [[reads[2 * f]] if f % 7 == 3 else [reads[2 * f], reads[2 * f + 1]] for f in range(n_frag)]
    kw = sx.MATCH_OPTS["q1e-4"]
    ix = sc.index()
    want = [ix.matches_frag(f, **kw) for f in frags]
    rep = np.asarray([m["rep_len"] for m in want])
    assert (rep[sx.REP_LEN_GRID:] > 0).sum() >= 10 and (rep[:sx.REP_LEN_GRID] > 0).sum() >= 9_000
    got = engine.collect_matches_frag(ix, frags, **kw)
    bad = next((f for f in range(n_frag) if not all(np.array_equal(got[f][k], want[f][k]) for k in ("seeds", "hits", "mini_pos")) or got[f]["rep_len"] != want[f]["rep_len"]), None)
    assert bad is None, f"fragment {bad} of {n_frag}"


# ---------------------------------------------------------------- the mapper
def distinct_keys(rd, o, sr):
    """The chaining calls' keys (n_seg, max_dist_x, max_dist_y) among a batch's fragments; single reads share one max_dist_y."""
    frags = pc.fragments(rd)
    single = max([len(f[0][1]) for f in frags if len(f) == 1] + [0])
    return {(len(f), pc.max_dist_x(o, sr, sum(len(s) for _, s in f)), max(sum(len(s) for _, s in f) if len(f) == 2 else single, o.max_gap)) for f in frags}


@pytest.mark.parametrize("stream", [False, True], ids=["whole", "stream"])
@pytest.mark.parametrize("seeding", [0, 1], ids=["host_seeds", "device_seeds"])
@pytest.mark.parametrize("run", list(pc.RUNS))
def test_mapper_equals_the_recorded_paf(engine, run, seeding, stream):
    paf, st = pc.map_run(engine, run, stream=stream, seeding_on_device=seeding)
    want = pc.golden_paf(run)
    if paf != want:
        got_l, want_l = paf.splitlines(), want.splitlines()
        first = next((i for i, (a, b) in enumerate(zip(got_l, want_l)) if a != b), min(len(got_l), len(want_l)))
        raise AssertionError(f"{run}: line {first} of {len(got_l)} / {len(want_l)}:\n{got_l[first:first + 1]}\n{want_l[first:first + 1]}")
    assert st["n_reads"] == len(pc.fragments())
    if run == "pe.f4_50":
        assert st["n_rescued"] > 0
    if run == "pe.f4_4":
        assert st["n_rescued"] == 0
    if not stream:
        o = mm.map_opt_sr()
        n_keys = len(distinct_keys(pc.reads(), o, mm.map_sr()))
        assert n_keys >= 5 and st["n_chain_calls"] >= n_keys
        print(f"{run}: {st['n_chain_calls']} chaining calls for {n_keys} keys, {st['n_rescued']} fragments rescued")


def test_a_finite_max_chain_skip_beyond_every_fragment(engine):
    """max_chain_skip = 5000 takes the finite-skip path of the score kernels (k_skip_fill); no fragment has as many anchors before one target, so the recorded PAF stands."""
    for seeding in (0, 1):
        paf, _ = pc.map_run(engine, "pe", max_chain_skip=5_000, seeding_on_device=seeding)
        assert paf == pc.golden_paf("pe")


def test_pairs_are_not_mapped_singly(engine):
    """Condition 1 of the fixture on this project's own output: mapped as single reads (no frags=), some mates get another target or quality than in the pair."""
    rd = pc.reads()
    opt = mm.map_opt_sr(host_threads=4)
    single, _ = mm.map_reads(engine, pc.index(), [n for n, _ in pc.contigs()], rd, opt=opt, k=pc.K, align=mm.map_sr())
    assert single != pc.golden_paf("pe")
    mates1 = "".join(ln + "\n" for ln in single.splitlines() if ln.split("\t")[0].endswith("/1"))
    mates2 = "".join(ln + "\n" for ln in single.splitlines() if ln.split("\t")[0].endswith("/2"))
    assert pc.worth_having(pc.gold()["pafs"], mates1 + mates2)["1 a mate's line differs from single-end in target or mapq"]


def flip(line, qlen):
    f = line.split("\t")
    f[2], f[3], f[4] = str(qlen - int(f[3])), str(qlen - int(f[2])), "+-"[f[4] == "+"]
    return "\t".join(f)


@pytest.mark.parametrize("pe_ori", [0, 2, 3])
def test_pe_ori(engine, pe_ori):
    """pe_ori turns a mate before mapping and flips its hits back after it: given reads that are turned already where pe_ori differs from 1, the mapper sees the fragments
    of the recorded run, and a line differs from the recorded one only in that a mate given turned has qs, qe and strand in the turned read's frame."""
    turned = [(pe_ori ^ 1) >> 1 & 1, (pe_ori ^ 1) & 1]
    rd = []
    for f in pc.fragments():
        rd += [(n, pc.revcomp(s) if len(f) == 2 and turned[j] else s) for j, (n, s) in enumerate(f)]
    paf, _ = pc.map_run(engine, "pe", rd=rd, pe_ori=pe_ori)
    mate_of = {}
    for f in pc.fragments():
        if len(f) == 2 and f[0][0] != f[1][0]:
            mate_of.update({f[0][0]: 0, f[1][0]: 1})
    want = [flip(ln, int(ln.split("\t")[1])) if turned[mate_of.get(ln.split("\t")[0], 0)] and ln.split("\t")[0] in mate_of else ln for ln in pc.golden_paf("pe").splitlines()]
    got = paf.splitlines()
    plain = next(f[0][0] for f in pc.fragments() if f[0][0].startswith("plain"))        # (both mates carry one name: which line is whose is not told by the name)
    assert [ln for ln in got if not ln.startswith(plain)] == [ln for ln in want if not ln.startswith(plain)]
    assert len(got) == len(want)


def test_refusals(engine):
    rd, names = pc.reads()[:8], [n for n, _ in pc.contigs()]
    refs = [s for _, s in pc.contigs()]
    kw = dict(opt=mm.map_opt_sr(host_threads=2), k=pc.K, frags=mm.frag_offsets([n for n, _ in rd]))
    for call in (lambda **k: mm.map_reads(engine, pc.index(), names, rd, **k), lambda **k: mm.map_reads_stream([engine], pc.index(), names, rd, **k)):
        with pytest.raises(mm.Mm2gbError, match="paired ends with base-level alignment"):
            call(align=mm.map_sr(refs=refs, align=True), **kw)
        with pytest.raises(mm.Mm2gbError, match="SAM output and MM_F_EQX are not supported for fragments"):
            call(align=mm.map_sr(), out=mm.map_out(sam=True), **kw)
        with pytest.raises(mm.Mm2gbError, match="pe_ori is 0..3"):
            call(align=mm.map_sr(), pe_ori=4, **kw)
        with pytest.raises(mm.Mm2gbError, match="more than two reads"):
            call(align=mm.map_sr(), **dict(kw, frags=[0, 3, 8]))
        with pytest.raises(mm.Mm2gbError, match="frag_off does not run from 0 to n_reads"):
            call(align=mm.map_sr(), **dict(kw, frags=[0, 2, 4]))
        with pytest.raises(mm.Mm2gbError, match="frags= goes with align=map_sr"):
            call(**kw)
        with pytest.raises(mm.Mm2gbError, match="MM_F_RMQ"):                        # what the single-end call refuses stays refused
            call(align=mm.map_sr(), **dict(kw, opt=mm.map_opt_sr(flag=mm.map_opt_sr().flag | mm.F_RMQ)))


def test_batches_without_pairs_print_what_they_printed(engine):
    """Without frags= the committed short-read PAF as ever; and through the fragment call with every read a fragment of its own the same bytes, -c included."""
    for run in ("sr", "sr.f4_50", "sr.c"):
        want = sc.golden_paf(run)
        assert sc.map_run(engine, run)[0] == want
        _, opt_kw, sr_kw = sc.RUNS[run]
        if sr_kw.get("align"):
            sr_kw = dict(sr_kw, refs=[sc.gold()["genome"].encode()])
        rd = sc.reads()
        off = mm.frag_offsets([n for n, _ in rd])
        assert len(off) == len(rd) + 1
        for seeding in (0, 1):
            opt = mm.map_opt_sr(host_threads=4, seeding_on_device=seeding, **opt_kw)
            assert mm.map_reads(engine, sc.index(), ["ref"], rd, opt=opt, k=21, align=mm.map_sr(**sr_kw), frags=off)[0] == want
            assert mm.map_reads_stream([engine], sc.index(), ["ref"], rd, opt=opt, k=21, chunk_bases=5_000, align=mm.map_sr(**sr_kw), frags=off)[0] == want
