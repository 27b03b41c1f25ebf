"""The splice-aware DP's host form (mm2gb_ksw_exts2_host, csrc/ksw_host.cpp) against the reference's ksw_exts2_sse: the committed fixtures
everywhere, the compiled reference where oracle/_ref is built, and one named case per point at which ksw2_exts2_sse.c departs from the
dual-affine file.  Every comparison is exact: the result fields and every CIGAR word of every job."""
import numpy as np
import pytest

import ksw_cases as kc
import ksw_splice_cases as sc
import mm2gb_amd as mm

FOR, REV, FLANK, V = sc.FOR, sc.REV, sc.FLANK, sc.V
GT_AG, FULL, CT_AC, NONE = sc.MOTIFS


def test_host_equals_fixtures():
    """2 000 recorded jobs over the whole grid (tests/tools/gen_golden_ksw_splice.py wrote what the reference answered)."""
    n = n_words = 0
    for k, (p, jobs, q, t, junc, want) in enumerate(sc.golden_batches()):
        kc.assert_same(mm.ksw_exts2_host_batch(p, jobs, q, t, junc, threads=2), want, f"fixture set {k}", jobs)
        n += len(jobs)
        n_words += int(((want[1] & 0xf) == 3).sum())
    assert n >= 2000 and n_words >= 100


def test_threads_do_not_change_the_answer():
    p, jobs, q, t, junc, want = sc.golden_batches()[0]
    for threads in (1, 3, 16):
        kc.assert_same(mm.ksw_exts2_host_batch(p, jobs, q, t, junc, threads=threads), want, f"{threads} threads", jobs)


@pytest.mark.skipif(not kc.ref_available(), reason="the reference build (oracle/_ref) is not here")
def test_host_equals_reference_fuzz():
    """20 000 seeded jobs: mutated pairs and planted introns of 20..3 000 bases, lengths 1..257 around multiples of 16, every flag set, tuple,
    matrix and zdrop of ksw_splice_cases.  SCORE_ONLY jobs are held to the reference run without that flag."""
    rng = np.random.default_rng(2)
    n = 0
    for k, p in enumerate(sc.params()):
        jobs, q, t, junc = mm.ksw_splice_jobs(sc.make_batch(rng, p.m, 1000, sc.LENS_CPU, p_empty=0.02))
        kc.assert_same(mm.ksw_exts2_host_batch(p, jobs, q, t, junc, threads=4), sc.ref_batch(p, jobs, q, t, junc), f"parameter set {k}", jobs)
        n += len(jobs)
    assert n >= 20000


@pytest.mark.skipif(not kc.ref_available(), reason="the reference build (oracle/_ref) is not here")
def test_reference_answers_on_planted_inputs_meet_the_conditions():
    """Of the reference's own records for 2 000 planted jobs at the `splice` tuple, at least one in ten carries an N word, one in twenty is
    z-dropped and one in ten is a full-length CIGAR without N: a condition on the inputs, counted on the reference alone."""
    rng = np.random.default_rng(4)
    jobs, q, t, junc = mm.ksw_splice_jobs(sc.planted_batch(rng, 2000, sc.LENS_CPU))
    sh = sc.input_shares(jobs, *sc.ref_batch(sc.params()[0], jobs, q, t, junc))
    print(sh)
    sc.check_input_shares(sh)


@pytest.mark.skipif(not kc.ref_available(), reason="the reference build (oracle/_ref) is not here")
def test_reference_score_only_differs_from_its_cigar_loops():
    """The observation the SCORE_ONLY definition rests on: the compiled reference (SSE2-only) answers some SCORE_ONLY jobs with other scores
    than the same jobs without the flag; the host form gives the flag-less fields for both."""
    rng = np.random.default_rng(5)
    pairs = [(q, t, dict(o, flag=(o["flag"] | sc.S) & ~(sc.A | sc.X))) for q, t, o in sc.planted_batch(rng, 300, sc.LENS_CPU)]
    jobs, q, t, junc = mm.ksw_splice_jobs(pairs)
    p = sc.params()[0]
    as_is, without = sc.ref_batch(p, jobs, q, t, junc, score_only_as_is=True), sc.ref_batch(p, jobs, q, t, junc)
    assert (as_is[0]["score"] != without[0]["score"]).sum() > 0
    kc.assert_same(mm.ksw_exts2_host_batch(p, jobs, q, t, junc), without, "SCORE_ONLY", jobs)


def test_score_only_equals_the_same_job_without_the_flag():
    rng = np.random.default_rng(6)
    pairs = sc.make_batch(rng, 5, 300, sc.LENS_CPU, flags=[f for f in sc.FLAGS if not f & sc.S])
    jobs, q, t, junc = mm.ksw_splice_jobs(pairs)
    so = jobs.copy()
    so["flag"] |= sc.S
    a, b = mm.ksw_exts2_host_batch(sc.params()[0], jobs, q, t, junc)[0], mm.ksw_exts2_host_batch(sc.params()[0], so, q, t, junc)
    assert len(b[1]) == 0 and not b[0]["n_cigar"].any()
    for k in mm.KSW_FIELDS[:10]:
        assert np.array_equal(a[k], b[0][k]), k


def _one(qlen=20, tlen=20):
    return kc.make_pair(np.random.default_rng(3), 5, tlen, qlen, err=0.1)


def test_refusals():
    q, t = _one()
    for bit, name in ((0x20, "0x20"), (0x800, "unknown flag bits 2048")):
        with pytest.raises(mm.Mm2gbError, match=name):
            mm.ksw_exts2_host([(q, t)], flag=bit | FOR)
    bad = q.copy()
    bad[7] = 5
    with pytest.raises(mm.Mm2gbError, match="query residue >= m at 7"):
        mm.ksw_exts2_host([(q, t), (bad, t)])
    with pytest.raises(mm.Mm2gbError, match="target residue >= m"):
        mm.ksw_exts2_host([(q, bad)])
    with pytest.raises(mm.Mm2gbError, match="MM2GB_KSW_MAX_CELLS"):
        mm.ksw_exts2_host([(q, t), (np.zeros(10001, np.uint8), np.zeros(10000, np.uint8))], flag=mm.KSW_SCORE_ONLY)
    six = mm.ksw_splice_param()
    six.m = 6
    with pytest.raises(mm.Mm2gbError, match="m must be"):
        mm.ksw_exts2_host([(q, t)], param=six)
    for kw, text in ((dict(e=0), "e must be above 0"), (dict(e=-1), "e must be above 0"), (dict(q=-1), "q and q2 must not be negative"), (dict(q2=-3), "q and q2 must not be negative"),
                     (dict(q=100, e=28), "q \\+ e exceeds 127"), (dict(noncan=-1), "noncan must be 0..127"), (dict(junc_bonus=-2), "junc_bonus must be 0..127")):
        with pytest.raises(mm.Mm2gbError, match=text):
            mm.ksw_exts2_host([(q, t)], param=mm.ksw_splice_param(**kw))
    jobs, qs, ts, _ = mm.ksw_splice_jobs([(q, t)])
    jobs["tlen"] = -1
    with pytest.raises(mm.Mm2gbError, match="negative length or offset"):
        mm.ksw_exts2_host_batch(mm.ksw_splice_param(), jobs, qs, ts)
    with pytest.raises(mm.Mm2gbError, match="null argument"):
        mm._check(mm.lib().mm2gb_ksw_exts2_host(None, 0, None, None, None, None, 1, None, None, None))


RESET = dict(max=0, zdropped=0, max_q=-1, max_t=-1, mqe=mm.KSW_NEG_INF, mqe_t=-1, mte=mm.KSW_NEG_INF, mte_q=-1, score=mm.KSW_NEG_INF, reach_end=0, n_cigar=0)


def test_early_returns_give_the_reset_record():
    q, t = _one()
    empty = np.zeros(0, np.uint8)
    cases = [([(empty, t), (q, empty), (empty, empty)], None),
             ([(q, t)], mm.ksw_splice_param(q=2, e=1, q2=3)),                  # q2 <= q + e
             ([(q, t)], mm.ksw_splice_param(a=1, b=7)),                        # -min(mat) = 7 > 2 (q + e) = 6
             ([(q % 1, t % 1)], mm.ksw_splice_param(m=1, mat=[1]))]
    for pairs, prm in cases:
        for r in mm.ksw_exts2_host(pairs, param=prm, flag=FOR):
            assert {k: r[k] for k in RESET} == RESET and len(r["cigar"]) == 0
    assert mm.ksw_exts2_host([(q, t)], param=mm.ksw_splice_param(q=2, e=1, q2=4))[0]["score"] > mm.KSW_NEG_INF
    assert mm.ksw_exts2_host([(q, t)], param=mm.ksw_splice_param(a=1, b=6))[0]["score"] > mm.KSW_NEG_INF


def test_e_is_checked_before_the_early_return():
    """The reference tests q2 <= q + e before it divides by e, so (q, e, q2) = (5, 0, 3) would return at once there; here e <= 0 is an error
    whatever q2 is, and also for an empty batch."""
    q, t = _one()
    for pairs in ([(q, t)], []):
        with pytest.raises(mm.Mm2gbError, match="e must be above 0"):
            mm.ksw_exts2_host(pairs, param=mm.ksw_splice_param(q=5, e=0, q2=3))


# ---- one named case per point of DESIGN 6d-b's list.  Exons are error-free, so every expected score is the sum of its parts:
#      1 per exon base, q2 = 32 for the intron, noncan = 9 per site without a signal, junc_bonus = 9 per annotated site. ----
def _planted(motif, len1=50, len2=70, intron=200, seed=11, bits=None, fill=None):
    """Exons and intron over {A, T}, which spell no signal of either strand, so the only sites are the planted ones; fill: the intron is that
    one residue instead.  The bases beside the junction differ from those at the intron's other end, so it cannot slide."""
    rng = np.random.default_rng(seed)
    e1, mid, e2 = (rng.choice(np.array([0, 3], np.uint8), n) for n in (len1, intron, len2))
    if fill is not None:
        mid[:] = fill
    head, tail = motif
    if len(head):
        mid[:len(head)], mid[intron - len(tail):] = head, tail
    e1[-1] = 3 if mid[-1] == 0 else 0
    e2[0] = 3 if mid[0] == 0 else 0
    t, q = np.concatenate([e1, mid, e2]), np.concatenate([e1, e2])
    junc = None
    if bits:
        junc = np.zeros(len(t), np.uint8)
        junc[len1], junc[len1 + intron - 1] = bits
    return q, t, junc


def _run(q, t, junc=None, flag=0, param=None, zdrop=-1):
    r = mm.ksw_exts2_host([(q, t, dict(junc=junc))], param=param, flag=flag, zdrop=zdrop)[0]
    return r, mm.cigar_string(r["cigar"])


def test_trap_long_gap_goes_on_against_donor_not_zero():
    """Without a signal donor[] is -noncan everywhere, and the long gap's state goes on where a2 beats THAT: tested against 0 the state would
    end after one base and the intron would not come out as one N."""
    q, t, _ = _planted(NONE)
    for flag in (FOR, FOR | mm.KSW_RIGHT, FOR | REV | mm.KSW_APPROX_MAX):
        r, cig = _run(q, t, flag=flag)
        assert (r["score"], cig) == (120 - 32 - 18, "50M200N70M"), (flag, r, cig)
    r, cig = _run(q, t, flag=0)                      # no sites asked for: donor[] = acceptor[] = 0
    assert (r["score"], cig) == (120 - 32, "50M200N70M")


def test_trap_signals_and_flank():
    """GT..AG scores 0 at both ends with the flanking bases (GTr..yAG) or without SPLICE_FLANK, and -noncan / 2 = -4 an end with a bare GT..AG
    under SPLICE_FLANK; CT..AC is the reverse strand's and is seen only with SPLICE_REV."""
    bare = _planted(GT_AG)
    bare[1][50 + 2], bare[1][50 + 200 - 3] = 1, 0    # GTc ... aAG: neither flank
    for (q, t, _), flag, want in ((bare, FOR, 88), (bare, FOR | FLANK, 80), (_planted(FULL), FOR | FLANK, 88), (_planted(CT_AC), FOR, 70), (_planted(CT_AC), REV, 88),
                                  (_planted(CT_AC), FOR | REV, 88), (bare, REV, 70)):
        r, cig = _run(q, t, flag=flag)
        assert (r["score"], cig) == (want, "50M200N70M"), (flag, want, r, cig)


def test_trap_rev_cigar_mirrors_the_signals():
    """A left extension hands both sequences over reversed with REV_CIGAR: the signals are then looked for mirrored (GA..TG), and the words
    come out in the original's order."""
    q, t, _ = _planted(FULL)
    rq, rt = q[::-1].copy(), t[::-1].copy()
    r, cig = _run(rq, rt, flag=FOR | FLANK | V)
    assert (r["score"], cig) == (88, "50M200N70M")
    r, cig = _run(rq, rt, flag=FOR | FLANK)          # reversed but not said so: no signal is found
    assert (r["score"], cig) == (70, "70M200N50M")
    r, cig = _run(q, t, flag=FOR | FLANK | V)        # said so but not reversed
    assert (r["score"], cig) == (70, "70M200N50M")


def test_trap_junc_bits_per_orientation():
    """Bits 1 / 2 annotate a donor / acceptor for SPLICE_FOR, bits 8 / 4 for SPLICE_REV, each worth junc_bonus; reversed with REV_CIGAR the
    intron's first base is the one that carried the acceptor's bit."""
    for bits, flag, want in (((1, 2), FOR, 88), ((8, 4), FOR, 70), ((8, 4), REV, 88), ((1, 2), REV, 70), ((1, 0), FOR, 79), ((0, 4), REV, 79), ((2, 1), FOR, 70)):
        q, t, junc = _planted(NONE, bits=bits)
        r, cig = _run(q, t, junc, flag=flag)
        assert (r["score"], cig) == (want, "50M200N70M"), (bits, flag, r, cig)
        r, cig = _run(q[::-1].copy(), t[::-1].copy(), junc[::-1].copy(), flag=flag | V)
        assert (r["score"], cig) == (want, "50M200N70M"), ("mirrored", bits, flag, r, cig)


def test_trap_long_thres_boundary():
    """long_thres = 29 at (q, e, q2) = (2, 1, 32): a gap of 29 costs 31 as a short one, one of 30 costs 32 either way and is taken as the long
    one (a tie inside the matrix, settled by the gap alignment's side).  The long gap's state prints N; a leftover leading deletion of i + 1
    bases prints N from i = long_thres on."""
    assert [sc.long_thres(*x[:3]) for x in sc.TUPLES] == [29, 17, 9, 0, 1]
    for n, want_mid, want_right, want_lead in ((29, "29D", "29D", "29D"), (30, "30D", "30N", "30N"), (31, "31N", "31N", "31N")):
        q, t, _ = _planted(NONE, intron=n, fill=1)
        r, cig = _run(q, t)                          # at 30 both gaps cost 32: the short one wins the tie with gaps left-aligned ...
        assert cig == f"50M{want_mid}70M" and r["score"] == 120 - min(2 + n, 32), (n, r, cig)
        r, cig = _run(q, t, flag=mm.KSW_RIGHT)       # ... and the long one with gaps right-aligned
        assert cig == f"50M{want_right}70M" and r["score"] == 120 - min(2 + n, 32), (n, r, cig)
        r, cig = _run(q[50:], t[50:])                # the target begins n bases before the query's first: a leftover leading deletion
        assert cig == f"{want_lead}70M", (n, r, cig)
    q, t, _ = _planted(NONE, intron=30, fill=1)
    assert _run(q[50:], t[50 + 30 - 29:])[1] == "29D70M" and _run(q[50:], t[50:])[1] == "30N70M"
    # long_thres = 1: every target-side gap of two bases or more is the long one
    p1 = mm.ksw_splice_param(q=2, e=4, q2=7)
    assert _run(q[50:], t[50 + 29:], param=p1)[1] == "1D70M" and _run(q[50:], t[50 + 28:], param=p1)[1] == "2N70M"


def test_trap_zdrop_has_no_length_term():
    """The z-drop is taken with gap extension 0: a row's best cell 14 bases off the best cell's diagonal, 16 below it, ends the job at
    zdrop = 15, where the dual-affine form would have allowed 15 + 14 e."""
    rng = np.random.default_rng(12)
    E, F = rng.integers(0, 4, 50).astype(np.uint8), rng.integers(1, 4, 50).astype(np.uint8)
    E[-1] = 1                                        # the A's after it cannot slide left
    p = mm.ksw_splice_param(a=1, b=4)
    q = np.concatenate([E, F])
    gap = lambda n: np.concatenate([E, np.zeros(n, np.uint8), F])
    r, cig = _run(q, gap(20), param=p, zdrop=15)
    assert (r["zdropped"], r["max"], r["max_t"], r["max_q"], cig) == (1, 50, 49, 49, "50M"), (r, cig)
    r, cig = _run(q, gap(10), param=p, zdrop=15)
    assert (r["zdropped"], r["score"], cig) == (0, 100 - 12, "50M10D50M"), (r, cig)
    r, cig = _run(q, gap(20), param=p, zdrop=-1)
    assert (r["zdropped"], r["score"], cig) == (0, 100 - 22, "50M20D50M"), (r, cig)


def test_trap_wildcard_scores_minus_e():
    """A matrix whose wildcard entry is 0 scores the wildcard -e (the dual-affine form takes -e2)."""
    q = np.tile(np.arange(4, dtype=np.uint8), 10)
    t = q.copy()
    t[17] = 4
    for e in (1, 3):
        r, cig = _run(q, t, param=mm.ksw_splice_param(sc_ambi=0, q=2, e=e, q2=32))
        assert (r["score"], cig) == (39 - e, "40M")
    assert _run(q, t, param=mm.ksw_splice_param(sc_ambi=2))[0]["score"] == 39 - 2


def test_trap_no_cap_at_the_match_score():
    """ksw_exts2_sse does not clamp a cell at the match score as ksw_extd2_sse does: with an annotated site's bonus above the site's cost the
    cell after an intron gains more than a match, and the score says so."""
    q, t, junc = _planted(FULL, bits=(1, 2))
    r, cig = _run(q, t, junc, flag=FOR)
    assert (r["score"], cig) == (120 - 32 + 18, "50M200N70M")


def test_empty_batch_dicts_and_text():
    assert mm.ksw_exts2_host([]) == []
    q = np.array([0, 1, 2, 3, 0, 1, 2, 3], np.uint8)
    r = mm.ksw_exts2_host([(q, q)])[0]
    assert r["score"] == 8 and list(r["cigar"]) == [8 << 4] and r["zdropped"] == 0 and r["reach_end"] == 0
    assert mm.cigar_string([5 << 4, 200 << 4 | 3, 7 << 4]) == "5M200N7M"
    assert mm.ksw_splice_param().q2 == 32 and (mm.KSW_SPLICE_FOR, mm.KSW_SPLICE_REV, mm.KSW_SPLICE_FLANK) == (0x100, 0x200, 0x400)
