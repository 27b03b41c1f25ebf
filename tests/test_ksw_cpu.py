"""The extension DP's host form (mm2gb_ksw_extd2_host, csrc/ksw_host.cpp) against the reference's ksw_extd2_sse: the committed fixtures
everywhere, the compiled reference where oracle/_ref is built.  Every comparison is exact: eleven fields and every CIGAR word of every job."""
import numpy as np
import pytest

import ksw_cases as kc
import mm2gb_amd as mm


def test_host_equals_fixtures():
    """2 000 recorded jobs over the whole grid (tests/tools/gen_golden_ksw.py wrote what the reference answered)."""
    n = 0
    for k, (p, jobs, q, t, want) in enumerate(kc.golden_batches()):
        kc.assert_same(mm.ksw_extd2_host_batch(p, jobs, q, t, threads=2), want, f"fixture set {k}", jobs)
        n += len(jobs)
    assert n >= 2000


def test_threads_do_not_change_the_answer():
    p, jobs, q, t, want = kc.golden_batches()[0]
    for threads in (1, 3, 16):
        kc.assert_same(mm.ksw_extd2_host_batch(p, jobs, q, t, threads=threads), want, f"{threads} threads", jobs)


@pytest.mark.skipif(not kc.ref_available(), reason="the reference build (oracle/_ref) is not here")
def test_host_equals_reference_fuzz():
    """20 000 seeded jobs: lengths 1..257 around multiples of 16, every w, flag set, gap tuple, matrix, zdrop and end_bonus of ksw_cases.
    The reference's own answers on this set fall into the four outcome classes as 47.3 % z-dropped, 2.9 % reach_end, 25.4 % full CIGAR and
    24.4 % no CIGAR, counted on the reference's answers alone; each must stay above 2 %."""
    rng = np.random.default_rng(1)
    recs = []
    for k, p in enumerate(kc.params()):
        jobs, q, t = kc.make_batch(rng, p.m, 1000, kc.LENS_CPU, p_empty=0.02)
        want = kc.ref_batch(p, jobs, q, t)
        kc.assert_same(mm.ksw_extd2_host_batch(p, jobs, q, t, threads=4), want, f"parameter set {k}", jobs)
        recs.append(want[0])
    recs = np.concatenate(recs)
    assert len(recs) >= 20000
    sh = kc.shares(recs)
    print({k: round(float(v), 4) for k, v in sh.items()})
    assert all(v >= 0.02 for v in sh.values()), sh


def _one(qlen=20, tlen=20, flag=0, m=5):
    rng = np.random.default_rng(3)
    return kc.make_pair(rng, m, tlen, qlen, err=0.1)


def test_refusals():
    q, t = _one()
    for bit, name in ((0x100, "SPLICE_FOR"), (0x200, "SPLICE_REV"), (0x400, "SPLICE_FLANK"), (0x20, "0x20"), (0x800, "unknown")):
        with pytest.raises(mm.Mm2gbError, match=name):
            mm.ksw_extd2_host([(q, t)], flag=bit)
    bad = q.copy()
    bad[7] = 5
    with pytest.raises(mm.Mm2gbError, match="query residue >= m at 7"):
        mm.ksw_extd2_host([(q, t), (bad, t)])
    with pytest.raises(mm.Mm2gbError, match="target residue >= m"):
        mm.ksw_extd2_host([(q, bad)])
    # an oversized job is refused before anything is allocated: 10 001 x 10 000 cells
    big_q, big_t = np.zeros(10001, np.uint8), np.zeros(10000, np.uint8)
    with pytest.raises(mm.Mm2gbError, match="MM2GB_KSW_MAX_CELLS"):
        mm.ksw_extd2_host([(q, t), (big_q, big_t)], flag=mm.KSW_SCORE_ONLY)
    six = mm.ksw_param()
    six.m = 6
    with pytest.raises(mm.Mm2gbError, match="m must be"):
        mm.ksw_extd2_host([(q, t)], param=six)


RESET = dict(max=0, zdropped=0, max_q=-1, max_t=-1, mqe=mm.KSW_NEG_INF, mqe_t=-1, mte=mm.KSW_NEG_INF, mte_q=-1, score=mm.KSW_NEG_INF, reach_end=0, n_cigar=0)


def test_early_returns_give_the_reset_record():
    q, t = _one()
    empty = np.zeros(0, np.uint8)
    dear = mm.ksw_param(q=4, e=2, q2=24, e2=1, a=1, b=13)          # -min(mat) = 13 > 2 (q + e) = 12
    dear_swapped = mm.ksw_param(q=24, e=1, q2=4, e2=2, a=1, b=13)  # ... after the tuple has been put in order
    one_code = mm.ksw_param(m=1, mat=[1])
    cases = [([(empty, t), (q, empty), (empty, empty)], None), ([(q, t)], dear), ([(q, t)], dear_swapped), ([(q % 1, t % 1)], one_code)]
    for pairs, prm in cases:
        for r in mm.ksw_extd2_host(pairs, param=prm):
            assert {k: r[k] for k in RESET} == RESET and len(r["cigar"]) == 0
    # and the same tuple with a mismatch it can afford runs
    assert mm.ksw_extd2_host([(q, t)], param=mm.ksw_param(q=4, e=2, q2=24, e2=1, a=1, b=12))[0]["score"] > mm.KSW_NEG_INF


def test_first_cell_uses_the_gap_tuple_as_given():
    """(q, e, q2, e2) = (24, 1, 4, 2) and (4, 2, 24, 1) are the same penalties, but H at the first cell is taken before the tuple is put in
    order: every score of the first is 19 below the second's."""
    q, t = _one(40, 40)
    a = mm.ksw_extd2_host([(q, t)], param=mm.ksw_param(q=4, e=2, q2=24, e2=1))[0]
    b = mm.ksw_extd2_host([(q, t)], param=mm.ksw_param(q=24, e=1, q2=4, e2=2))[0]
    assert a["score"] - b["score"] == 19 and np.array_equal(a["cigar"], b["cigar"])


def test_empty_batch_and_dicts():
    assert mm.ksw_extd2_host([]) == []
    q = np.array([0, 1, 2, 3, 0, 1, 2, 3], np.uint8)
    r = mm.ksw_extd2_host([(q, q)], w=-1)[0]
    assert r["score"] == 16 and list(r["cigar"]) == [8 << 4] and r["zdropped"] == 0
