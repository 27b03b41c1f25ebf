"""The single-affine extension DP's host form (mm2gb_ksw_extz2_host, csrc/ksw_host.cpp) against the reference's ksw_extz2_sse: the committed
fixtures everywhere, the compiled reference where oracle/_ref is built.  Every comparison is exact: eleven fields and every CIGAR word."""
import numpy as np
import pytest

import ksw_cases as kc
import ksw_single_cases as ks
import mm2gb_amd as mm

RESET = dict(max=0, zdropped=0, max_q=-1, max_t=-1, mqe=mm.KSW_NEG_INF, mqe_t=-1, mte=mm.KSW_NEG_INF, mte_q=-1, score=mm.KSW_NEG_INF, reach_end=0, n_cigar=0)


def _is_reset(rec):
    return all(int(rec[k]) == v for k, v in RESET.items())


def test_host_equals_fixtures():
    """2 000 recorded jobs over the whole grid (tests/tools/gen_golden_ksw_single.py wrote what the reference answered)."""
    n = 0
    for k, (p, jobs, q, t, want) in enumerate(ks.golden_batches()):
        kc.assert_same(mm.ksw_extz2_host_batch(p, jobs, q, t, threads=2), want, f"fixture set {k}", jobs)
        n += len(jobs)
    assert n >= 2000


def test_thread_counts_give_identical_bytes():
    p, jobs, q, t, want = ks.golden_batches()[0]
    one, many = mm.ksw_extz2_host_batch(p, jobs, q, t, threads=1), mm.ksw_extz2_host_batch(p, jobs, q, t, threads=16)
    assert one[0].tobytes() == many[0].tobytes() and one[1].tobytes() == many[1].tobytes()
    kc.assert_same(one, want, "1 thread", jobs)


@pytest.mark.skipif(not kc.ref_available(), reason="the reference build (oracle/_ref) is not here")
def test_host_equals_reference_fuzz():
    """20 000 seeded jobs: lengths 1..257 around multiples of 16, every w, flag set, matrix, zdrop and end_bonus of ksw_cases, (q, e) from
    ksw_single_cases.GAPS.  The reference's own answers on this set fall into the four outcome classes as 50.0 % z-dropped, 3.0 % reach_end,
    27.2 % full CIGAR and 19.9 % no CIGAR, counted on the reference's answers alone; each must stay at or above 1 %."""
    rng = np.random.default_rng(1)
    recs = []
    for k, p in enumerate(ks.params()):
        jobs, q, t = kc.make_batch(rng, p.m, 1000, kc.LENS_CPU, p_empty=0.02)
        want = ks.ref_batch(p, jobs, q, t)
        kc.assert_same(mm.ksw_extz2_host_batch(p, jobs, q, t, threads=4), want, f"parameter set {k}", jobs)
        recs.append(want[0])
    recs = np.concatenate(recs)
    assert len(recs) >= 20000
    sh = kc.shares(recs)
    print({k: round(float(v), 4) for k, v in sh.items()})
    assert all(v >= 0.01 for v in sh.values()), sh


def _trap(name):
    return ks.golden_batches(traps=True)[ks.TRAPS.index(name)]


@pytest.mark.parametrize("name", ks.TRAPS)
def test_trap_equals_fixture(name):
    """Each named trap as a recorded batch; live against the reference too where it is built (the batch is the generator's)."""
    p, jobs, q, t, want = _trap(name)
    got = mm.ksw_extz2_host_batch(p, jobs, q, t, threads=2)
    kc.assert_same(got, want, name, jobs)
    if kc.ref_available():
        p2, jobs2, q2, t2 = ks.trap_batches()[name]
        assert jobs2.tobytes() == jobs.tobytes() and q2.tobytes() == q.tobytes() and t2.tobytes() == t.tobytes(), "the fixture is not the generator's batch"
        kc.assert_same(got, ks.ref_batch(p2, jobs2, q2, t2), name + " (live)", jobs)


def test_trap_m1_is_no_early_return():
    """ksw_extz2_sse returns at m <= 0 only: with one residue code every pair scores the wildcard's mat[0], and the job runs.  The dual-affine
    DP returns at once on the same input."""
    p, jobs, q, t, want = _trap("m1")
    live = [k for k in range(len(jobs)) if jobs["qlen"][k] > 0 and jobs["tlen"][k] > 0]
    assert live and not any(_is_reset(want[0][k]) for k in live)
    assert all(_is_reset(r) for r in mm.ksw_extd2_host_batch(p, jobs, q, t)[0])
    z = np.zeros(8, np.uint8)
    r = mm.ksw_extz2_host([(z, z)], param=ks.param(4, 2, m=1, mat=[1]))[0]
    assert r["score"] == 8 and list(r["cigar"]) == [8 << 4]
    r = mm.ksw_extz2_host([(z, z)], param=ks.param(4, 2, m=1, mat=[0]))[0]          # mat[m * m - 1] == 0: the wildcard costs e
    assert r["score"] == -16
    assert _is_reset(mm.ksw_extz2_host_batch(ks.param(4, 2, m=0), *mm.ksw_jobs([(z, z)]))[0][0])


def test_trap_cap_above_127():
    """(q, e) = (39, 3) with a match of 45: the cap is 129 and a match's shifted score byte, 129 as well, reads as negative where the
    reference clamps z at 0 with a signed compare -- a perfect match does not score 45 a base."""
    p, jobs, q, t, want = _trap("cap")
    assert int(p.mat[0]) + 2 * (p.q + p.e) > 127
    s = np.array([0, 1, 2, 3] * 4, np.uint8)
    assert mm.ksw_extz2_host([(s, s)], param=p)[0]["score"] < 45 * 16
    assert mm.ksw_extz2_host([(s, s)], param=ks.param(39, 3, a=43, b=80))[0]["score"] == 43 * 16          # 43 + 84 = 127 still fits


def test_trap_min_of_matrix():
    """-min(mat) == 2(q + e) runs; one above returns the reset record, and so does it with m = 1, where the minimum is still mat[1]."""
    p, jobs, q, t, want = _trap("min_equal")
    live = (jobs["qlen"] > 0) & (jobs["tlen"] > 0)
    assert not any(_is_reset(r) for r in want[0][live])
    p, jobs, q, t, want = _trap("min_above")
    assert all(_is_reset(r) for r in want[0]) and len(want[1]) == 0
    z = np.zeros(8, np.uint8)
    assert _is_reset(mm.ksw_extz2_host_batch(ks.param(4, 2, m=1, mat=[1, -13]), *mm.ksw_jobs([(z, z)]))[0][0])
    assert not _is_reset(mm.ksw_extz2_host_batch(ks.param(4, 2, m=1, mat=[1, -12]), *mm.ksw_jobs([(z, z)]))[0][0])


def test_q2_and_e2_are_not_read():
    p, jobs, q, t, want = ks.golden_batches()[0]
    other = mm.ksw_param(q=p.q, e=p.e, q2=99, e2=-7, mat=list(p.mat), m=p.m)
    kc.assert_same(mm.ksw_extz2_host_batch(other, jobs, q, t), want, "q2 = 99, e2 = -7", jobs)


def test_refusals():
    rng = np.random.default_rng(3)
    q, t = kc.make_pair(rng, 5, 20, 20, err=0.1)
    for bit, name in ((0x100, "KSW_EZ_SPLICE_FOR"), (0x200, "KSW_EZ_SPLICE_REV"), (0x400, "KSW_EZ_SPLICE_FLANK"), (0x20, "0x20"), (0x800, "unknown flag bits")):
        with pytest.raises(mm.Mm2gbError, match="mm2gb_ksw_extz2_host: job 0: .*" + name):
            mm.ksw_extz2_host([(q, t)], flag=bit)
    bad = q.copy()
    bad[7] = 5
    with pytest.raises(mm.Mm2gbError, match="query residue >= m at 7"):
        mm.ksw_extz2_host([(q, t), (bad, t)])
    with pytest.raises(mm.Mm2gbError, match="target residue >= m"):
        mm.ksw_extz2_host([(q, bad)])
    with pytest.raises(mm.Mm2gbError, match="query residue >= m at 0"):          # m == 1 reads its residues here
        mm.ksw_extz2_host([(q % 2 + 1, t % 1)], param=ks.param(4, 2, m=1, mat=[1]))
    big_q, big_t = np.zeros(10001, np.uint8), np.zeros(10000, np.uint8)
    with pytest.raises(mm.Mm2gbError, match="MM2GB_KSW_MAX_CELLS"):
        mm.ksw_extz2_host([(q, t), (big_q, big_t)], flag=mm.KSW_SCORE_ONLY)
    six = ks.param()
    six.m = 6
    with pytest.raises(mm.Mm2gbError, match="m must be"):
        mm.ksw_extz2_host([(q, t)], param=six)
    for qq, ee in ((0, 2), (4, 0), (-1, 2), (4, -2)):
        with pytest.raises(mm.Mm2gbError, match="mm2gb_ksw_extz2_host: q and e must be above 0"):
            mm.ksw_extz2_host([(q, t)], param=ks.param(qq, ee))
    with pytest.raises(mm.Mm2gbError, match=r"mm2gb_ksw_extz2_host: 2 \* \(q \+ e\) exceeds 127"):
        mm.ksw_extz2_host([(q, t)], param=ks.param(61, 3))
    assert mm.ksw_extz2_host([(q, t)], param=ks.param(60, 3))[0]["score"] > mm.KSW_NEG_INF          # 126 passes


def test_empty_batch_and_dicts():
    assert mm.ksw_extz2_host([]) == []
    q = np.array([0, 1, 2, 3, 0, 1, 2, 3], np.uint8)
    r = mm.ksw_extz2_host([(q, q)], param=ks.param(), w=-1)[0]
    assert r["score"] == 16 and list(r["cigar"]) == [8 << 4] and r["zdropped"] == 0
    empty = np.zeros(0, np.uint8)
    for r in mm.ksw_extz2_host([(empty, q), (q, empty), (empty, empty)], param=ks.param()):
        assert {k: r[k] for k in RESET} == RESET and len(r["cigar"]) == 0
