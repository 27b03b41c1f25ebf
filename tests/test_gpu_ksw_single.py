"""The single-affine DP's device form (mm2gb_ksw_extz2_gpu: k_ksw's third form, csrc/ksw_kernels.hip) against the host form, the committed
fixtures and, where oracle/_ref is built, the reference's ksw_extz2_sse.  Every comparison is exact: eleven fields and every CIGAR word."""
import os

import numpy as np
import pytest

import ksw_cases as kc
import ksw_single_cases as ks
import ksw_splice_cases as sc
import mm2gb_amd as mm

pytestmark = pytest.mark.gpu
X, A, D, R, V, S = mm.KSW_EXTZ_ONLY, mm.KSW_APPROX_MAX, mm.KSW_APPROX_DROP, mm.KSW_RIGHT, mm.KSW_REV_CIGAR, mm.KSW_SCORE_ONLY


@pytest.fixture(scope="module")
def eng():
    with mm.Engine(device=0) as e:
        yield e


def shuffled(rng, batch):
    jobs, q, t = batch
    return jobs[rng.permutation(len(jobs))], q, t


def check(eng, p, jobs, q, t, what, reference=True):
    host = mm.ksw_extz2_host_batch(p, jobs, q, t, threads=16)
    got = eng.ksw_extz2_batch(p, jobs, q, t)
    kc.assert_same(got, host, what + ": device against host", jobs)
    if reference and kc.ref_available():
        kc.assert_same(got, ks.ref_batch(p, jobs, q, t), what + ": device against the reference", jobs)
    return got


def test_mixed_batch_equals_host(eng):
    """20 000 jobs in one call at (4, 2) with the map-ont matrix, then every other (q, e) and matrix with 500 each: lengths around multiples
    of 16 up to 257, wildcards, every w / flag set / zdrop / end_bonus of the grid, empty jobs and jobs the reference returns from at once
    mixed in, neighbours of different sizes."""
    rng = np.random.default_rng(11)
    sets = ks.params()
    jobs, q, t = shuffled(rng, kc.make_batch(rng, sets[0].m, 20000, kc.LENS_GPU, p_empty=0.02))
    kc.assert_same(eng.ksw_extz2_batch(sets[0], jobs, q, t), mm.ksw_extz2_host_batch(sets[0], jobs, q, t, threads=16), "20 000 mixed jobs", jobs)
    for k, p in enumerate(sets[1:], 1):
        jobs, q, t = shuffled(rng, kc.make_batch(rng, p.m, 500, kc.LENS_GPU, p_empty=0.02))
        kc.assert_same(eng.ksw_extz2_batch(p, jobs, q, t), mm.ksw_extz2_host_batch(p, jobs, q, t, threads=16), f"parameter set {k}", jobs)


def test_device_equals_fixtures(eng):
    for traps in (False, True):
        for k, (p, jobs, q, t, want) in enumerate(ks.golden_batches(traps=traps)):
            kc.assert_same(eng.ksw_extz2_batch(p, jobs, q, t), want, f"fixture set {k}" if not traps else "trap " + ks.TRAPS[k], jobs)


def test_kernel_seams(eng):
    """One job either side of every boundary the kernel has, with this form's numbers: the band widths at which a workgroup gets more
    threads, the image sizes at which a launch asks for more LDS -- 13 T + Q bytes with H, 9 T + Q without (T, Q rounded to 16) -- and the
    largest image LDS holds."""
    info = eng.ksw_info()
    rng = np.random.default_rng(5)
    p = ks.param()
    pairs = []
    for band in info["band"] + [info["nt"][2]]:          # widest band of a class: min(...) = band - 16
        for n in (band - 16, band - 15):
            for flag in (0, A | R, X | V):
                q, t = kc.make_pair(rng, 5, 700, 690, err=0.1)
                pairs.append((q, t, dict(w=n - 1, zdrop=200, end_bonus=5, flag=flag)))
    for lds in (8 << 10, 32 << 10, 64 << 10, info["lds_max"]):
        for flag, per_t in ((0, 13), (A, 9)):
            square = lds // (per_t + 1) <= 5600                           # else a 5 600-base query: 17 472 x 5 600 stays below the cell limit
            fit = lds // (per_t + 1) // 16 * 16 if square else (lds - 5600) // per_t // 16 * 16
            for tlen in (fit, fit + 16):
                q, t = kc.make_pair(rng, 5, tlen, tlen if square else 5600, err=0.05)
                assert (per_t * tlen + (tlen if square else 5600) <= lds) == (tlen == fit)
                pairs.append((q, t, dict(w=20, zdrop=-1, end_bonus=0, flag=flag if square else flag | X)))
    before = eng.ksw_class_jobs()
    check(eng, p, *mm.ksw_jobs(pairs), "seams")
    after = eng.ksw_class_jobs()
    assert after[1] - before[1] == 2, "one job of each kind lies beyond the largest image LDS holds"


def test_large_shapes(eng):
    """An image that lives in global memory (14 000 x 7 000 at w 100 with H: 13 x 14 000 + 7 008 bytes, 9.8 x 10^7 cells, under the cell
    limit), a wide band with a drop (3 000 x 3 000, w 500, zdrop 400), and the one-base shapes."""
    rng = np.random.default_rng(6)
    p = ks.param()
    big = kc.make_pair(rng, 5, 14000, 14000, err=0.05)
    big = (big[0][:7000].copy(), big[1])                 # the query ends half way: the band runs empty there, and the job walks from its best cell
    sq = kc.make_pair(rng, 5, 3000, 3000, err=0.1)
    sq[0][1500:2400] = rng.integers(0, 4, 900)          # unrelated sequence in the middle: the drop
    one = np.array([2], np.uint8)
    long = rng.integers(0, 4, 5000).astype(np.uint8)
    pairs = [big + (dict(w=100, flag=X),), big + (dict(w=100, flag=A | D | X, zdrop=400),), sq + (dict(w=500, zdrop=400, flag=X),), sq + (dict(w=500, zdrop=400, flag=R),),
             (one, long, dict(flag=0)), (long, one, dict(flag=0)), (one, long, dict(flag=X, w=10)), (long, one, dict(flag=X | R))]
    batch = mm.ksw_jobs(pairs)
    assert 13 * 14000 + 7008 > eng.ksw_info()["lds_max"]
    before = eng.ksw_class_jobs()
    got = check(eng, p, *batch, "large shapes")
    assert eng.ksw_class_jobs()[1] - before[1] == 1          # without H the same job fits: 9 x 14 000 + 7 008
    assert got[0]["n_cigar"][0] > 0 and got[0]["zdropped"][0] == 1 and got[0]["max_q"][0] > 6000
    assert got[0]["zdropped"][2] == 1 and got[0]["zdropped"][3] == 1


def test_one_job_and_none(eng):
    rng = np.random.default_rng(8)
    p = ks.param()
    q, t = kc.make_pair(rng, 5, 100, 90, err=0.1)
    check(eng, p, *mm.ksw_jobs([(q, t)], w=30, zdrop=100), "one job")
    assert eng.ksw_extz2([], param=p) == []
    res, words = eng.ksw_extz2_batch(p, *mm.ksw_jobs([(np.zeros(0, np.uint8), t)]))
    assert len(res) == 1 and res["score"][0] == mm.KSW_NEG_INF and len(words) == 0
    r = eng.ksw_extz2([(q, t)], param=p, w=30)[0]
    assert sorted(r) == sorted(mm.KSW_FIELDS + ("cigar",)) and r["cigar"].dtype == np.uint32


def test_forms_take_turns(eng):
    """A dual-affine batch, a single-affine one, a splice-aware one, and the first again on one engine: each equals its host form, and the
    first gives identical bytes the second time."""
    rng = np.random.default_rng(9)
    pd, ps_ = kc.params()[0], ks.params()[0]
    dual = kc.make_batch(rng, pd.m, 600, kc.LENS_GPU, p_empty=0.02)
    single = kc.make_batch(rng, ps_.m, 600, kc.LENS_GPU + [400], p_empty=0.02)
    psp, sj, sq, st, sjunc, swant = sc.golden_batches()[0]
    first = eng.ksw_extd2_batch(pd, *dual)
    kc.assert_same(eng.ksw_extz2_batch(ps_, *single), mm.ksw_extz2_host_batch(ps_, *single, threads=16), "single after dual", single[0])
    kc.assert_same(eng.ksw_exts2_batch(psp, sj, sq, st, sjunc), swant, "splice after single", sj)
    again = eng.ksw_extd2_batch(pd, *dual)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
    kc.assert_same(first, mm.ksw_extd2_host_batch(pd, *dual, threads=16), "dual", dual[0])
    # the same jobs under both gap models on one engine: (4, 2, 4, 2) through the dual-affine kernel is not this DP
    kc.assert_same(eng.ksw_extz2_batch(ps_, *dual), mm.ksw_extz2_host_batch(ps_, *dual, threads=16), "single on the dual batch", dual[0])


def test_several_launches(eng):
    """A slab budget of 1 MiB cuts a batch whose direction bytes need more into several launches; the answers do not change."""
    rng = np.random.default_rng(10)
    p = ks.param()
    batch = kc.make_batch(rng, p.m, 400, [257, 400, 129])
    os.environ["MM2GB_KSW_SLAB_MB"] = "1"
    try:
        got = eng.ksw_extz2_batch(p, *batch)
    finally:
        del os.environ["MM2GB_KSW_SLAB_MB"]
    kc.assert_same(got, mm.ksw_extz2_host_batch(p, *batch), "1 MiB of direction bytes per launch", batch[0])


def test_device_refuses_what_the_host_refuses(eng):
    q = np.zeros(10, np.uint8)
    with pytest.raises(mm.Mm2gbError, match="mm2gb_ksw_extz2_gpu: job 0: flag KSW_EZ_SPLICE_FOR"):
        eng.ksw_extz2([(q, q)], flag=0x100)
    with pytest.raises(mm.Mm2gbError, match="residue >= m"):
        eng.ksw_extz2([(q + 5, q)])
    with pytest.raises(mm.Mm2gbError, match="MM2GB_KSW_MAX_CELLS"):
        eng.ksw_extz2([(np.zeros(10001, np.uint8), np.zeros(10000, np.uint8))])
    with pytest.raises(mm.Mm2gbError, match="mm2gb_ksw_extz2_gpu: q and e must be above 0"):
        eng.ksw_extz2([(q, q)], param=ks.param(4, 0))
    with pytest.raises(mm.Mm2gbError, match=r"mm2gb_ksw_extz2_gpu: 2 \* \(q \+ e\) exceeds 127"):
        eng.ksw_extz2([(q, q)], param=ks.param(61, 3))
