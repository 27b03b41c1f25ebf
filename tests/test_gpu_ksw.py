"""The extension DP's device form (mm2gb_ksw_extd2_gpu, csrc/ksw_kernels.hip) against the host form, the committed fixtures and, where
oracle/_ref is built, the reference's ksw_extd2_sse.  Every comparison is exact: eleven fields and every CIGAR word of every job."""
import os

import numpy as np
import pytest

import ksw_cases as kc
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
    host = mm.ksw_extd2_host_batch(p, jobs, q, t, threads=8)
    got = eng.ksw_extd2_batch(p, jobs, q, t)
    kc.assert_same(got, host, what + ": device against host", jobs)
    if reference and kc.ref_available():
        kc.assert_same(got, kc.ref_batch(p, jobs, q, t), what + ": device against the reference", jobs)
    return got


def test_mixed_batch_equals_host(eng):
    """20 000 jobs in one call at the map-ont scores, then every other gap tuple and matrix with 500 each: lengths around multiples of 16
    up to 257, wildcards, every w / flag set / zdrop / end_bonus of the grid, empty jobs and jobs the reference returns from at once mixed
    in, neighbours of different sizes."""
    rng = np.random.default_rng(11)
    sets = kc.params()
    jobs, q, t = shuffled(rng, kc.make_batch(rng, sets[0].m, 20000, kc.LENS_GPU, p_empty=0.02))
    kc.assert_same(eng.ksw_extd2_batch(sets[0], jobs, q, t), mm.ksw_extd2_host_batch(sets[0], jobs, q, t, threads=16), "20 000 mixed jobs", jobs)
    for k, p in enumerate(sets[1:], 1):
        jobs, q, t = shuffled(rng, kc.make_batch(rng, p.m, 500, kc.LENS_GPU, p_empty=0.02))
        kc.assert_same(eng.ksw_extd2_batch(p, jobs, q, t), mm.ksw_extd2_host_batch(p, jobs, q, t, threads=16), f"parameter set {k}", jobs)


def test_device_equals_fixtures(eng):
    for k, (p, jobs, q, t, want) in enumerate(kc.golden_batches()):
        kc.assert_same(eng.ksw_extd2_batch(p, jobs, q, t), want, f"fixture set {k}", jobs)


def test_kernel_seams(eng):
    """One job either side of every boundary the kernel has: the band widths at which a workgroup gets more threads (a job's class goes by
    its row of direction bytes, ((min(qlen, tlen, w + 1) + 15) / 16 + 1) * 16 cells), the image sizes at which a launch asks for more
    LDS, and the largest image LDS holds."""
    info = eng.ksw_info()
    rng = np.random.default_rng(5)
    p = mm.ksw_param()
    pairs = []
    for band in info["band"] + [info["nt"][2]]:          # widest band of a class: min(...) = band - 16
        for n in (band - 16, band - 15):
            for flag in (0, A | R, X | V):
                q, t = kc.make_pair(rng, 5, 700, 690, err=0.1)
                pairs.append((q, t, dict(w=n - 1, zdrop=200, end_bonus=5, flag=flag)))
    for lds in (8 << 10, 32 << 10, 64 << 10, info["lds_max"]):            # image: 16 T + Q with H, 12 T + Q without (T, Q rounded to 16)
        for flag, per_t in ((0, 16), (A, 12)):
            square = lds // (per_t + 1) <= 6000                           # else a 6 000-base query: the job stays below the cell limit
            fit = lds // (per_t + 1) // 16 * 16 if square else (lds - 6000) // per_t // 16 * 16
            for tlen in (fit, fit + 16):
                q, t = kc.make_pair(rng, 5, tlen, tlen if square else 6000, err=0.05)
                pairs.append((q, t, dict(w=20, zdrop=-1, end_bonus=0, flag=flag if square else flag | X)))
    check(eng, p, *mm.ksw_jobs(pairs), "seams")


def test_large_shapes(eng):
    """An image that does not fit LDS (10 050 x 9 950, w 100: 16 x 10 064 + 9 952 bytes with H; the cell limit of 10^8 rules out the
    20 000 x 19 500 the shape was first thought of at), a wide band with a drop (3 000 x 3 000, w 500, zdrop 400), and the one-base shapes."""
    rng = np.random.default_rng(6)
    p = mm.ksw_param()
    big = kc.make_pair(rng, 5, 10050, 9950, err=0.05)
    sq = kc.make_pair(rng, 5, 3000, 3000, err=0.1)
    one = np.array([2], np.uint8)
    long = rng.integers(0, 4, 5000).astype(np.uint8)
    pairs = [big + (dict(w=100, flag=0),), big + (dict(w=100, flag=A | D | X, zdrop=400),), sq + (dict(w=500, zdrop=400, flag=X),), sq + (dict(w=500, zdrop=400, flag=R),),
             (one, long, dict(flag=0)), (long, one, dict(flag=0)), (one, long, dict(flag=X, w=10)), (long, one, dict(flag=X | R))]
    batch = mm.ksw_jobs(pairs)
    assert 16 * 10064 + 9952 > eng.ksw_info()["lds_max"]
    got = check(eng, p, *batch, "large shapes")
    assert got[0]["n_cigar"][0] > 0 and got[0]["zdropped"][0] == 0


def test_one_job_and_none(eng):
    rng = np.random.default_rng(8)
    p = mm.ksw_param()
    q, t = kc.make_pair(rng, 5, 100, 90, err=0.1)
    check(eng, p, *mm.ksw_jobs([(q, t)], w=30, zdrop=100), "one job")
    assert eng.ksw_extd2([], param=p) == []
    res, words = eng.ksw_extd2_batch(p, *mm.ksw_jobs([(np.zeros(0, np.uint8), t)]))
    assert len(res) == 1 and res["score"][0] == mm.KSW_NEG_INF and len(words) == 0
    r = eng.ksw_extd2([(q, t)], w=30)[0]
    assert sorted(r) == sorted(mm.KSW_FIELDS + ("cigar",)) and r["cigar"].dtype == np.uint32


def test_arenas_are_reused(eng):
    """The same batch before and after a larger one on the same engine: identical bytes."""
    rng = np.random.default_rng(9)
    p = kc.params()[0]
    small = kc.make_batch(rng, p.m, 300, kc.LENS_GPU, p_empty=0.02)
    large = kc.make_batch(rng, p.m, 3000, kc.LENS_GPU + [400, 700])
    first = eng.ksw_extd2_batch(p, *small)
    kc.assert_same(eng.ksw_extd2_batch(p, *large), mm.ksw_extd2_host_batch(p, *large, threads=8), "the larger batch", large[0])
    again = eng.ksw_extd2_batch(p, *small)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
    kc.assert_same(first, mm.ksw_extd2_host_batch(p, *small), "the small batch", small[0])


def test_several_launches(eng):
    """A slab budget of 1 MiB cuts a batch whose direction bytes need more into several launches; the answers do not change."""
    rng = np.random.default_rng(10)
    p = mm.ksw_param()
    batch = kc.make_batch(rng, p.m, 400, [257, 400, 129])
    os.environ["MM2GB_KSW_SLAB_MB"] = "1"
    try:
        got = eng.ksw_extd2_batch(p, *batch)
    finally:
        del os.environ["MM2GB_KSW_SLAB_MB"]
    kc.assert_same(got, mm.ksw_extd2_host_batch(p, *batch), "1 MiB of direction bytes per launch", batch[0])


def test_device_refuses_what_the_host_refuses(eng):
    q = np.zeros(10, np.uint8)
    with pytest.raises(mm.Mm2gbError, match="SPLICE_FOR"):
        eng.ksw_extd2([(q, q)], flag=0x100)
    with pytest.raises(mm.Mm2gbError, match="residue >= m"):
        eng.ksw_extd2([(q + 5, q)])
    with pytest.raises(mm.Mm2gbError, match="MM2GB_KSW_MAX_CELLS"):
        eng.ksw_extd2([(np.zeros(10001, np.uint8), np.zeros(10000, np.uint8))])
