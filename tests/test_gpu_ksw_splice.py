"""The splice-aware DP's device form (mm2gb_ksw_exts2_gpu, csrc/ksw_kernels.hip) against the host form, the committed fixtures and, where
oracle/_ref is built, the reference's ksw_exts2_sse.  Every comparison is exact: the result fields and every CIGAR word of every job."""
import os

import numpy as np
import pytest

import ksw_cases as kc
import ksw_splice_cases as sc
import mm2gb_amd as mm

pytestmark = pytest.mark.gpu
X, A, D, R, V, S = sc.X, sc.A, sc.D, sc.R, sc.V, sc.S
FOR, REV, FLANK = sc.FOR, sc.REV, sc.FLANK


@pytest.fixture(scope="module")
def eng():
    with mm.Engine(device=0) as e:
        yield e


def exactly(q, n):
    """q cut or repeated to n residues (a mutated query is a few bases off the length asked for)."""
    return q[:n].copy() if len(q) >= n else np.resize(q, n)


def batch_of(rng, m, n, lens, **kw):
    jobs, q, t, junc = mm.ksw_splice_jobs(sc.make_batch(rng, m, n, lens, **kw))
    return jobs[rng.permutation(len(jobs))], q, t, junc


def check(eng, p, jobs, q, t, junc, what, reference=True):
    host = mm.ksw_exts2_host_batch(p, jobs, q, t, junc, threads=16)
    got = eng.ksw_exts2_batch(p, jobs, q, t, junc)
    kc.assert_same(got, host, what + ": device against host", jobs)
    if reference and kc.ref_available():
        kc.assert_same(got, sc.ref_batch(p, jobs, q, t, junc), what + ": device against the reference", jobs)
    return got


def test_mixed_batch_equals_host(eng):
    """5 000 jobs in one call at the `splice` tuple, then every other tuple and matrix with 300 each: mutated pairs and planted introns,
    every flag set and zdrop of the grid, junc on some, empty jobs and early returns mixed in, neighbours of different sizes."""
    rng = np.random.default_rng(21)
    sets = sc.params()
    jobs, q, t, junc = batch_of(rng, sets[0].m, 5000, sc.LENS_GPU, p_empty=0.02, intron_hi=1000)
    got = eng.ksw_exts2_batch(sets[0], jobs, q, t, junc)
    kc.assert_same(got, mm.ksw_exts2_host_batch(sets[0], jobs, q, t, junc, threads=16), "5 000 mixed jobs", jobs)
    assert sc.has_N(*got).sum() >= 250
    for k, p in enumerate(sets[1:], 1):
        jobs, q, t, junc = batch_of(rng, p.m, 300, sc.LENS_GPU, p_empty=0.02, intron_hi=600)
        kc.assert_same(eng.ksw_exts2_batch(p, jobs, q, t, junc), mm.ksw_exts2_host_batch(p, jobs, q, t, junc, threads=16), f"parameter set {k}", jobs)


def test_device_equals_fixtures(eng):
    for k, (p, jobs, q, t, junc, want) in enumerate(sc.golden_batches()):
        kc.assert_same(eng.ksw_exts2_batch(p, jobs, q, t, junc), want, f"fixture set {k}", jobs)


def test_kernel_seams(eng):
    """One job either side of every boundary the kernel has: the row widths ((min(qlen, tlen) + 15) / 16 + 1) * 16 at which a workgroup gets
    more threads, the image sizes (17 T + Q bytes with H, 13 T + Q without; T, Q rounded to 16) at which a launch asks for more LDS, and the
    largest image LDS holds."""
    info = eng.ksw_info()
    rng = np.random.default_rng(22)
    p = mm.ksw_splice_param()
    pairs = []
    for band in info["band"] + [info["nt"][2]]:
        for n in (band - 16, band - 15):                                  # min(qlen, tlen) = n: the row is band, band + 16 cells
            for flag in (FOR, FOR | A | R, FOR | REV | X | V):
                q, t, junc = sc.make_intron_pair(rng, 5, n // 2, n - n // 2, 150, sc.MOTIFS[0], 0.05)
                pairs.append((exactly(q, n), t, dict(zdrop=200, flag=flag, junc=junc)))
    for lds in (8 << 10, 32 << 10, 64 << 10, info["lds_max"]):
        for flag, per_t in ((FOR, 17), (FOR | A, 13)):
            fit = (lds - 304) // per_t // 16 * 16                         # a 300-base query: 304 bytes
            for tlen in (fit, fit + 16):
                q, t, junc = sc.make_intron_pair(rng, 5, 150, 150, tlen - 300, sc.MOTIFS[1], 0.05)
                pairs.append((exactly(q, 300), t, dict(zdrop=-1, flag=flag, junc=junc)))
    got = check(eng, p, *mm.ksw_splice_jobs(pairs), "seams")
    assert sc.has_N(*got).sum() >= len(pairs) // 2


def test_global_image_with_a_narrow_row(eng):
    """What a spliced read's stretch across a long intron looks like: 300-base two-exon queries against targets of 20 000 and 60 000 bases.
    The image (13 T or 17 T bytes and the query) is far beyond LDS and lives in global memory, the row is 320 cells, the slab holds
    60 299 rows of them, and the walk writes one N of five figures."""
    rng = np.random.default_rng(23)
    p = mm.ksw_splice_param()
    pairs = []
    for tlen in (20000, 60000):
        for flag in (FOR, FOR | A, FOR | R, FOR | A | R | FLANK, FOR | REV | X | V, FOR | A | D | X | V | R):
            q, t, junc = sc.make_intron_pair(rng, 5, 150, 150, tlen - 300, sc.MOTIFS[1], 0.03)
            q = exactly(q, 300)
            if flag & V:
                q, t, junc = q[::-1].copy(), t[::-1].copy(), None if junc is None else junc[::-1].copy()
            pairs.append((q, t, dict(zdrop=-1, flag=flag, junc=junc)))
    assert 13 * 20000 + 304 > eng.ksw_info()["lds_max"]
    jobs, q, t, junc = mm.ksw_splice_jobs(pairs)
    got = check(eng, p, jobs, q, t, junc, "long introns")
    assert sc.has_N(*got).all()
    lens = [int(w) >> 4 for w in got[1] if int(w) & 0xf == 3]
    assert max(lens) > 59000 and min(lens) > 19000


def test_one_base_shapes(eng):
    rng = np.random.default_rng(24)
    one = np.array([2], np.uint8)
    long = rng.integers(0, 4, 5000).astype(np.uint8)
    pairs = [(one, long, dict(flag=FOR)), (long, one, dict(flag=FOR)), (one, long, dict(flag=X | REV)), (long, one, dict(flag=X | R | FOR)), (one, long, dict(flag=A | V | FOR))]
    check(eng, mm.ksw_splice_param(), *mm.ksw_splice_jobs(pairs), "1 x 5 000 and 5 000 x 1")


def test_one_job_and_none(eng):
    rng = np.random.default_rng(25)
    p = mm.ksw_splice_param()
    q, t, junc = sc.make_intron_pair(rng, 5, 60, 40, 90, sc.MOTIFS[0], 0.05, p_junc=1.0)
    got = check(eng, p, *mm.ksw_splice_jobs([(q, t, dict(junc=junc))], zdrop=100, flag=FOR), "one job")
    assert sc.has_N(*got).all()
    assert eng.ksw_exts2([], param=p) == []
    res, words = eng.ksw_exts2_batch(p, *mm.ksw_splice_jobs([(np.zeros(0, np.uint8), t)]))
    assert len(res) == 1 and res["score"][0] == mm.KSW_NEG_INF and len(words) == 0
    r = eng.ksw_exts2([(q, t)], flag=FOR)[0]
    assert sorted(r) == sorted(mm.KSW_FIELDS + ("cigar",)) and r["cigar"].dtype == np.uint32 and "N" in mm.cigar_string(r["cigar"])


def test_arenas_are_reused(eng):
    """The same batch before and after a larger one on the same engine: identical bytes."""
    rng = np.random.default_rng(26)
    p = sc.params()[0]
    small = batch_of(rng, p.m, 300, sc.LENS_GPU, p_empty=0.02, intron_hi=300)
    large = batch_of(rng, p.m, 2000, sc.LENS_GPU + [400, 700], intron_hi=2000)
    first = eng.ksw_exts2_batch(p, *small)
    kc.assert_same(eng.ksw_exts2_batch(p, *large), mm.ksw_exts2_host_batch(p, *large, threads=16), "the larger batch", large[0])
    again = eng.ksw_exts2_batch(p, *small)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
    kc.assert_same(first, mm.ksw_exts2_host_batch(p, *small), "the small batch", small[0])


def test_both_forms_take_turns_on_one_engine(eng):
    """The two DPs are one kernel body and share the engine's arenas: a dual-affine batch, a splice-aware one, and both again on the same
    engine.  Each batch has about 40 jobs over the three workgroup sizes (rows of at most 64, at most 256 and more cells), both maxima, and
    a job whose image lives in global memory: 10 000 x 10 000 at w = 50 for the dual-affine form (16 T + Q bytes; the 10 240 x 10 240 pair
    this was first written down with is 1.05 x 10^8 cells and refused by the cell limit, which the test asserts, so it is the largest
    square under the limit), a 300-base query on a 12 800-base target for the splice-aware one (13 T alone is beyond LDS).  Every run
    equals the host form, and a repeat is its first run byte for byte."""
    info = eng.ksw_info()
    rng = np.random.default_rng(28)
    pd, ps = mm.ksw_param(), mm.ksw_splice_param()
    sizes = (30, 200, 420)                                                    # min(qlen, tlen): rows of 48, 224 and 448 cells
    dual, splice = [], []
    for k in range(39):
        n, flag = sizes[k % 3], (0, A, X | R | V, A | D | X, R, A | V)[k // 3 % 6]
        q, t = kc.make_pair(rng, 5, n + int(rng.integers(0, 40)), n, err=0.1)
        dual.append((q, t, dict(w=(-1, n, 500)[k // 3 % 3], zdrop=(200, -1)[k % 2], end_bonus=5, flag=flag)))
        q, t, junc = sc.make_intron_pair(rng, 5, n // 2, n - n // 2, int(rng.integers(20, 400)), sc.MOTIFS[k % 4], 0.05)
        splice.append((exactly(q, n), t, dict(zdrop=(200, -1)[k % 2], flag=flag | (FOR, FOR | REV | FLANK)[k // 3 % 2], junc=junc)))
    big = kc.make_pair(rng, 5, 10000, 10000, err=0.05)
    dual.append(big + (dict(w=50, flag=0),))
    for flag in (FOR, FOR | A):
        q, t, junc = sc.make_intron_pair(rng, 5, 150, 150, 12800 - 300, sc.MOTIFS[1], 0.03)
        splice.append((exactly(q, 300), t, dict(flag=flag, junc=junc)))
    assert 16 * 10000 + 10000 > info["lds_max"] and 13 * 12800 > info["lds_max"]
    with pytest.raises(mm.Mm2gbError, match="MM2GB_KSW_MAX_CELLS"):
        eng.ksw_extd2([(np.zeros(10240, np.uint8), np.zeros(10240, np.uint8))], w=50)
    dual, splice = mm.ksw_jobs(dual), mm.ksw_splice_jobs(splice)
    for jobs in (dual[0], splice[0]):                                         # the three classes, and both maxima
        rows = np.minimum(jobs["qlen"], jobs["tlen"])
        rows = ((np.where(jobs["w"] >= 0, np.minimum(rows, jobs["w"] + 1), rows) + 15) // 16 + 1) * 16
        assert (rows <= info["band"][0]).any() and ((rows > info["band"][0]) & (rows <= info["band"][1])).any() and (rows > info["band"][1]).any()
        assert (jobs["flag"] & A).any() and not (jobs["flag"] & A).all()
    want_d, want_s = mm.ksw_extd2_host_batch(pd, *dual, threads=16), mm.ksw_exts2_host_batch(ps, *splice, threads=16)
    runs = [eng.ksw_extd2_batch(pd, *dual), eng.ksw_exts2_batch(ps, *splice), eng.ksw_extd2_batch(pd, *dual), eng.ksw_exts2_batch(ps, *splice)]
    for k, got in enumerate(runs):
        kc.assert_same(got, (want_d, want_s)[k % 2], ("dual-affine", "splice-aware")[k % 2] + (" batch", " batch again")[k // 2], (dual, splice)[k % 2][0])
    for first, again in ((runs[0], runs[2]), (runs[1], runs[3])):
        assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
    assert sc.has_N(*runs[1]).sum() >= 10 and runs[0][0]["n_cigar"][-1] > 0


def test_several_launches(eng):
    """A slab budget of 1 MiB cuts a batch whose direction bytes need more into several launches; the answers do not change."""
    rng = np.random.default_rng(27)
    p = mm.ksw_splice_param()
    batch = batch_of(rng, p.m, 400, [257, 400, 129], intron_hi=500)
    os.environ["MM2GB_KSW_SLAB_MB"] = "1"
    try:
        got = eng.ksw_exts2_batch(p, *batch)
    finally:
        del os.environ["MM2GB_KSW_SLAB_MB"]
    kc.assert_same(got, mm.ksw_exts2_host_batch(p, *batch), "1 MiB of direction bytes per launch", batch[0])


def test_device_refuses_what_the_host_refuses(eng):
    q = np.zeros(10, np.uint8)
    with pytest.raises(mm.Mm2gbError, match="unknown flag bits 2048"):
        eng.ksw_exts2([(q, q)], flag=0x800 | FOR)
    with pytest.raises(mm.Mm2gbError, match="0x20"):
        eng.ksw_exts2([(q, q)], flag=0x20)
    with pytest.raises(mm.Mm2gbError, match="residue >= m"):
        eng.ksw_exts2([(q + 5, q)])
    with pytest.raises(mm.Mm2gbError, match="MM2GB_KSW_MAX_CELLS"):
        eng.ksw_exts2([(np.zeros(10001, np.uint8), np.zeros(10000, np.uint8))])
    for kw, text in ((dict(e=0, q2=0), "e must be above 0"), (dict(q=-1), "must not be negative"), (dict(q=120, e=8), "exceeds 127"), (dict(noncan=-1), "noncan"),
                     (dict(junc_bonus=-1), "junc_bonus")):
        with pytest.raises(mm.Mm2gbError, match=text):
            eng.ksw_exts2([(q, q)], param=mm.ksw_splice_param(**kw))
    with pytest.raises(mm.Mm2gbError, match="SPLICE_FOR"):             # and the dual-affine call still does not know the bit
        eng.ksw_extd2([(q, q)], flag=FOR)
