"""Cases for the extension DP (mm2gb_ksw_extd2_*): the grid of parameters, batches of jobs from this project's read simulator, the
reference's ksw_extd2_sse through ctypes (oracle/_ref/libminimap2ref.so, where it is built), and the exact comparison of two sets of results.
Test infrastructure only: imported by tests/test_ksw_cpu.py, tests/test_gpu_ksw.py, tests/tools/gen_golden_ksw.py and profiles/ksw_rate.py."""
import ctypes as C
import itertools
import os

import numpy as np

import mm2gb_amd as mm
import orc
import sim_reads

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ksw", "extd2_cases.npz")
REF_LIB = os.path.join(orc.REF_DIR, "libminimap2ref.so")

S, R, G, A, D, X, V = mm.KSW_SCORE_ONLY, mm.KSW_RIGHT, mm.KSW_GENERIC_SC, mm.KSW_APPROX_MAX, mm.KSW_APPROX_DROP, mm.KSW_EXTZ_ONLY, mm.KSW_REV_CIGAR
WIDTHS = [-1, 0, 1, 2, 7, 15, 16, 17, 31, 50, 500]
FLAGS = [0, S, R, G, A, A | D, X, X | R | V, X | A | D, V, G | R | X, S | A | X]
GAPS = [(4, 2, 24, 1), (24, 1, 4, 2), (6, 2, 26, 1), (5, 4, 56, 1), (4, 2, 4, 2)]          # the second is the first swapped (the first cell's constant)
ZDROPS = [-1, 0, 10, 40, 400]
END_BONUS = [-1, 0, 5, 20]
LENS_CPU = sorted({1, 2, 3} | {16 * k + d for k in (1, 2, 3, 4, 8, 16) for d in (-1, 0, 1)} | {5, 24, 100, 200})       # 1..257 around multiples of 16
LENS_GPU = [1, 2, 3, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 127, 128, 129, 257]


def matrices():
    """Four matrices: minimap2's for map-ont; one whose wildcard scores 0 (it then costs the long gap's extension) and whose mismatch is
    too dear for the cheaper gap tuples (the reference returns at once); an asymmetric one (only GENERIC_SC looks at it whole); one with m = 3."""
    rng = np.random.default_rng(7)
    odd = rng.integers(-6, 3, (5, 5))
    odd[0, 0] = 3
    return [(5, mm.ksw_param(a=2, b=4, sc_ambi=1).mat[:]), (5, mm.ksw_param(a=1, b=13, sc_ambi=0).mat[:]), (5, list(odd.reshape(-1))), (3, mm.ksw_param(a=2, b=3, sc_ambi=1, m=3).mat[:])]


def params():
    """Every gap tuple with every matrix: the twenty parameter sets a batch can have."""
    out = []
    for (q, e, q2, e2), (m, mat) in itertools.product(GAPS, matrices()):
        out.append(mm.ksw_param(q=q, e=e, q2=q2, e2=e2, mat=list(mat)[:25], m=m))
    return out


_CODE = np.full(256, 0, np.uint8)
_CODE[list(b"ACGT")] = [0, 1, 2, 3]


def make_pair(rng, m, tlen, qlen, err=None, p_wild=0.02):
    """A target of tlen codes and a query of qlen: the target mutated by the read simulator, then cut or extended at random; wildcards on both."""
    err = rng.choice([0.0, 0.0, 0.02, 0.05, 0.15, 0.4]) if err is None else err
    n_sym = max(m - 1, 1)
    t = rng.integers(0, n_sym, tlen).astype(np.uint8)
    q = _CODE[sim_reads.mutate(rng, sim_reads.BASES[t % 4], err)] % n_sym if tlen > 1 else t.copy()
    if len(q) >= qlen:
        at = rng.integers(0, len(q) - qlen + 1) if rng.random() < 0.3 else 0
        q = q[at:at + qlen]
    else:
        q = np.concatenate([q, rng.integers(0, n_sym, qlen - len(q)).astype(np.uint8)])
    q = q.astype(np.uint8)
    if m > 1:
        t[rng.random(tlen) < p_wild] = m - 1
        q[rng.random(qlen) < p_wild] = m - 1
    return q, t


def make_batch(rng, m, n, lens, p_empty=0.0):
    """n jobs over the grid: lengths from lens, every other setting drawn from the lists above."""
    pairs = []
    for _ in range(n):
        tlen, qlen = int(rng.choice(lens)), int(rng.choice(lens))
        if rng.random() < 0.5:
            qlen = max(1, tlen + int(rng.integers(-3, 4)))
        if rng.random() < p_empty:
            tlen, qlen = (0, qlen) if rng.random() < 0.5 else (tlen, 0)
        q, t = make_pair(rng, m, tlen, qlen)
        pairs.append((q, t, dict(w=int(rng.choice(WIDTHS)), zdrop=int(rng.choice(ZDROPS)), end_bonus=int(rng.choice(END_BONUS)), flag=int(rng.choice(FLAGS)))))
    return mm.ksw_jobs(pairs)


class _Extz(C.Structure):
    _fields_ = [("max_zd", C.c_uint32), ("max_q", C.c_int), ("max_t", C.c_int), ("mqe", C.c_int), ("mqe_t", C.c_int), ("mte", C.c_int), ("mte_q", C.c_int),
                ("score", C.c_int), ("m_cigar", C.c_int), ("n_cigar", C.c_int), ("reach_end", C.c_int), ("cigar", C.POINTER(C.c_uint32))]


def ref_available():
    return os.path.exists(REF_LIB)


_ref = None


def ref_lib():
    global _ref
    if _ref is None:
        _ref = C.CDLL(REF_LIB)
        _ref.ksw_extd2_sse.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int8, C.c_void_p] + [C.c_int8] * 4 + [C.c_int] * 4 + [C.POINTER(_Extz)]
        _ref.ksw_extd2_sse.restype = None
        _ref.kfree.argtypes = [C.c_void_p, C.c_void_p]
        _ref.kfree.restype = None
    return _ref


def ref_batch(param, jobs, queries, targets):
    """The reference's answers for a batch, one call per job: the records (KSW_RES_DTYPE) and the concatenated CIGAR words."""
    L = ref_lib()
    res = np.zeros(len(jobs), mm.KSW_RES_DTYPE)
    words = []
    total = 0
    mat = (C.c_int8 * 25)(*param.mat)
    qp, tp = queries.ctypes.data, targets.ctypes.data
    ez = _Extz()
    for k, j in enumerate(jobs):
        ez.m_cigar, ez.n_cigar, ez.cigar = 0, 0, None
        L.ksw_extd2_sse(None, int(j["qlen"]), qp + int(j["q_off"]), int(j["tlen"]), tp + int(j["t_off"]), param.m, mat, param.q, param.e, param.q2, param.e2,
                        int(j["w"]), int(j["zdrop"]), int(j["end_bonus"]), int(j["flag"]), C.byref(ez))
        mx, zd = ez.max_zd & 0x7fffffff, ez.max_zd >> 31
        res[k] = (mx, zd, ez.max_q, ez.max_t, ez.mqe, ez.mqe_t, ez.mte, ez.mte_q, ez.score, ez.reach_end, ez.n_cigar, 0, total)
        if ez.n_cigar:
            words.append(np.ctypeslib.as_array(ez.cigar, shape=(ez.n_cigar,)).copy())
            total += ez.n_cigar
        if ez.cigar:
            L.kfree(None, ez.cigar)
    return res, (np.concatenate(words) if words else np.zeros(0, np.uint32))


def assert_same(got, want, what, jobs=None):
    """Exact: the eleven fields of every job, where its words lie, and every word."""
    (gr, gw), (wr, ww) = got, want
    assert len(gr) == len(wr), f"{what}: {len(gr)} records against {len(wr)}"
    for k in mm.KSW_FIELDS + ("cigar_off",):
        bad = np.flatnonzero(gr[k] != wr[k])
        if len(bad):
            j = int(bad[0])
            raise AssertionError(f"{what}: {len(bad)} jobs differ in {k}; first job {j}: got {gr[j]} want {wr[j]}" + (f" job {jobs[j]}" if jobs is not None else ""))
    assert len(gw) == len(ww), f"{what}: {len(gw)} CIGAR words against {len(ww)}"
    bad = np.flatnonzero(gw != ww)
    if len(bad):
        j = int(np.searchsorted(wr["cigar_off"], bad[0], side="right")) - 1
        raise AssertionError(f"{what}: {len(bad)} CIGAR words differ, first in job {j}" + (f" {jobs[j]}" if jobs is not None else ""))


def shares(res):
    """The four outcome classes of a set of records, as fractions: z-dropped, reach_end, full CIGAR, no CIGAR."""
    zd = res["zdropped"] != 0
    re = ~zd & (res["reach_end"] != 0)
    full = ~zd & ~re & (res["n_cigar"] > 0)
    n = max(len(res), 1)
    return dict(zdropped=zd.sum() / n, reach_end=re.sum() / n, full_cigar=full.sum() / n, no_cigar=(~zd & ~re & ~full).sum() / n)


def golden_batches():
    """The committed fixtures (tests/tools/gen_golden_ksw.py): per parameter set, (param, jobs, queries, targets, (records, words))."""
    g = np.load(GOLD)
    out = []
    for k, row in enumerate(g["params"]):
        p = mm.ksw_param(q=int(row[26]), e=int(row[27]), q2=int(row[28]), e2=int(row[29]), mat=list(row[1:26]), m=int(row[0]))
        cut = lambda name, ends: g[name][int(g[ends][k]):int(g[ends][k + 1])]
        out.append((p, cut("jobs", "job_end"), cut("queries", "q_end"), cut("targets", "t_end"), (cut("res", "job_end"), cut("words", "word_end"))))
    return out
