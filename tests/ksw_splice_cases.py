"""Cases for the splice-aware DP (mm2gb_ksw_exts2_*): the grid of parameters, batches of jobs (mutated pairs as ksw_cases makes them, and
two-exon queries against targets with a planted intron), the reference's ksw_exts2_sse through ctypes (oracle/_ref/libminimap2ref.so, where
it is built), and the committed fixtures.  Test infrastructure only: imported by tests/test_ksw_splice_cpu.py, tests/test_gpu_ksw_splice.py,
tests/tools/gen_golden_ksw_splice.py and profiles/ksw_splice_rate.py."""
import ctypes as C
import itertools
import os

import numpy as np

import ksw_cases as kc
import mm2gb_amd as mm
import sim_reads

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ksw", "exts2_cases.npz")

S, R, G, A, D, X, V = kc.S, kc.R, kc.G, kc.A, kc.D, kc.X, kc.V
FOR, REV, FLANK = mm.KSW_SPLICE_FOR, mm.KSW_SPLICE_REV, mm.KSW_SPLICE_FLANK
SPLICE_SETS = [0, FOR, REV, FOR | REV, FOR | FLANK, FOR | REV | FLANK]
FLAGS = [a | b for a, b in itertools.product(kc.FLAGS, SPLICE_SETS)]
# (q, e, q2, noncan, junc_bonus): splice, splice:hq, no site costs, q2 <= q + e (the early return), and long_thres = 1.  long_thres = 0 cannot
# be had from parameters that run: q2 > q + e makes (q2 - q) / e at least 1, and with no remainder q2 == q + e + long_thres * e keeps it there.
TUPLES = [(2, 1, 32, 9, 9), (6, 1, 24, 9, 5), (4, 2, 24, 0, 0), (2, 1, 3, 9, 9), (2, 4, 7, 9, 9)]
ZDROPS = [-1, 0, 10, 40, 200]
LENS_CPU, LENS_GPU = kc.LENS_CPU, kc.LENS_GPU
# an intron's first and last bases as residue codes (A C G T = 0 1 2 3): GT..AG, GTA..CAG (the full signal), CT..AC (the reverse strand's), none
MOTIFS = [([2, 3], [0, 2]), ([2, 3, 0], [1, 0, 2]), ([1, 3], [0, 1]), ([], [])]


def long_thres(q, e, q2):
    lt = int((q2 - q) / e) - 1
    return lt + 1 if q2 > q + e + lt * e else lt


def params(tuples=None):
    """Every gap tuple with every matrix of ksw_cases.matrices(): the twenty parameter sets a batch can have."""
    out = []
    for (q, e, q2, nc, jb), (m, mat) in itertools.product(TUPLES if tuples is None else tuples, kc.matrices()):
        out.append(mm.ksw_splice_param(q=q, e=e, q2=q2, noncan=nc, junc_bonus=jb, mat=list(mat)[:25], m=m))
    return out


def make_intron_pair(rng, m, len1, len2, intron, motif, err, p_junc=0.5, p_wild=0.01):
    """query = exon1 + exon2, mutated; target = exon1 + intron + exon2, the intron beginning and ending with motif.  Returns query, target and
    junc, which marks the two boundaries as ksw_exts2_sse reads them (donor bits at the intron's first base, acceptor bits at its last) with
    probability p_junc, else is None."""
    n_sym = max(m - 1, 1)
    e1, e2 = rng.integers(0, n_sym, len1).astype(np.uint8), rng.integers(0, n_sym, len2).astype(np.uint8)
    mid = rng.integers(0, n_sym, intron).astype(np.uint8)
    head, tail = (np.array(x, np.uint8) % n_sym for x in motif)
    if len(head):
        mid[:len(head)] = head
        mid[intron - len(tail):] = tail
    t = np.concatenate([e1, mid, e2])
    ex = np.concatenate([e1, e2])
    q = (kc._CODE[sim_reads.mutate(rng, sim_reads.BASES[ex % 4], err)] % n_sym).astype(np.uint8) if len(ex) > 1 else ex.copy()
    if len(q) == 0:
        q = ex.copy()
    if m > 1:
        t[rng.random(len(t)) < p_wild] = m - 1
        q[rng.random(len(q)) < p_wild] = m - 1
    junc = None
    if rng.random() < p_junc:
        junc = np.zeros(len(t), np.uint8)
        bits = [(1, 2), (8, 4), (1 | 8, 2 | 4)][int(rng.integers(0, 3))]
        junc[len1] |= bits[0]
        junc[len1 + intron - 1] |= bits[1]
    return q, t, junc


def make_batch(rng, m, n, lens, p_planted=0.5, p_empty=0.0, intron_hi=3000, flags=None, zdrops=None):
    """n jobs over the grid, as pairs for mm.ksw_splice_jobs.  A planted job whose flags carry REV_CIGAR is handed over reversed, as a left
    extension is: the mirrored orientation."""
    flags, zdrops = FLAGS if flags is None else flags, ZDROPS if zdrops is None else zdrops
    pairs = []
    for _ in range(n):
        opt = dict(zdrop=int(rng.choice(zdrops)), flag=int(rng.choice(flags)))
        if rng.random() < p_planted:
            # a good third below the `splice` tuple's long_thres + 1 = 30 bases, where the gap is still a deletion; the rest log-uniform
            intron = int(rng.integers(20, 30)) if rng.random() < 0.35 else int(round(np.exp(rng.uniform(np.log(20), np.log(intron_hi)))))
            q, t, junc = make_intron_pair(rng, m, int(rng.choice(lens)), int(rng.choice(lens)), intron, MOTIFS[int(rng.integers(0, 4))], float(rng.choice([0.0, 0.02, 0.05, 0.12])))
            if opt["flag"] & V:
                q, t, junc = q[::-1].copy(), t[::-1].copy(), None if junc is None else junc[::-1].copy()
            if junc is not None:
                opt["junc"] = junc
        else:
            tlen, qlen = int(rng.choice(lens)), int(rng.choice(lens))
            if rng.random() < 0.5:
                qlen = max(1, tlen + int(rng.integers(-3, 4)))
            if rng.random() < p_empty:
                tlen, qlen = (0, qlen) if rng.random() < 0.5 else (tlen, 0)
            q, t = kc.make_pair(rng, m, tlen, qlen)
            if rng.random() < 0.2 and tlen:
                opt["junc"] = (rng.integers(0, 16, tlen) * (rng.random(tlen) < 0.1)).astype(np.uint8)
        pairs.append((q, t, opt))
    return pairs


def planted_batch(rng, n, lens, m=5):
    """The planted kind alone, without SCORE_ONLY and with the sites switched on: the set the conditions on the inputs are counted over."""
    flags = [f for f in FLAGS if not f & S and f & (FOR | REV)]
    return make_batch(rng, m, n, lens, p_planted=1.0, flags=flags)


_ref = None


def ref_lib():
    global _ref
    if _ref is None:
        _ref = C.CDLL(kc.REF_LIB)
        _ref.ksw_exts2_sse.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int8, C.c_void_p] + [C.c_int8] * 4 + [C.c_int, C.c_int8, C.c_int, C.c_void_p,
                                       C.POINTER(kc._Extz)]
        _ref.ksw_exts2_sse.restype = None
        _ref.kfree.argtypes = [C.c_void_p, C.c_void_p]
        _ref.kfree.restype = None
    return _ref


def ref_batch(param, jobs, queries, targets, junc=None, score_only_as_is=False):
    """The reference's answers for a batch, one call per job.  A SCORE_ONLY job is run WITHOUT that flag and its words dropped: the SSE2
    build's score-only loop computes another x2 than its CIGAR loops do, and the definition here is the latter.
    score_only_as_is: hand the flag over as it is (to see that difference)."""
    L = ref_lib()
    res = np.zeros(len(jobs), mm.KSW_RES_DTYPE)
    words = []
    total = 0
    mat = (C.c_int8 * 25)(*param.mat)
    qp, tp, jp = queries.ctypes.data, targets.ctypes.data, None if junc is None else junc.ctypes.data
    ez = kc._Extz()
    for k, j in enumerate(jobs):
        ez.m_cigar, ez.n_cigar, ez.cigar = 0, 0, None
        flag = int(j["flag"])
        L.ksw_exts2_sse(None, int(j["qlen"]), qp + int(j["q_off"]), int(j["tlen"]), tp + int(j["t_off"]), param.m, mat, param.q, param.e, param.q2, param.noncan,
                        int(j["zdrop"]), param.junc_bonus, flag if score_only_as_is else flag & ~S, None if jp is None else jp + int(j["t_off"]), C.byref(ez))
        n = 0 if flag & S else ez.n_cigar
        mx, zd = ez.max_zd & 0x7fffffff, ez.max_zd >> 31
        res[k] = (mx, zd, ez.max_q, ez.max_t, ez.mqe, ez.mqe_t, ez.mte, ez.mte_q, ez.score, ez.reach_end, n, 0, total)
        if n:
            words.append(np.ctypeslib.as_array(ez.cigar, shape=(n,)).copy())
            total += n
        if ez.cigar:
            L.kfree(None, ez.cigar)
    return res, (np.concatenate(words) if words else np.zeros(0, np.uint32))


def has_N(res, words):
    """Per job: does its CIGAR carry an N word?"""
    is_n = np.concatenate([[0], np.cumsum((words & 0xf) == 3)])
    return is_n[res["cigar_off"] + res["n_cigar"]] > is_n[res["cigar_off"]]


def input_shares(jobs, res, words):
    """The three shares the issue conditions the planted inputs on: jobs with an N word, z-dropped jobs, full-length CIGARs without N."""
    n = max(len(res), 1)
    with_n = has_N(res, words)
    full = (res["zdropped"] == 0) & (res["n_cigar"] > 0) & ~with_n & ((jobs["flag"] & X) == 0)
    return dict(with_N=float(with_n.sum()) / n, zdropped=float((res["zdropped"] != 0).sum()) / n, full_no_N=float(full.sum()) / n)


def check_input_shares(sh):
    assert sh["with_N"] >= 0.1 and sh["zdropped"] >= 0.05 and sh["full_no_N"] >= 0.1, sh


def golden_batches():
    """The committed fixtures (tests/tools/gen_golden_ksw_splice.py): per parameter set, (param, jobs, queries, targets, junc, (records, words))."""
    g = np.load(GOLD)
    out = []
    for k, row in enumerate(g["params"]):
        p = mm.ksw_splice_param(q=int(row[26]), e=int(row[27]), q2=int(row[28]), noncan=int(row[29]), junc_bonus=int(row[30]), mat=list(row[1:26]), m=int(row[0]))
        cut = lambda name, ends: g[name][int(g[ends][k]):int(g[ends][k + 1])]
        out.append((p, cut("jobs", "job_end"), cut("queries", "q_end"), cut("targets", "t_end"), cut("junc", "t_end"), (cut("res", "job_end"), cut("words", "word_end"))))
    return out
