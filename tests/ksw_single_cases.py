"""Cases for the single-affine extension DP (mm2gb_ksw_extz2_*): ksw_cases' grid with one gap cost, the reference's ksw_extz2_sse through
ctypes (oracle/_ref/libminimap2ref.so, where it is built), and the committed fixtures.
Test infrastructure only: imported by tests/test_ksw_single_cpu.py, tests/test_gpu_ksw_single.py, tests/tools/gen_golden_ksw_single.py and
profiles/ksw_single_rate.py."""
import ctypes as C
import itertools
import os

import numpy as np

import ksw_cases as kc
import mm2gb_amd as mm

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ksw", "extz2_cases.npz")
# (39, 3): 2(q + e) = 84, the last even value options.c lets through with e = 3; with a match of 45 the cap mat[0] + 2(q + e) passes 127
GAPS = [(4, 2), (6, 2), (2, 1), (12, 2), (39, 3)]


def param(q=4, e=2, **kw):
    """ksw_param with q2 = q and e2 = e (neither is read by the single-affine calls)."""
    return mm.ksw_param(q=q, e=e, q2=q, e2=e, **kw)


def params():
    """Every gap pair with every matrix of ksw_cases: the twenty parameter sets a batch can have."""
    return [param(q, e, mat=list(mat)[:25], m=m) for (q, e), (m, mat) in itertools.product(GAPS, kc.matrices())]


# single-affine scoring above the DP (tests/tools/gen_golden_paf_single.py): the recorded alignment batches, name of tests/golden/align's batch ->
# (q, e), and the command line that makes the reference's program take that path
PAF_GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "paf_single")
ALIGN_BATCHES = {"ont": (4, 2), "pb": (6, 2)}
PAF_FLAGS = ["-O4", "-E2"]


def align_fixture(name):
    """(refs, reads, preset) of a recorded alignment batch: the path reads of tests/golden/align's batch, and six reads with a deletion or an
    insertion of 25-90 bases inside a fill -- past (q2 - q) / (e - e2), where the two gap models part."""
    import align_cases as ac
    import sim_reads
    refs, reads, preset, _ = ac.fixture_batches()[name]
    rng = np.random.default_rng(31)
    g = [np.frombuffer(s, np.uint8) for s in refs]
    more = []
    for k, n in enumerate((25, 40, 60, 90, 33, 70)):
        c = k % len(g); st = 2000 + 3500 * k
        left, right = sim_reads.mutate(rng, np.array(g[c][st:st + 1200]), 0.03), sim_reads.mutate(rng, np.array(g[c][st + 1200 + (n if k % 2 == 0 else 0):st + 2400]), 0.03)
        mid = sim_reads.BASES[rng.integers(0, 4, n)] if k % 2 else np.zeros(0, np.uint8)
        s = np.concatenate([left, mid, right])
        more.append(bytes(np.asarray(sim_reads.revcomp(s) if k % 3 == 0 else s, np.uint8)))
    return refs, list(reads) + more, preset


def load_align(name):
    """A recorded alignment batch: (the call's input, what the reference answered), as align_cases.load_batch gives them."""
    import align_cases as ac
    return ac.load_batch(os.path.join(os.pardir, "paf_single", "align_" + name))


def run_align_host(b, threads=4):
    return mm.align_regs_extz_host(b["opt"], b["k"], b["hpc"], b["refs"], b["reads"], b["regs"], b["anchors"], threads=threads)


def run_align_gpu(eng, b):
    return eng.align_regs_extz(b["opt"], b["k"], b["hpc"], b["refs"], b["reads"], b["regs"], b["anchors"])


TRAPS = ("m1", "cap", "min_equal", "min_above", "one_base", "w0")


def trap_batches(seed=22):
    """The named traps of DESIGN 6d-c as small batches, name -> (param, jobs, queries, targets):
    m1: m = 1, which the dual-affine DP returns from at once and this one does not;
    cap: mat[0] + 2(q + e) = 129, past the signed byte the compares read;
    min_equal / min_above: -min(mat) = 2(q + e), the last value that runs, and one above it, which returns at once;
    one_base: a query or a target of one base; w0: the band of width 0."""
    rng = np.random.default_rng(seed)
    out = {}
    out["m1"] = (param(4, 2, m=1, mat=[1]),) + kc.make_batch(rng, 1, 40, kc.LENS_CPU)
    out["cap"] = (param(39, 3, a=45, b=80),) + kc.make_batch(rng, 5, 60, kc.LENS_CPU)
    out["min_equal"] = (param(4, 2, a=1, b=12),) + kc.make_batch(rng, 5, 40, kc.LENS_CPU)
    out["min_above"] = (param(4, 2, a=1, b=13),) + kc.make_batch(rng, 5, 20, kc.LENS_CPU)
    p = param(4, 2)
    pairs = []
    for k in range(40):
        n = int(rng.choice(kc.LENS_CPU))
        q, t = kc.make_pair(rng, 5, 1 if k % 2 else n, n if k % 2 else 1)
        pairs.append((q, t, dict(w=int(rng.choice(kc.WIDTHS)), zdrop=int(rng.choice(kc.ZDROPS)), end_bonus=int(rng.choice(kc.END_BONUS)), flag=int(rng.choice(kc.FLAGS)))))
    out["one_base"] = (p,) + mm.ksw_jobs(pairs)
    jobs, q, t = kc.make_batch(rng, 5, 40, kc.LENS_CPU)
    jobs["w"] = 0
    out["w0"] = (p, jobs, q, t)
    return out


_ref = None


def ref_lib():
    global _ref
    if _ref is None:
        _ref = kc.ref_lib()
        _ref.ksw_extz2_sse.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int8, C.c_void_p] + [C.c_int8] * 2 + [C.c_int] * 4 + [C.POINTER(kc._Extz)]
        _ref.ksw_extz2_sse.restype = None
    return _ref


def ref_batch(p, jobs, queries, targets):
    """The reference's answers for a batch, one call per job: the records (KSW_RES_DTYPE) and the concatenated CIGAR words."""
    L = ref_lib()
    res = np.zeros(len(jobs), mm.KSW_RES_DTYPE)
    words = []
    total = 0
    mat = (C.c_int8 * 25)(*p.mat)
    qp, tp = queries.ctypes.data, targets.ctypes.data
    ez = kc._Extz()
    for k, j in enumerate(jobs):
        ez.m_cigar, ez.n_cigar, ez.cigar = 0, 0, None
        L.ksw_extz2_sse(None, int(j["qlen"]), qp + int(j["q_off"]), int(j["tlen"]), tp + int(j["t_off"]), p.m, mat, p.q, p.e,
                        int(j["w"]), int(j["zdrop"]), int(j["end_bonus"]), int(j["flag"]), C.byref(ez))
        mx, zd = ez.max_zd & 0x7fffffff, ez.max_zd >> 31
        res[k] = (mx, zd, ez.max_q, ez.max_t, ez.mqe, ez.mqe_t, ez.mte, ez.mte_q, ez.score, ez.reach_end, ez.n_cigar, 0, total)
        if ez.n_cigar:
            words.append(np.ctypeslib.as_array(ez.cigar, shape=(ez.n_cigar,)).copy())
            total += ez.n_cigar
        if ez.cigar:
            L.kfree(None, ez.cigar)
    return res, (np.concatenate(words) if words else np.zeros(0, np.uint32))


def dump_batch(path, p, jobs, queries, targets, want):
    """One batch and its expected answers as the file tests/tools/ksw_single_replay.cpp reads."""
    res, words = want
    with open(path, "wb") as f:
        f.write(np.array([len(jobs), len(queries), len(targets), len(words), C.sizeof(p)], np.int64).tobytes())
        f.write(bytes(p))
        for x, dt in ((jobs, mm.KSW_JOB_DTYPE), (queries, np.uint8), (targets, np.uint8), (res, mm.KSW_RES_DTYPE), (words, np.uint32)):
            f.write(np.ascontiguousarray(x, dtype=dt).tobytes())


def golden_batches(traps=False):
    """The committed fixtures (tests/tools/gen_golden_ksw_single.py): per parameter set, (param, jobs, queries, targets, (records, words)).
    traps: the batches of trap_batches() instead, which the file holds behind the grid's sets, in the order of TRAPS."""
    g = np.load(GOLD)
    out = []
    n_grid = len(g["params"]) - len(TRAPS)
    for k, row in enumerate(g["params"]):
        if (k >= n_grid) != traps:
            continue
        p = param(int(row[26]), int(row[27]), mat=list(row[1:26]), m=int(row[0]))
        cut = lambda name, ends: g[name][int(g[ends][k]):int(g[ends][k + 1])]
        out.append((p, cut("jobs", "job_end"), cut("queries", "q_end"), cut("targets", "t_end"), (cut("res", "job_end"), cut("words", "word_end"))))
    return out
