"""Cases for the HiFi and assembly presets (map-hifi / map-ccs, asm5, asm10, asm20): the simulated contigs, the reference's option sets, its
chaining under MM_F_RMQ (mg_lchain_rmq first, map.c:690-707) and mm_align_skeleton through ctypes where oracle/_ref is built, the DP's parameter
sets at the presets' scores, and the committed fixtures (tests/golden/asm, tests/golden/ksw/extd2_asm_cases.npz).  Test infrastructure only:
imported by tests/test_asm_cpu.py, tests/test_gpu_asm.py and tests/tools/gen_golden_asm.py."""
import ctypes as C
import hashlib
import json
import os

import numpy as np

import align_cases as ac
import golden_io
import ksw_cases as kc
import mm2gb_amd as mm
import orc
import sim_reads

GOLD = os.path.join(golden_io.GOLD, "asm")
KSW_GOLD = os.path.join(golden_io.GOLD, "ksw", "extd2_asm_cases.npz")
PRESETS = ("map-hifi", "asm5", "asm10", "asm20")
NAMES = PRESETS + ("map-ccs",)
ASM = ("asm5", "asm10", "asm20")
INDEX = {n: dict(k=19, w=10 if n == "asm20" else 19, hpc=False) for n in NAMES}
ac.PRESETS.update(INDEX)                                 # (align_cases' RefIndex looks the index parameters up by name)
INF = 2**31 - 1
SKIPS = {"inf": INF, "s25": 25}
F_RMQ = 0x80000000
# the mapping fields a preset sets, beside those mm2gb_align_opt_t has
MAP_FIELDS = ("flag", "max_gap", "bw", "bw_long", "min_mid_occ", "max_mid_occ", "best_n", "occ_dist")
PAIRS = {"mt": ("MT-human.fa", "MT-orang.fa"), "inv": ("t-inv.fa", "q-inv.fa")}
DIVS = {"d05": 0.005, "d3": 0.03, "d8": 0.08}
EMPTY = ("d8", "asm5")                                   # the one recorded set without a line: it stays the case of no output
# the simulated set's parameters (the generator adds the seed, where each contig lies (place_contigs) and the md5, and writes them to tests/golden/asm/sim.json)
SIM = dict(genome=dict(n_chr=2, chr_len=200_000, n_rep_families=3, rep_len=2000, copies=6, tandem=2), inversion=1500, deletion=4000)
# (name, length on the reference, kind).  Only the plain contig, the shortest, lies across a tandem array: a contig across one has hundreds of thousands of
# raw anchors, tens of seconds of chaining for either program, and one such contig is what a test needs
CONTIGS = (("ctg_inv", 70_000, "inversion"), ("ctg_del", 62_300, "deletion"), ("ctg_rc", 85_000, "revcomp"), ("ctg_plain", 35_000, "plain"))


# ---------------------------------------------------------------- the simulated contigs
def sim_set(meta):
    """(references, {divergence tag: contigs}), both lists of (name, bytes): 2 chromosomes of 200 kb from tests/sim_reads.make_genome and four contigs of
    30-90 kb cut from them -- one with a stretch of 1.5 kb reverse-complemented, one with 4 kb deleted, one reverse-complemented whole, one plain --
    each mutated at 0.5 %, 3 % and 8 %."""
    rng = np.random.default_rng(meta["seed"])
    chrs = sim_reads.make_genome(rng, **meta["genome"])
    base = []
    for name, c, st, n, kind in meta["contigs"]:
        s, m = chrs[c][st:st + n].copy(), n // 2
        if kind == "inversion":
            s = np.concatenate([s[:m], sim_reads.revcomp(s[m:m + meta["inversion"]]), s[m + meta["inversion"]:]])
        elif kind == "deletion":
            s = np.concatenate([s[:m], s[m + meta["deletion"]:]])
        base.append((name, kind, s))
    out = {}
    for tag, err in DIVS.items():
        recs = []
        for name, kind, s in base:
            x = sim_reads.mutate(rng, s, err)
            recs.append((f"{name}_{tag}", bytes(sim_reads.revcomp(x) if kind == "revcomp" else x)))
        out[tag] = recs
    return [(f"chr{k + 1}", bytes(c)) for k, c in enumerate(chrs)], out


def tandem_spans(seq, min_run=1500):
    """[(start, end)] of the tandem arrays of a sequence of sim_reads.make_genome (units of 30-199 bases): the stretches that equal themselves one period on."""
    s = np.frombuffer(bytes(seq), np.uint8)
    mark = np.zeros(len(s) + 1, np.int32)
    for p in range(30, 200):
        eq = np.concatenate([[0], (s[:-p] == s[p:]).astype(np.int8), [0]])
        edge = np.flatnonzero(np.diff(eq))
        for a, b in zip(edge[::2], edge[1::2]):
            if b - a >= min_run:
                mark[a] += 1; mark[b + p] -= 1
    inside = np.concatenate([[0], (np.cumsum(mark[:-1]) > 0).astype(np.int8), [0]])
    edge = np.flatnonzero(np.diff(inside))
    return [(int(a), int(b)) for a, b in zip(edge[::2], edge[1::2])]


def place_contigs(meta):
    """meta["contigs"] = [[name, chromosome, start, length, kind]] for CONTIGS on the genome of meta's seed: the plain contig around the shortest tandem
    array that it can hold with 8 kb either side, every other contig at the first place (in steps of 5 kb, chromosomes in turn) at least 2 kb away from
    every array.  None where the genome has no such places."""
    rng = np.random.default_rng(meta["seed"])
    chrs = sim_reads.make_genome(rng, **meta["genome"])
    spans = [tandem_spans(c) for c in chrs]
    out = []
    for name, n, kind in CONTIGS:
        if kind == "plain":
            fit = sorted((b - a, c, a) for c, sp in enumerate(spans) for a, b in sp if b - a <= n - 16_000 and a >= 8000 and a - 8000 + n <= len(chrs[c]))
            if not fit:
                return None
            out.append([name, fit[0][1], fit[0][2] - 8000, n, kind])
            continue
        free = [(c, st) for st in range(0, len(chrs[0]) - n, 5000) for c in range(len(chrs)) if all(b + 2000 <= st or a - 2000 >= st + n for a, b in spans[c])]
        taken = [(x[1], x[2]) for x in out]
        free = [x for x in free if x not in taken] or free
        if not free:
            return None
        out.append([name, free[len(out) % len(free)][0], free[len(out) % len(free)][1], n, kind])
    return dict(meta, contigs=out)


def same_paf(got, want, what):
    if got != want:
        g, w = got.splitlines(), want.splitlines()
        bad = [k for k in range(min(len(g), len(w))) if g[k] != w[k]]
        first = bad[0] if bad else min(len(g), len(w))
        at = next((i for i, (x, y) in enumerate(zip(g[first], w[first])) if x != y), None) if bad else None
        raise AssertionError(f"{what}: {len(bad)} of {len(w)} PAF lines differ (got {len(g)}); first: line {first}, byte {at}: "
                             f"{g[first][max((at or 0) - 60, 0):(at or 0) + 60] if bad else None!r} vs {w[first][max((at or 0) - 60, 0):(at or 0) + 60] if bad else None!r}")


def sim_md5(refs, contigs):
    h = hashlib.md5()
    for _, s in refs + [r for tag in DIVS for r in contigs[tag]]:
        h.update(s)
    return h.hexdigest()


_sim = None


def load_sim():
    """The committed set, regenerated from tests/golden/asm/sim.json (once per process)."""
    global _sim
    if _sim is None:
        meta = json.load(open(os.path.join(GOLD, "sim.json")))
        refs, contigs = sim_set(meta)
        assert sim_md5(refs, contigs) == meta["md5"], "simulator drifted: regenerate the golden"
        _sim = (refs, contigs)
    return _sim


def pair_inputs(pair):
    """(references, queries) of a recorded pair: one of PAIRS, or "sim_<tag>"."""
    if pair in PAIRS:
        t, q = PAIRS[pair]
        return read_fasta(os.path.join(ac.DATA, t)), read_fasta(os.path.join(ac.DATA, q))
    refs, contigs = load_sim()
    return refs, contigs[pair[4:]]


def read_fasta(path):
    """[(name, sequence)]"""
    out = []
    for line in open(path, "rb"):
        if line.startswith(b">"):
            out.append([line[1:].split()[0].decode(), []])
        else:
            out[-1][1].append(line.strip())
    return [(n, b"".join(s)) for n, s in out]


# ---------------------------------------------------------------- the recorded PAFs
def paf_key(pair, preset, skip, variant):
    return f"{pair}.{preset}.{skip}.{variant}"


def paf_cases():
    """Every recorded (pair, preset, skip, variant): skip infinity for the four presets, the reference's default 25 for the asm presets; -c --cs for asm10 as well."""
    out = []
    for pair in list(PAIRS) + ["sim_" + t for t in DIVS]:
        for preset in PRESETS:
            for skip in SKIPS:
                if skip == "s25" and preset not in ASM:
                    continue
                for variant in ("c", "cs") if preset == "asm10" else ("c",):
                    out.append((pair, preset, skip, variant))
    return out


_pafs = None


def golden_paf(pair, preset, skip, variant):
    global _pafs
    if _pafs is None:
        _pafs = np.load(os.path.join(GOLD, "pafs.npz"))
    return _pafs[paf_key(pair, preset, skip, variant)].tobytes().decode()


def golden_options():
    return json.load(open(os.path.join(GOLD, "options.json")))


# ---------------------------------------------------------------- the reference's options
def ref_options(name):
    """mm_set_opt(NULL) + mm_set_opt(name): every field of mm2gb_align_opt_t, MAP_FIELDS, and the index's k, w, hpc."""
    L = ac.ref_lib()
    io, mo = ac._IdxOpt(), ac.MapOpt()
    assert L.mm_set_opt(None, C.byref(io), C.byref(mo)) == 0 and L.mm_set_opt(name.encode(), C.byref(io), C.byref(mo)) == 0
    d = dict(align={k: getattr(mo, k) for k, _ in mm.AlignOpt._fields_}, map={k: getattr(mo, k) for k in MAP_FIELDS}, index=dict(k=io.k, w=io.w, hpc=bool(io.flag & 1)))
    return json.loads(json.dumps(d))             # (floats as JSON holds them)


def own_options(name):
    """The same three groups from this project's calls."""
    a, m = mm.align_opt(name), mm.map_opt_preset(name)
    d = dict(align={k: getattr(a, k) for k, _ in mm.AlignOpt._fields_}, map={k: getattr(m, k) for k in MAP_FIELDS}, index=mm.preset(name))
    return json.loads(json.dumps(d))


# ---------------------------------------------------------------- anchors, chaining parameters
def own_anchors(refs, reads, preset, threads=4):
    """Every read's raw sorted anchors from this project's seeding path at the preset's k, w and mid_occ bounds (50, 500)."""
    p = INDEX[preset]
    with mm.SeedIndex(refs, k=p["k"], w=p["w"], hpc=False, threads=threads) as ix:
        mid_occ = ix.mid_occ(min_mid_occ=50, max_mid_occ=500)
        recs = [ix.matches(s, mid_occ) for s in reads]
    return mm.collect_seeds_host(0, recs, threads=threads) if recs else []


def pen_gap(k=19):
    return np.float32(float(np.float32(0.8)) * 0.01 * k)     # map.c:688: float * double * int, kept as a float


def rmq_param_first(skip):
    """What map.c:691 passes under the asm presets: bw = 1000, max_gap = 10000 (orc's parameter set; to_lib for this project's)."""
    return orc.default_rmq_param(max_dist=10000, max_dist_inner=1000, bw=1000, max_chn_skip=skip, pen_gap=pen_gap(), pen_skip=np.float32(0.0))


def to_lib(prm):
    return mm.RmqParam(max_dist=prm.max_dist, max_dist_inner=prm.max_dist_inner, bw=prm.bw, max_chn_skip=prm.max_chn_skip, cap_rmq_size=prm.cap_rmq_size,
                       min_cnt=prm.min_cnt, min_sc=prm.min_sc, chn_pen_gap=np.float32(prm.pen_gap), chn_pen_skip=np.float32(prm.pen_skip))


def offsets_of(anchors):
    off = np.zeros(len(anchors) + 1, np.int64)
    off[1:] = np.cumsum([len(a) for a in anchors])
    return off


def same_chains(got, want, what):
    assert len(got) == len(want), what
    for r, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]), f"{what}: read {r} differs"


# ---------------------------------------------------------------- the reference's chaining and mm_align_skeleton
def _declare(L):
    L.mg_lchain_rmq.restype = C.c_void_p
    L.mg_lchain_rmq.argtypes = [C.c_int] * 7 + [C.c_float, C.c_float, C.c_int64, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_void_p), C.c_void_p]
    L.radix_sort_128x.restype = None
    L.radix_sort_128x.argtypes = [C.c_void_p, C.c_void_p]


def ref_prepare(ri, read, anchors, r_id, squeeze=True):
    """align_cases.ref_prepare with map.c's own chaining: mg_lchain_rmq with bw under MM_F_RMQ, mg_lchain_dp otherwise (map.c:690-696), then the
    re-chaining with bw_long where map.c:698-707 asks for it.  Returns its five values and whether the read was re-chained."""
    L, mo = ac.ref_lib(), ri.mo
    _declare(L)
    a = np.ascontiguousarray(anchors, dtype=np.uint64).reshape(-1, 2)
    none = (None, 0, None, np.zeros(0, mm.REG_DTYPE), np.zeros((0, 2), np.uint64))
    if len(a) == 0:
        return none + (False,)
    n_u, u_ptr = C.c_int(0), C.c_void_p(0)
    buf = ac._libc.malloc(a.nbytes)
    C.memmove(buf, a.ctypes.data, a.nbytes)
    gap, skip = pen_gap(ri.io.k), np.float32(mo.chain_skip_scale * 0.01 * ri.io.k)
    rmq = lambda bw, n, ptr: L.mg_lchain_rmq(mo.max_gap, mo.rmq_inner_dist, bw, mo.max_chain_skip, mo.rmq_size_cap, mo.min_cnt, mo.min_chain_score, gap, skip, n, ptr, C.byref(n_u), C.byref(u_ptr), None)
    if mo.flag & F_RMQ:
        out = rmq(mo.bw, len(a), buf)
    else:
        out = L.mg_lchain_dp(mo.max_gap, mo.max_gap, mo.bw, mo.max_chain_skip, mo.max_chain_iter, mo.min_cnt, mo.min_chain_score, gap, skip, 0, 1, len(a), buf, C.byref(n_u), C.byref(u_ptr), None)
    if n_u.value == 0:
        return none + (False,)
    again = False
    if mo.bw_long > mo.bw and n_u.value > 1:
        u = np.ctypeslib.as_array(C.cast(u_ptr, C.POINTER(C.c_uint64)), shape=(n_u.value,))
        n_a = int((u & 0xffffffff).sum())
        y = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint64)), shape=(n_a, 2))[:, 1].astype(np.uint32).astype(np.int32)
        st, en = int(y[0]), int(y[int(u[0] & 0xffffffff) - 1])
        if len(read) - (en - st) > mo.rmq_rescue_size or np.float32(en - st) > np.float32(len(read)) * np.float32(mo.rmq_rescue_ratio):
            again = True
            ac._libc.free(u_ptr)
            L.radix_sort_128x(out, out + n_a * 16)
            out = rmq(mo.bw_long, n_a, out)
            if n_u.value == 0:
                return none + (True,)
    regs = L.mm_gen_regs(None, ac.read_hash(r_id), len(read), n_u.value, u_ptr, out, 0)
    n_out = int((np.ctypeslib.as_array(C.cast(u_ptr, C.POINTER(C.c_uint64)), shape=(n_u.value,)) & 0xffffffff).sum())
    ac._libc.free(u_ptr)
    n = C.c_int(n_u.value)
    L.mm_set_parent(None, mo.mask_level, mo.mask_len, n.value, regs, mo.a * 2 + mo.b, int(bool(mo.flag & 0x20000000)), mo.alt_drop)
    L.mm_select_sub(None, mo.pri_ratio, ri.io.k * 2, mo.best_n, 1, int(mo.max_gap * 0.8), C.byref(n), regs)
    # mm_squeeze_a (hit.c) here already, on the reference's own arrays: only the anchors of the records that are left travel on -- a contig across a tandem
    # array has hundreds of thousands that no record holds.  mm_align_skeleton's own squeeze then moves nothing, and both sides get the same input
    ints = np.ctypeslib.as_array(C.cast(regs, C.POINTER(C.c_int32)), shape=(max(n.value, 1), ac.REG1_BYTES // 4))[:n.value]
    arr = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint64)), shape=(n_out, 2))
    src, pos = arr.copy(), 0
    if not squeeze:                                           # (one small fixture keeps the arrays as the chaining left them)
        return regs, n.value, out, ac._snap_regs(regs, n.value)[0], arr.copy(), again
    for i in np.argsort(ints[:, 10], kind="stable"):          # column 10: as, column 1: cnt
        at, cnt = int(ints[i, 10]), int(ints[i, 1])
        arr[pos:pos + cnt] = src[at:at + cnt]
        ints[i, 10] = pos
        pos += cnt
    return regs, n.value, out, ac._snap_regs(regs, n.value)[0], arr[:pos].copy(), again


def ref_batch(refs, reads, preset, anchors=None, squeeze=True):
    """align_cases.ref_batch for these presets: (the call's input, `want`, how many reads the reference re-chained)."""
    ri = ac.RefIndex(refs, preset)
    try:
        anchors = own_anchors(refs, reads, preset) if anchors is None else anchors
        regs_in, a_in, want, n_again = [], [], [], 0
        for r, (s, a) in enumerate(zip(reads, anchors)):
            regs, n, a_ptr, snap_r, snap_a, again = ref_prepare(ri, s, a, r, squeeze)
            regs_in.append(snap_r); a_in.append(snap_a); n_again += again
            want.append(ac.ref_align(ri, s, regs, n, a_ptr))
        return dict(opt=ac.opt_from_ref(ri.mo), k=ri.io.k, hpc=False, refs=[bytes(s) for s in refs], reads=[bytes(s) for s in reads], regs=regs_in, anchors=a_in), want, n_again
    finally:
        ri.close()


def load_align(preset):
    """tests/golden/asm/align_<preset>.npz in align_cases' layout: (batch, want)."""
    keep = ac.GOLD
    ac.GOLD = GOLD
    try:
        return ac.load_batch("align_" + preset)
    finally:
        ac.GOLD = keep


def fresh_contigs(seed, n=40):
    """For the live comparison: a genome of 2 x 60 kb and n contigs of 3-12 kb at 0.5-8 %, a tenth with junk or an inverted block in the middle."""
    rng = np.random.default_rng(seed)
    g = sim_reads.make_genome(rng, n_chr=2, chr_len=60_000, n_rep_families=2, rep_len=1500, copies=6, tandem=0)      # (a tandem array can be longer than 60 kb)
    reads = []
    for _ in range(n):
        c = int(rng.integers(0, 2)); L = int(rng.integers(3000, 12_000)); st = int(rng.integers(0, len(g[c]) - L))
        s = sim_reads.mutate(rng, g[c][st:st + L].copy(), float(rng.choice([0.005, 0.03, 0.08])))
        u = rng.random()
        if u < 0.1:
            s = np.concatenate([s[:L // 2], sim_reads.BASES[rng.integers(0, 4, int(rng.integers(500, 3000)))], s[L // 2:]])
        elif u < 0.25:
            s = np.concatenate([s[:L // 3], sim_reads.revcomp(s[L // 3:L // 3 + 1200]), s[L // 3 + 1200:]])
        reads.append(bytes(sim_reads.revcomp(s) if rng.random() < 0.5 else s))
    return [bytes(c) for c in g], reads


# ---------------------------------------------------------------- the DP at the presets' scores
def ksw_params():
    """The four presets' (q, e, q2, e2) with their a / b matrices (options.c:113, 126-130), from this project's own option call."""
    out = []
    for name in PRESETS:
        o = mm.align_opt(name)
        out.append(mm.ksw_param(q=o.q, e=o.e, q2=o.q2, e2=o.e2, a=o.a, b=o.b, sc_ambi=o.sc_ambi))
    return out


def golden_ksw():
    """tests/golden/ksw/extd2_asm_cases.npz in the layout of ksw_cases.golden_batches: per preset (param, jobs, queries, targets, (records, words))."""
    g = np.load(KSW_GOLD)
    out = []
    for k, row in enumerate(g["params"]):
        p = mm.ksw_param(q=int(row[26]), e=int(row[27]), q2=int(row[28]), e2=int(row[29]), mat=list(row[1:26]), m=int(row[0]))
        cut = lambda name, ends: g[name][int(g[ends][k]):int(g[ends][k + 1])]
        out.append((p, cut("jobs", "job_end"), cut("queries", "q_end"), cut("targets", "t_end"), (cut("res", "job_end"), cut("words", "word_end"))))
    return out
