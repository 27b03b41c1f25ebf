"""Cases for the base-level alignment of hits (mm2gb_align_regs_*): the batches that exercise each path of mm_align_skeleton, the reference's own
mm_align_skeleton through ctypes (oracle/_ref/libminimap2ref.so, where it is built) fed the same records and anchors as this project's call, the
committed fixtures (tests/golden/align) and the exact comparison.  Test infrastructure only: imported by tests/test_align_cpu.py,
tests/test_gpu_align.py, tests/tools/gen_golden_align.py and profiles/align_rate.py."""
import copy
import ctypes as C
import json
import os

import numpy as np

import golden_io
import mm2gb_amd as mm
import orc
import sim_reads

GOLD = os.path.join(golden_io.GOLD, "align")
DATA = os.path.join(golden_io.GOLD, "data")
REF_LIB = os.path.join(orc.REF_DIR, "libminimap2ref.so")
PRESETS = {"map-ont": dict(k=15, w=10, hpc=False), "map-pb": dict(k=19, w=10, hpc=True)}
# what the reference's answers on the fixture batches must contain (counts of mm.ALN_COUNTS summed over the batches, plus n_ambi): at least one of each
MUST_HAVE = ("gap_skipped", "fill_one_pass", "fill_two_pass", "split", "reads_3_rounds", "split_refused", "inv", "left_end", "left_short", "right_end", "right_short",
             "left_at_0", "rev_chain", "seam_merged", "lead_gap_cut", "filtered", "dp_max_rewritten", "hpc_moved", "over_sw_mat", "n_ambi")


# ---------------------------------------------------------------- the reference through ctypes
class _IdxOpt(C.Structure):
    _fields_ = [("k", C.c_short), ("w", C.c_short), ("flag", C.c_short), ("bucket_bits", C.c_short), ("mini_batch_size", C.c_int64), ("batch_size", C.c_uint64)]


class MapOpt(C.Structure):
    """mm_mapopt_t (minimap.h:128-186)."""
    _fields_ = ([("flag", C.c_int64)] + [(k, C.c_int) for k in "seed sdust_thres max_qlen bw bw_long max_gap max_gap_ref max_frag_len max_chain_skip max_chain_iter min_cnt min_chain_score".split()] +
                [("chain_gap_scale", C.c_float), ("chain_skip_scale", C.c_float), ("rmq_size_cap", C.c_int), ("rmq_inner_dist", C.c_int), ("rmq_rescue_size", C.c_int),
                 ("rmq_rescue_ratio", C.c_float), ("mask_level", C.c_float), ("mask_len", C.c_int), ("pri_ratio", C.c_float), ("best_n", C.c_int), ("alt_drop", C.c_float)] +
                [(k, C.c_int) for k in "a b q e q2 e2 sc_ambi noncan junc_bonus zdrop zdrop_inv end_bonus min_dp_max min_ksw_len anchor_ext_len anchor_ext_shift".split()] +
                [("max_clip_ratio", C.c_float), ("rank_min_len", C.c_int), ("rank_frac", C.c_float), ("pe_ori", C.c_int), ("pe_bonus", C.c_int), ("mid_occ_frac", C.c_float),
                 ("q_occ_frac", C.c_float)] + [(k, C.c_int32) for k in "min_mid_occ max_mid_occ mid_occ max_occ max_max_occ occ_dist".split()] +
                [("mini_batch_size", C.c_int64), ("max_sw_mat", C.c_int64), ("cap_kalloc", C.c_int64), ("split_prefix", C.c_char_p), ("gpu_chain_max_reads", C.c_int),
                 ("gpu_chain_max_anchors", C.c_size_t), ("gpu_chain_min_n", C.c_int), ("gpu_config_file", C.c_char * 1024)])


class _Extra(C.Structure):
    _fields_ = [("capacity", C.c_uint32), ("dp_score", C.c_int32), ("dp_max", C.c_int32), ("dp_max2", C.c_int32), ("ambi_strand", C.c_uint32), ("n_cigar", C.c_uint32)]


REG1_BYTES = 80          # mm_reg1_t: the 72 bytes of mm2gb_reg_t, then the pointer p


def ref_available():
    return os.path.exists(REF_LIB)


_ref = None
_libc = C.CDLL(None)
_libc.malloc.restype = C.c_void_p
_libc.malloc.argtypes = [C.c_size_t]
_libc.free.argtypes = [C.c_void_p]


def ref_lib():
    global _ref
    if _ref is None:
        L = C.CDLL(REF_LIB)
        L.mm_idx_str.restype = C.c_void_p
        L.mm_idx_str.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p)]
        L.mm_idx_destroy.argtypes = [C.c_void_p]
        L.mm_idx_destroy.restype = None
        L.mm_set_opt.argtypes = [C.c_char_p, C.POINTER(_IdxOpt), C.POINTER(MapOpt)]
        L.mm_mapopt_update.argtypes = [C.POINTER(MapOpt), C.c_void_p]
        L.mm_mapopt_update.restype = None
        L.mg_lchain_dp.restype = C.c_void_p
        L.mg_lchain_dp.argtypes = [C.c_int] * 7 + [C.c_float, C.c_float, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_void_p), C.c_void_p]
        L.mm_gen_regs.restype = C.c_void_p
        L.mm_gen_regs.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        L.mm_set_parent.restype = None
        L.mm_set_parent.argtypes = [C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float]
        L.mm_select_sub.restype = None
        L.mm_select_sub.argtypes = [C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_void_p]
        L.mm_align_skeleton.restype = C.c_void_p
        L.mm_align_skeleton.argtypes = [C.c_void_p, C.POINTER(MapOpt), C.c_void_p, C.c_int, C.c_char_p, C.POINTER(C.c_int), C.c_void_p, C.c_void_p]
        C.c_int.in_dll(L, "mm_verbose").value = 0
        _ref = L
    return _ref


class RefIndex:
    """mm_idx_str on the reference sequences, and the preset's options after mm_mapopt_update."""

    def __init__(self, refs, preset, **opt_kw):
        L = ref_lib()
        self.refs = [bytes(s) for s in refs]
        p = PRESETS[preset]
        self._seqs = (C.c_char_p * len(self.refs))(*self.refs)
        self._names = (C.c_char_p * len(self.refs))(*[f"ref{k}".encode() for k in range(len(self.refs))])
        self.io, self.mo = _IdxOpt(), MapOpt()
        assert L.mm_set_opt(None, C.byref(self.io), C.byref(self.mo)) == 0 and L.mm_set_opt(preset.encode(), C.byref(self.io), C.byref(self.mo)) == 0
        assert (self.io.k, self.io.w, bool(self.io.flag & 1)) == (p["k"], p["w"], p["hpc"])
        self.mi = L.mm_idx_str(self.io.w, self.io.k, self.io.flag & 1, self.io.bucket_bits, len(self.refs), self._seqs, self._names)
        L.mm_mapopt_update(C.byref(self.mo), self.mi)
        for k, v in opt_kw.items():
            setattr(self.mo, k, v)

    def close(self):
        if self.mi:
            ref_lib().mm_idx_destroy(self.mi)
            self.mi = None


def opt_from_ref(mo):
    """The mm2gb_align_opt_t that holds a mm_mapopt_t's values, field by field (nothing taken from this project's defaults)."""
    o = mm.AlignOpt()
    for k, _ in mm.AlignOpt._fields_:
        setattr(o, k, getattr(mo, k))
    return o


def read_hash(r):
    return (r * 2654435761 + 12345) & 0xffffffff


def ref_prepare(ri, read, anchors, r_id):
    """Steps 4-5: the reference's mg_lchain_dp, mm_gen_regs, mm_set_parent and mm_select_sub (map.c:336-337, 694, 737) on this project's anchors.
    Returns (regs pointer, n_regs, anchors pointer, snapshot of the records, snapshot of the anchors); the pointers are the reference's (malloc'd)."""
    L, mo = ref_lib(), ri.mo
    a = np.ascontiguousarray(anchors, dtype=np.uint64).reshape(-1, 2)
    n_u, u_ptr = C.c_int(0), C.c_void_p(0)
    if len(a) == 0:
        return None, 0, None, np.zeros(0, mm.REG_DTYPE), np.zeros((0, 2), np.uint64)
    buf = _libc.malloc(a.nbytes)
    C.memmove(buf, a.ctypes.data, a.nbytes)
    pen_gap, pen_skip = np.float32(mo.chain_gap_scale * 0.01 * ri.io.k), np.float32(mo.chain_skip_scale * 0.01 * ri.io.k)
    out = L.mg_lchain_dp(mo.max_gap, mo.max_gap, mo.bw, mo.max_chain_skip, mo.max_chain_iter, mo.min_cnt, mo.min_chain_score, pen_gap, pen_skip, 0, 1, len(a), buf,
                         C.byref(n_u), C.byref(u_ptr), None)
    if n_u.value == 0:
        return None, 0, None, np.zeros(0, mm.REG_DTYPE), np.zeros((0, 2), np.uint64)
    regs = L.mm_gen_regs(None, read_hash(r_id), len(read), n_u.value, u_ptr, out, 0)
    n_out = int((np.ctypeslib.as_array(C.cast(u_ptr, C.POINTER(C.c_uint64)), shape=(n_u.value,)) & 0xffffffff).sum())
    _libc.free(u_ptr)
    n = C.c_int(n_u.value)
    L.mm_set_parent(None, mo.mask_level, mo.mask_len, n.value, regs, mo.a * 2 + mo.b, int(bool(mo.flag & 0x20000000)), mo.alt_drop)
    L.mm_select_sub(None, mo.pri_ratio, ri.io.k * 2, mo.best_n, 1, int(mo.max_gap * 0.8), C.byref(n), regs)
    return regs, n.value, out, _snap_regs(regs, n.value)[0], np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint64)), shape=(n_out, 2)).copy()


def _snap_regs(regs, n):
    """The leading 72 bytes of n mm_reg1_t records, and their p pointers."""
    if n == 0:
        return np.zeros(0, mm.REG_DTYPE), []
    raw = np.ctypeslib.as_array(C.cast(regs, C.POINTER(C.c_uint8)), shape=(n * REG1_BYTES,)).reshape(n, REG1_BYTES)
    return raw[:, :72].copy().view(mm.REG_DTYPE).reshape(-1), [int(x) for x in raw[:, 72:80].copy().view(np.uint64).reshape(-1)]


def ref_align(ri, read, regs, n_regs, a_ptr):
    """Steps 6-7: mm_align_skeleton, then the records, one ALN_DTYPE row per record and the read's CIGAR words.  Frees what the reference made."""
    L = ref_lib()
    if n_regs == 0:
        return np.zeros(0, mm.REG_DTYPE), np.zeros(0, mm.ALN_DTYPE), np.zeros(0, np.uint32)
    n = C.c_int(n_regs)
    regs = L.mm_align_skeleton(None, C.byref(ri.mo), ri.mi, len(read), bytes(read), C.byref(n), regs, a_ptr)
    rec, ps = _snap_regs(regs, n.value)
    aln = np.zeros(n.value, mm.ALN_DTYPE)
    words, total = [], 0
    for k, p in enumerate(ps):
        if not p:
            aln[k]["cigar_off"] = -1
            continue
        x = _Extra.from_address(p)
        aln[k] = (x.dp_score, x.dp_max, x.dp_max2, x.ambi_strand & 0x3fffffff, x.ambi_strand >> 30, x.n_cigar, total)
        if x.n_cigar:
            words.append(np.ctypeslib.as_array(C.cast(p + C.sizeof(_Extra), C.POINTER(C.c_uint32)), shape=(x.n_cigar,)).copy())
        total += x.n_cigar
        _libc.free(p)
    _libc.free(regs)
    _libc.free(a_ptr)
    return rec, aln, (np.concatenate(words) if words else np.zeros(0, np.uint32))


# ---------------------------------------------------------------- this project's anchors, and a batch
def own_anchors(refs, reads, preset, threads=4):
    """Step 3: every read's anchors from this project's seeding path (index, matches, collect_seed_hits with its sort)."""
    p = PRESETS[preset]
    with mm.SeedIndex(refs, k=p["k"], w=p["w"], hpc=p["hpc"], threads=threads) as ix:
        mid_occ = ix.mid_occ()
        recs = [ix.matches(s, mid_occ) for s in reads]
    return mm.collect_seeds_host(0, recs, threads=threads) if recs else []


def ref_batch(refs, reads, preset, anchors=None, **opt_kw):
    """A batch through the harness: dict(opt, k, hpc, refs, reads, regs, anchors) -- the call's input -- and `want`: per read (regs, aln, words)."""
    ri = RefIndex(refs, preset, **opt_kw)
    try:
        anchors = own_anchors(refs, reads, preset) if anchors is None else anchors
        regs_in, a_in, want = [], [], []
        for r, (s, a) in enumerate(zip(reads, anchors)):
            regs, n, a_ptr, snap_r, snap_a = ref_prepare(ri, s, a, r)
            regs_in.append(snap_r); a_in.append(snap_a)
            want.append(ref_align(ri, s, regs, n, a_ptr))
        return dict(opt=opt_from_ref(ri.mo), k=ri.io.k, hpc=PRESETS[preset]["hpc"], refs=[bytes(s) for s in refs], reads=[bytes(s) for s in reads], regs=regs_in, anchors=a_in), want
    finally:
        ri.close()


def run_host(b, threads=4, **kw):
    return mm.align_regs_host(b["opt"], b["k"], b["hpc"], b["refs"], b["reads"], b["regs"], b["anchors"], threads=threads, **kw)


def run_gpu(eng, b):
    return eng.align_regs(b["opt"], b["k"], b["hpc"], b["refs"], b["reads"], b["regs"], b["anchors"])


def assert_same(got, want, what):
    """Exact: the number and order of every read's records, every field of both structures, where the words lie and every word."""
    assert len(got) == len(want), f"{what}: {len(got)} reads against {len(want)}"
    for r, ((gr, ga, gw), (wr, wa, ww)) in enumerate(zip(got, want)):
        assert len(gr) == len(wr), f"{what}: read {r}: {len(gr)} records against {len(wr)}"
        for name in mm.REG_DTYPE.names:
            g, w = (gr[name].view(np.uint32), wr[name].view(np.uint32)) if name == "div" else (gr[name], wr[name])
            bad = np.flatnonzero(g != w)
            assert len(bad) == 0, f"{what}: read {r}: record {int(bad[0])} differs in {name}: got {gr[bad[0]]} want {wr[bad[0]]}"
        for name in mm.ALN_DTYPE.names:
            bad = np.flatnonzero(ga[name] != wa[name])
            assert len(bad) == 0, f"{what}: read {r}: record {int(bad[0])} differs in {name}: got {ga[bad[0]]} want {wa[bad[0]]}"
        assert len(gw) == len(ww), f"{what}: read {r}: {len(gw)} CIGAR words against {len(ww)}"
        bad = np.flatnonzero(gw != ww)
        assert len(bad) == 0, f"{what}: read {r}: {len(bad)} CIGAR words differ, first at {int(bad[0])}: got {mm.cigar_string(gw[bad[0]:bad[0] + 4])} want {mm.cigar_string(ww[bad[0]:bad[0] + 4])}"


# ---------------------------------------------------------------- inputs that reach each path
def _b(x):
    return bytes(np.asarray(x, np.uint8))


def genome(seed=5, n=60_000):
    """About 60 kb from sim_reads.make_genome: two sequences, two repeat families (no tandem array: its anchors alone would outweigh every other fixture), a run of N in the first."""
    rng = np.random.default_rng(seed)
    chrs = sim_reads.make_genome(rng, n_chr=2, chr_len=n // 2, n_rep_families=2, rep_len=600, copies=6, tandem=0)
    chrs[0][12_000:12_007] = ord("N")
    cp = chrs[0][8500:10_000].copy()                                              # a second copy of 1.5 kb, 1 % apart: two hits of nearly equal score
    mut = rng.random(len(cp)) < 0.01
    cp[mut] = sim_reads.BASES[rng.integers(0, 4, int(mut.sum()))]
    chrs[1][10_500:12_000] = cp
    return [_b(c) for c in chrs]


def path_reads(refs, seed, hpc=False, n_plain=10):
    """Reads of 1-6 kb built to reach mm_align_skeleton's paths (the names say which); err: the simulator's rate."""
    rng = np.random.default_rng(seed)
    g = [np.frombuffer(s, np.uint8) for s in refs]
    err = 0.06 if not hpc else 0.03
    mut = lambda x, e=err: sim_reads.mutate(rng, np.array(x), e)
    rnd = lambda n: sim_reads.BASES[rng.integers(0, 4, n)]
    out = []
    for _ in range(n_plain):                                                      # plain reads, either strand, one across the run of N
        c = int(rng.integers(0, len(g))); L = int(rng.integers(1000, 6000)); st = int(rng.integers(0, len(g[c]) - L))
        s = mut(g[c][st:st + L])
        out.append(("plain", sim_reads.revcomp(s) if rng.random() < 0.5 else s))
    out.append(("at_ref_start", mut(g[0][0:2500], 0.02)))                         # a chain that starts at reference position 0
    out.append(("two_copies", mut(g[0][8600:9900], 0.03)))                        # mm_update_dp_max rewrites dp_max
    out.append(("exact_ends", np.array(g[1][3000:5000])))                         # both extensions reach the read's ends
    out.append(("across_N", mut(g[0][11_000:13_500])))
    s = mut(g[0][14_000:16_000]); s[700:704] = ord("N"); out.append(("read_N", s))
    out.append(("junk_mid", np.concatenate([mut(g[1][6000:8000]), rnd(3000), mut(g[1][8000:10_000])])))               # a z-drop that splits
    out.append(("junk_twice", np.concatenate([mut(g[0][17_000:18_500]), rnd(3000), mut(g[0][18_500:20_000]), rnd(3000), mut(g[0][20_000:21_500])])))
    for n in (30, 40, 50, 60):                                                    # too few anchors remain behind the drop for a split
        out.append(("junk_short_tail", np.concatenate([mut(g[1][14_000:16_000]), rnd(800), np.array(g[1][16_800:16_800 + n])])))     # junk IN PLACE of 800 bases: one diagonal
    out.append(("inversion", np.concatenate([mut(g[0][22_000:24_000]), sim_reads.revcomp(mut(g[0][24_000:25_000])), mut(g[0][25_000:27_000])])))
    out.append(("inversion_rev", sim_reads.revcomp(np.concatenate([mut(g[1][20_000:22_000]), sim_reads.revcomp(mut(g[1][22_000:23_000])), mut(g[1][23_000:25_000])]))))
    out.append(("clipped_ends", np.concatenate([rnd(400), mut(g[0][27_500:29_500]), rnd(400)])))                      # extensions that stop short
    out.append(("big_deletion", np.concatenate([mut(g[1][25_000:26_500]), mut(g[1][27_300:28_800])])))                # a long gap inside one fill
    out.append(("big_insertion", np.concatenate([mut(g[0][5000:6500]), rnd(700), mut(g[0][6500:8000])])))
    return [n for n, _ in out], [_b(s) for _, s in out]


def fixture_batches():
    """name -> (refs, reads, preset, option overrides): the batches tests/tools/gen_golden_align.py records."""
    refs = genome()
    hp = [hpc_genome(9), hpc_genome(10)]
    inv_t, inv_q = read_fasta(os.path.join(DATA, "t-inv.fa")), read_fasta(os.path.join(DATA, "q-inv.fa"))
    return {
        "ont": (refs, path_reads(refs, 21)[1], "map-ont", {}),
        "pb": (hp, path_reads(hp, 22, hpc=True, n_plain=6)[1], "map-pb", {}),
        "small_mat": (refs, small_reads(refs, 23), "map-ont", dict(max_sw_mat=10_000)),
        "end_bonus": (refs, end_reads(refs, 24), "map-ont", dict(end_bonus=20)),
        "inv_pair": (inv_t, inv_q, "map-ont", {}),
    }


def small_reads(refs, seed):
    """Two reads of about 1.2 kb, one on the reverse strand: with max_sw_mat = 10 000 every fill of 200 x 200 is over the limit and ends its chain."""
    rng = np.random.default_rng(seed)
    g = [np.frombuffer(s, np.uint8) for s in refs]
    return [_b(sim_reads.mutate(rng, np.array(g[0][1000:2200]), 0.05)), _b(sim_reads.revcomp(sim_reads.mutate(rng, np.array(g[1][5000:6300]), 0.05)))]


def end_reads(refs, seed):
    """Reads whose ends an end bonus can reach: exact ends, a few unrelated bases at either end (the extension then ends in a gap), long unrelated ends."""
    rng = np.random.default_rng(seed)
    g = [np.frombuffer(s, np.uint8) for s in refs]
    rnd = lambda n: sim_reads.BASES[rng.integers(0, 4, n)]
    out = [np.array(g[1][3000:5000]), np.array(g[0][0:1500])]
    for n in (3, 4, 5, 6):
        body = sim_reads.mutate(rng, np.array(g[0][2000 + 1000 * n:3500 + 1000 * n]), 0.03)
        out.append(np.concatenate([rnd(n), body, rnd(n)]))
        out.append(sim_reads.revcomp(np.concatenate([rnd(n), body])))
    out.append(np.concatenate([rnd(300), np.array(g[1][9000:10_500]), rnd(300)]))
    return [_b(s) for s in out]


def hpc_genome(seed=9, n=30_000):
    """A sequence with homopolymer runs (tests/hpc_cases.hpc_seq), so that anchors end inside runs under the HPC preset."""
    import hpc_cases
    return hpc_cases.hpc_seq(np.random.default_rng(seed), n, p_n=0.0005, mixed_case=False)


def read_fasta(path):
    out, cur = [], []
    for line in open(path, "rb"):
        if line.startswith(b">"):
            if cur:
                out.append(b"".join(cur))
            cur = []
        else:
            cur.append(line.strip())
    if cur:
        out.append(b"".join(cur))
    return out


def random_batch(seed, preset, n_reads=300):
    """A fresh batch for the live comparison: plain reads of 1-6 kb, a tenth of them with junk or an inverted block in the middle."""
    hpc = PRESETS[preset]["hpc"]
    refs = [hpc_genome(seed + 100), hpc_genome(seed + 101)] if hpc else genome(seed + 100)
    rng = np.random.default_rng(seed)
    g = [np.frombuffer(s, np.uint8) for s in refs]
    reads = []
    for _ in range(n_reads):
        c = int(rng.integers(0, len(g))); L = int(rng.integers(1000, 6000)); st = int(rng.integers(0, len(g[c]) - L))
        s = sim_reads.mutate(rng, np.array(g[c][st:st + L]), float(rng.choice([0.02, 0.06, 0.1])))
        u = rng.random()
        if u < 0.05:
            s = np.concatenate([s[:L // 2], sim_reads.BASES[rng.integers(0, 4, int(rng.integers(500, 3500)))], s[L // 2:]])
        elif u < 0.1 and L > 3000:
            s = np.concatenate([s[:L // 3], sim_reads.revcomp(s[L // 3:L // 3 + 900]), s[L // 3 + 900:]])
        reads.append(_b(sim_reads.revcomp(s) if rng.random() < 0.5 else s))
    return refs, reads


def refusals(b):
    """(what the error names, the batch that is refused)"""
    def with_opt(**kw):
        c = dict(b)
        c["opt"] = copy.copy(b["opt"])
        for k, v in kw.items():
            setattr(c["opt"], k, v)
        return c
    out = [(name, with_opt(flag=b["opt"].flag | bit)) for name, bit in (("MM_F_SPLICE", mm.F_SPLICE), ("MM_F_SR", mm.F_SR), ("MM_F_QSTRAND", mm.F_QSTRAND), ("MM_F_EQX", mm.F_EQX))]
    out.append(("ksw_extz2_sse", with_opt(q2=b["opt"].q, e2=b["opt"].e)))
    out.append(("max_sw_mat", with_opt(max_sw_mat=0)))
    out.append(("max_sw_mat", with_opt(max_sw_mat=100_000_001)))
    c = dict(b); c["regs"] = [x.copy() for x in b["regs"]]
    k = next(i for i, x in enumerate(c["regs"]) if len(x))
    c["regs"][k]["cnt"][0] = len(b["anchors"][k]) + 1
    out.append(("leaves the read's anchors", c))
    c = dict(b); c["anchors"] = [x.copy() for x in b["anchors"]]
    c["anchors"][k][0, 1] |= np.uint64(1 << 48)
    out.append(("multi-segment", c))
    c = dict(b); c["regs"] = [x.copy() for x in b["regs"]]
    c["regs"][k]["flags"][0] |= 1 << 15
    out.append(("multi-segment", c))
    return out


# ---------------------------------------------------------------- the committed fixtures
def save_batch(path, b, want):
    o = b["opt"]
    cat = lambda xs, dt: np.concatenate(xs) if len(xs) else np.zeros(0, dt)
    ends = lambda xs: np.cumsum([0] + [len(x) for x in xs]).astype(np.int64)
    np.savez_compressed(path, opt=json.dumps({k: getattr(o, k) for k, _ in mm.AlignOpt._fields_}), k=b["k"], hpc=int(b["hpc"]),
                        refs=np.frombuffer(b"".join(b["refs"]), np.uint8), ref_end=ends(b["refs"]), reads=np.frombuffer(b"".join(b["reads"]), np.uint8), read_end=ends(b["reads"]),
                        regs=cat(b["regs"], mm.REG_DTYPE), reg_end=ends(b["regs"]), anchors=cat(b["anchors"], np.uint64).reshape(-1, 2), a_end=ends(b["anchors"]),
                        w_regs=cat([w[0] for w in want], mm.REG_DTYPE), w_aln=cat([w[1] for w in want], mm.ALN_DTYPE), w_end=ends([w[0] for w in want]),
                        w_words=cat([w[2] for w in want], np.uint32), w_word_end=ends([w[2] for w in want]))


def load_batch(name):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    cut = lambda arr, end: [z[arr][int(z[end][i]):int(z[end][i + 1])] for i in range(len(z[end]) - 1)]
    o = mm.AlignOpt()
    for k, v in json.loads(str(z["opt"])).items():
        setattr(o, k, v)
    b = dict(opt=o, k=int(z["k"]), hpc=bool(z["hpc"]), refs=[x.tobytes() for x in cut("refs", "ref_end")], reads=[x.tobytes() for x in cut("reads", "read_end")],
             regs=cut("regs", "reg_end"), anchors=cut("anchors", "a_end"))
    want = list(zip(cut("w_regs", "w_end"), cut("w_aln", "w_end"), cut("w_words", "w_word_end")))
    return b, want


def dump_batch(path, b, want):
    """A batch as the flat file tests/tools/align_replay.cpp reads, with a digest (FNV-1a) of the expected record offsets, records and words."""
    ends = lambda xs: np.cumsum([0] + [len(x) for x in xs]).astype(np.int64)
    regs = np.concatenate(b["regs"]) if b["regs"] else np.zeros(0, mm.REG_DTYPE)
    anchors = np.concatenate([np.asarray(a, np.uint64).reshape(-1, 2) for a in b["anchors"]]) if b["anchors"] else np.zeros((0, 2), np.uint64)
    h = 1469598103934665603
    for blob in (ends([w[0] for w in want]).tobytes(), b"".join(w[0].tobytes() for w in want), b"".join(w[2].tobytes() for w in want)):
        for byte in blob:
            h = ((h ^ byte) * 1099511628211) & (2**64 - 1)
    with open(path, "wb") as f:
        f.write(np.array([b["k"], int(b["hpc"]), len(b["refs"]), len(b["reads"]), len(regs), len(anchors), 0, C.sizeof(mm.AlignOpt)], np.int64).tobytes()[:48])
        f.write(np.array([h], np.uint64).tobytes() + np.array([C.sizeof(mm.AlignOpt)], np.int64).tobytes())
        f.write(bytes(b["opt"]))
        f.write(np.array([len(s) for s in b["refs"]], np.int32).tobytes() + np.array([len(s) for s in b["reads"]], np.int32).tobytes())
        f.write(ends(b["regs"]).tobytes() + ends(b["anchors"]).tobytes() + regs.tobytes() + anchors.tobytes() + b"".join(b["refs"]) + b"".join(b["reads"]))


def golden_names():
    return sorted(json.load(open(os.path.join(GOLD, "meta.json")))["batches"])


def golden_meta():
    return json.load(open(os.path.join(GOLD, "meta.json")))
