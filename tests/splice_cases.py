"""Cases for the spliced alignment of hits (mm2gb_align_regs_splice_*): a small genome with genes on both strands, reads cut from their
transcripts and built to reach each branch mm_align_skeleton takes under MM_F_SPLICE, the reference's own mm_align_skeleton through
align_cases' ctypes harness with the splice preset's options, the committed fixtures (tests/golden/splice) and their loader.  Deterministic,
numpy only.  Test infrastructure: imported by tests/test_splice_align_cpu.py, tests/test_gpu_splice.py and tests/tools/gen_golden_splice.py."""
import ctypes as C
import json
import os

import numpy as np

import align_cases as ac
import golden_io
import mm2gb_amd as mm
import sim_reads

GOLD = os.path.join(golden_io.GOLD, "splice")
K, W = 15, 5
MAX_SW_MAT = 100_000_000          # the stated departure: the preset's 0 (no limit) is mm_mapopt_init's own default here and in the reference run
# what the fixture batches together must have met (mm.SPLICE_COUNTS), over_sw_mat in the batch made for it alone
MUST_HAVE = ("trial_for_won", "trial_rev_won", "trial_tie_kept_0", "trial_tie_kept_1", "end_flt_head", "end_flt_tail", "end_flt_probe_kept", "left_ext_intron",
             "right_ext_intron", "fill_intron", "fill_two_pass", "split", "tail_other_strand", "n_seam_merged", "noncanonical_intron", "single_trial", "rev_chain",
             "over_sw_mat")
PAIR_APART = (560, 520, 580, 540)
BIG_INTRON = 60_000
BIG_FLANK = 1400                  # the exons on either side of the 60 kb intron
BIG_READ = 700                    # ... and the bases of each its read holds: were the whole read ONE fill, it would stay under MAX_SW_MAT (asserted in genes())


def _b(x):
    return bytes(np.asarray(x, np.uint8))


# ---------------------------------------------------------------- genome, genes, transcripts
def genes(seed=3, chr_lens=(230_000, 170_000, 260_000)):
    """(refs, genes): random sequences with genes planted; a gene is dict(chrom, strand, exons=[(start, end), ...]) in reference coordinates.
    Intron ends as the transcript's strand reads them: mostly GT..AG, some GC..AG and AT..AC, some left random.  Gene 0 holds the 60 kb intron."""
    rng = np.random.default_rng(seed)
    chrs = [sim_reads.BASES[rng.integers(0, 4, n)].copy() for n in chr_lens]
    out = []

    def plant(chrom, strand, start, exon_lens, intron_lens, kinds, kind="plain"):
        pos, exons = start, []
        for k, el in enumerate(exon_lens):
            exons.append((pos, pos + el))
            pos += el
            if k < len(intron_lens):
                s, e = pos, pos + intron_lens[k]
                don, acc = {"gtag": (b"GT", b"AG"), "gcag": (b"GC", b"AG"), "atac": (b"AT", b"AC"), "random": (None, None)}[kinds[k]]
                if don is not None:
                    if strand == "+":
                        chrs[chrom][s:s + 2] = np.frombuffer(don, np.uint8); chrs[chrom][e - 2:e] = np.frombuffer(acc, np.uint8)
                    else:                                                     # the transcript reads the other strand: its donor lies at the intron's end here
                        chrs[chrom][e - 2:e] = sim_reads.revcomp(np.frombuffer(don, np.uint8)); chrs[chrom][s:s + 2] = sim_reads.revcomp(np.frombuffer(acc, np.uint8))
                pos = e
        assert pos < len(chrs[chrom])
        out.append(dict(chrom=chrom, strand=strand, exons=exons, kind=kind))
        return pos

    # gene 0: the 60 kb intron between two long exons (a device job beyond the LDS-image class), then ordinary ones
    end = plant(0, "+", 2000, [BIG_FLANK, BIG_FLANK, 200, 150], [BIG_INTRON, 900, 300], ["gtag", "gtag", "gtag"])
    assert BIG_READ < 1500 and 2 * BIG_READ * (2 * BIG_READ + BIG_INTRON) < MAX_SW_MAT
    last_end = {0: end, 1: 0}
    kinds_all = ["gtag"] * 7 + ["gcag", "atac", "random"]
    for chrom, strand, start in ((0, "-", end + 3000), (0, "+", 110_000), (0, "-", 150_000), (0, "+", 190_000), (1, "+", 4000), (1, "-", 65_000), (1, "-", 100_000), (1, "+", 135_000)):
        assert start > last_end[chrom], "genes overlap"
        n_ex = int(rng.integers(4, 11))
        exon_lens = [int(x) for x in rng.integers(60, 401, n_ex)]
        exon_lens[int(rng.integers(0, n_ex))] = 400                           # room for a read inside one exon
        intron_lens = [int(x) for x in np.exp(rng.uniform(np.log(80), np.log(8000), n_ex - 1))]
        if strand == "+" and chrom == 1 and start == 4000:
            intron_lens[1] = 30_000
        last_end[chrom] = plant(chrom, strand, start, exon_lens, intron_lens, [kinds_all[int(rng.integers(0, len(kinds_all)))] for _ in range(n_ex - 1)])
    # chromosome 2: genes made for one branch each
    pos = 3000
    for strand in "+-+":                      # long first and last introns: the end anchors of a read with short end exons are probed (span < ln(gap) + shift)
        pos = plant(2, strand, pos, [300, 250, 300, 200, 300], [int(rng.integers(15_000, 25_000)), 400, 700, int(rng.integers(10_000, 20_000))], ["gtag"] * 4, "long_ends") + 3000
    for strand in "+-":                       # short introns between long exons: an extension can cross one
        pos = plant(2, strand, pos, [400, 400, 400], [85, 95], ["gtag"] * 2, "short_introns") + 3000
    for (sa, sb), apart in zip((("+", "-"), ("-", "+"), ("+", "+"), ("-", "-")), PAIR_APART):          # two genes a few hundred bases apart: a read of both and a diverged copy of those is one chain that a z-drop splits
        pos = plant(2, sa, pos, [300, 300], [500], ["gtag"], "pair_a") + apart
        pos = plant(2, sb, pos, [300, 300], [500], ["gtag"], "pair_b") + 3000
    for n in range(4):                        # the junction's 15-mer (7 + 8 bases) copied into the middle of the intron, exon 1 ending in AG and exon 2 beginning with GT,
        s0 = pos                              # and the read (seam_read) with a substitution on either side of it, so that the chain gains by the anchor there: it ends one
        pos = plant(2, "+", pos, [300, 300], [2000 + 100 * n], ["gtag"], "seam") + 2000          # stretch in N and begins the next with N (mm_append_cigar merges the two words)
        c = chrs[2]
        e1, e2 = s0 + 300, s0 + 300 + 2000 + 100 * n
        mid = e1 + 1000
        is_mini = lambda seq, at: at in {int(y) >> 1 & 0x7fffffff for y in mm.sketch(_b(seq), w=W, k=K)[:, 1]}
        for _ in range(200):                  # the free bases of the 15-mer are redrawn until it is a minimizer in the read and in the intron (mm.sketch)
            c[e1 - 7:e1 - 2] = sim_reads.BASES[rng.integers(0, 4, 5)]; c[e1 - 2:e1] = np.frombuffer(b"AG", np.uint8)
            c[e2:e2 + 2] = np.frombuffer(b"GT", np.uint8); c[e2 + 2:e2 + 8] = sim_reads.BASES[rng.integers(0, 4, 6)]
            c[mid - 7:mid] = c[e1 - 7:e1]; c[mid:mid + 8] = c[e2:e2 + 8]
            if is_mini(c[mid - 40:mid + 40], 47) and is_mini(seam_read(c, out[-1])[SEAM_HALF - 40:SEAM_HALF + 40], 47):
                break
        else:
            raise AssertionError("no junction 15-mer that is a minimizer on both sides")
    return [_b(c) for c in chrs], out


SEAM_HALF = 214          # the junction lies where the first gap fill ends: 200 bases (min_ksw_len) behind the first anchor's middle, which no anchor before it reaches


def seam_read(chrom, g):
    """A seam gene's read: the last / first SEAM_HALF bases of its two exons, the bases 8 before and 8 behind the junction substituted."""
    (_, e1), (s2, _) = g["exons"]
    return _subs(np.concatenate([np.asarray(chrom[e1 - SEAM_HALF:e1]), np.asarray(chrom[s2:s2 + SEAM_HALF])]), [SEAM_HALF - 8, SEAM_HALF + 8])


def plain(gs):
    return [g for g in gs if g["kind"] == "plain"]


def transcript(refs, g, lo=0, hi=None):
    """The bases of exons lo .. hi-1 joined, on the REFERENCE's strand (the transcript itself is its reverse complement for a '-' gene)."""
    ex = g["exons"][lo:hi]
    return np.concatenate([np.frombuffer(refs[g["chrom"]], np.uint8)[s:e] for s, e in ex])


def _subs(s, at):
    s = np.array(s)
    for p in at:
        s[p] = sim_reads.BASES[(int(np.searchsorted(sim_reads.BASES, s[p])) + 1) % 4]
    return s


def planted_reads(refs, gs, seed=31):
    """[(name, read)]: the reads built for one branch each (the names say which)."""
    rng = np.random.default_rng(seed)
    mut = lambda x, e=0.04: sim_reads.mutate(rng, np.array(x), e)
    rnd = lambda n: sim_reads.BASES[rng.integers(0, 4, n)]
    G = lambda c: np.frombuffer(refs[c], np.uint8)
    out = []
    # inside one exon: no intron, the two trials tie; exact and with substitutions, so that (qlen + dp_score) & 1 takes both values
    pl = plain(gs)
    for g in pl[1:5]:
        s, e = max(g["exons"], key=lambda x: x[1] - x[0])
        for n_sub, L in ((0, 300), (1, 300), (2, 301), (1, 330)):
            piece = _subs(G(g["chrom"])[s + 20:s + 20 + L], [40 + 70 * k for k in range(n_sub)])
            out.append(("one_exon", piece if len(out) % 2 else sim_reads.revcomp(piece)))
    # the 60 kb intron
    out.append(("big_intron", mut(transcript(refs, gs[0], 0, 2)[BIG_FLANK - BIG_READ:BIG_FLANK + BIG_READ], 0.02)))
    # whole and partial transcripts, both orientations, 0-8 % errors
    for g in pl[1:]:
        t = transcript(refs, g)
        for err in (0.0, 0.03, 0.08):
            lo = int(rng.integers(0, max(1, len(t) // 4))); hi = len(t) - int(rng.integers(0, max(1, len(t) // 4)))
            if hi - lo < 300:
                lo, hi = 0, len(t)
            s = mut(t[lo:hi][:3000], err) if err else np.array(t[lo:hi][:3000])
            out.append(("transcript", sim_reads.revcomp(s) if rng.random() < 0.5 else s))
    # a short first / last exon behind / before a long intron: the end filter probes the end anchor (span < ln(gap) + shift).  A lone 15-mer of
    # the end exon scores about 15 and is left out, 20 bases and more stay.  The 15-mer is one that is a minimizer on both sides (mm.sketch).
    for g in (g for g in gs if g["kind"] == "long_ends"):
        ex = g["exons"]
        for head in (True, False):
            (es, ee), body = (ex[0], transcript(refs, g, 1, 2)) if head else (ex[-1], transcript(refs, g, len(ex) - 2, len(ex) - 1))
            genome_mini = {int(y) >> 1 & 0x7fffffff for y in mm.sketch(_b(G(g["chrom"])[es:ee]), w=W, k=K)[:, 1]}
            n_lone = 0
            for p in sorted(genome_mini):                                        # p: the k-mer's last base within the exon
                piece = G(g["chrom"])[es + p - (K - 1):es + p + 1]
                s = np.concatenate([piece, body]) if head else np.concatenate([body, piece])
                at = K - 1 if head else len(s) - 1
                if p >= K - 1 and at in {int(y) >> 1 & 0x7fffffff for y in mm.sketch(_b(s), w=W, k=K)[:, 1]} and n_lone < 3:
                    out.append(("lone_end_kmer", s if n_lone % 2 else sim_reads.revcomp(s)))
                    n_lone += 1
            piece = G(g["chrom"])[ee - 24:ee] if head else G(g["chrom"])[es:es + 24]
            out.append(("short_end", np.concatenate([piece, body]) if head else np.concatenate([body, piece])))
    # extensions across an intron: 112 bases of the neighbouring exon with a substitution every 14th base (no 15-mer survives, so no anchor there)
    for g in (g for g in gs if g["kind"] == "short_introns"):
        ex = g["exons"]
        at = list(range(13, 112, 14))
        out.append(("left_ext_intron", np.concatenate([_subs(G(g["chrom"])[ex[0][1] - 112:ex[0][1]], at), transcript(refs, g, 1, 3)])))
        out.append(("right_ext_intron", np.concatenate([transcript(refs, g, 0, 2), _subs(G(g["chrom"])[ex[2][0]:ex[2][0] + 112], at)])))
    pa, pb = [g for g in gs if g["kind"] == "pair_a"], [g for g in gs if g["kind"] == "pair_b"]
    for n, (a, b2) in enumerate(zip(pa, pb)):            # the tail a z-drop splits off gets its own two trials: another transcript strand in the first two pairs
        between = np.array(G(2)[a["exons"][-1][1]:b2["exons"][0][0]])          # a copy with 55 % substitutions: no anchor, a score that falls by more than zdrop on
        hit = np.flatnonzero(rng.random(len(between)) < 0.55)                   # one diagonal (unrelated bases would go as I + N, which mm_test_zdrop's walk forgives)
        s = np.concatenate([mut(transcript(refs, a), 0.02), _subs(between, hit), mut(transcript(refs, b2), 0.02)])
        out.append(("pair", sim_reads.revcomp(s) if n == 1 else s))
    for g in (g for g in gs if g["kind"] == "seam"):
        out.append(("seam", seam_read(G(2), g)))
    # chimeric reads: part of one gene, unrelated bases, part of the next gene downstream (a z-drop splits the chain; the tail gets its own trials);
    # genes 1 / 2 and 3 / 4 lie on opposite strands, so head and tail differ in transcript strand
    for a, b2 in ((1, 2), (2, 3), (3, 4), (6, 7)):
        ta, tb = transcript(refs, pl[a])[-700:], transcript(refs, pl[b2])[:700]
        s = np.concatenate([mut(ta, 0.02), rnd(900), mut(tb, 0.02)])
        out.append(("chimeric", s if a % 2 else sim_reads.revcomp(s)))
    ta = transcript(refs, pl[5])                                                # unrelated bases IN PLACE of bases inside one long transcript
    if len(ta) > 1400:
        out.append(("junk_mid", np.concatenate([ta[:600], rnd(600), ta[1200:]])))
    # N in the read
    s = np.array(transcript(refs, pl[8])[:1200]); s[400:403] = ord("N")
    out.append(("read_N", s))
    return out


def reads_for(refs, gs, seed, n_random=0):
    rng = np.random.default_rng(seed + 1000)
    out = [s for _, s in planted_reads(refs, gs, seed)]
    for _ in range(n_random):
        out.append(random_read(rng, refs, gs))
    return [_b(s) for s in out]


def random_read(rng, refs, gs):
    g = gs[int(rng.integers(1, len(gs)))]
    t = transcript(refs, g)
    L = int(rng.integers(min(300, len(t)), min(3000, len(t)) + 1)); st = int(rng.integers(0, len(t) - L + 1))
    s = sim_reads.mutate(rng, np.array(t[st:st + L]), float(rng.choice([0.0, 0.02, 0.05, 0.08])))
    if rng.random() < 0.06:
        s = np.concatenate([s[:len(s) // 2], sim_reads.BASES[rng.integers(0, 4, int(rng.integers(300, 900)))], s[len(s) // 2:]])
    return sim_reads.revcomp(s) if rng.random() < 0.5 else s


def random_batch(seed, n_reads=300):
    """A fresh batch for the live comparison."""
    refs, gs = genes(seed + 50)
    rng = np.random.default_rng(seed)
    return refs, [_b(random_read(rng, refs, gs)) for _ in range(n_reads)]


# option sets of the fixture batches: name -> (preset, overrides of mm_mapopt_t fields; flag_clear / flag_set change the flag word)
OPTION_SETS = {
    "default": ("splice", {}),
    "hq": ("splice:hq", {}),
    "for_only": ("splice", dict(flag_clear=mm.F_SPLICE_REV)),
    "rev_only": ("splice", dict(flag_clear=mm.F_SPLICE_FOR)),
    "no_flank": ("splice", dict(flag_clear=mm.F_SPLICE_FLANK)),
    "no_end_flt": ("splice", dict(flag_set=mm.F_NO_END_FLT)),
    "small_mat": ("splice", dict(max_sw_mat=200_000)),
}


def fixture_batches():
    """(refs, {name: (reads, preset, overrides)}): the batches tests/tools/gen_golden_splice.py records.  "default" holds every planted read and ten
    random ones; the other option sets every read built for a branch (without the 60 kb intron) and every third of the rest; "small_mat" a few reads,
    whose intron fills are all over its limit."""
    refs, gs = genes()
    named = planted_reads(refs, gs)
    rng = np.random.default_rng(77)
    every = [_b(s) for _, s in named] + [_b(random_read(rng, refs, gs)) for _ in range(10)]
    some = [_b(s) for i, (n, s) in enumerate(named) if n != "big_intron" and (n not in ("transcript", "one_exon") or i % 3 == 0)]
    few = [_b(s) for n, s in named if n in ("pair", "read_N", "short_end")] + [_b(s) for n, s in named if n == "transcript"][:6]
    return refs, {name: ((every if name == "default" else few if name == "small_mat" else some), preset, kw) for name, (preset, kw) in OPTION_SETS.items()}


# ---------------------------------------------------------------- the reference through align_cases' harness
class RefIndex(ac.RefIndex):
    """mm_idx_str with the preset's k and w, and mm_set_opt(preset) with max_sw_mat = MAX_SW_MAT (the stated departure) and the overrides."""

    def __init__(self, refs, preset="splice", flag_clear=0, flag_set=0, **opt_kw):
        L = ac.ref_lib()
        self.refs = [bytes(s) for s in refs]
        self._seqs = (C.c_char_p * len(self.refs))(*self.refs)
        self._names = (C.c_char_p * len(self.refs))(*[f"ref{k}".encode() for k in range(len(self.refs))])
        self.io, self.mo = ac._IdxOpt(), ac.MapOpt()
        assert L.mm_set_opt(None, C.byref(self.io), C.byref(self.mo)) == 0 and L.mm_set_opt(preset.encode(), C.byref(self.io), C.byref(self.mo)) == 0
        assert (self.io.k, self.io.w, self.io.flag & 1) == (K, W, 0)
        self.preset_values = {k: getattr(self.mo, k) for k, _ in ac.MapOpt._fields_ if k not in ("split_prefix", "gpu_config_file")}
        self.mi = L.mm_idx_str(self.io.w, self.io.k, 0, self.io.bucket_bits, len(self.refs), self._seqs, self._names)
        L.mm_mapopt_update(C.byref(self.mo), self.mi)
        self.mo.max_sw_mat = MAX_SW_MAT
        self.mo.flag = (self.mo.flag & ~flag_clear) | flag_set
        for k, v in opt_kw.items():
            setattr(self.mo, k, v)


def opt_from_ref(mo):
    """The mm2gb_align_splice_opt_t that holds a mm_mapopt_t's values, field by field."""
    o = mm.AlignSpliceOpt()
    for k, _ in mm.AlignOpt._fields_:
        setattr(o.base, k, getattr(mo, k))
    for k, _ in mm.AlignSpliceOpt._fields_[1:]:
        setattr(o, k, getattr(mo, k))
    return o


def ref_prepare(ri, read, anchors, r_id):
    """align_cases.ref_prepare with map.c's chaining arguments under MM_F_SPLICE: max_dist_x = max_gap_ref, max_dist_y = max_gap, is_cdna = 1."""
    L, mo = ac.ref_lib(), ri.mo
    a = np.ascontiguousarray(anchors, dtype=np.uint64).reshape(-1, 2)
    n_u, u_ptr = C.c_int(0), C.c_void_p(0)
    none = (None, 0, None, np.zeros(0, mm.REG_DTYPE), np.zeros((0, 2), np.uint64))
    if len(a) == 0:
        return none
    buf = ac._libc.malloc(a.nbytes)
    C.memmove(buf, a.ctypes.data, a.nbytes)
    pen_gap, pen_skip = np.float32(mo.chain_gap_scale * 0.01 * ri.io.k), np.float32(mo.chain_skip_scale * 0.01 * ri.io.k)
    out = L.mg_lchain_dp(mo.max_gap_ref, mo.max_gap, mo.bw, mo.max_chain_skip, mo.max_chain_iter, mo.min_cnt, mo.min_chain_score, pen_gap, pen_skip, 1, 1, len(a), buf,
                         C.byref(n_u), C.byref(u_ptr), None)
    if n_u.value == 0:
        return none
    regs = L.mm_gen_regs(None, ac.read_hash(r_id), len(read), n_u.value, u_ptr, out, 0)
    n_out = int((np.ctypeslib.as_array(C.cast(u_ptr, C.POINTER(C.c_uint64)), shape=(n_u.value,)) & 0xffffffff).sum())
    ac._libc.free(u_ptr)
    n = C.c_int(n_u.value)
    L.mm_set_parent(None, mo.mask_level, mo.mask_len, n.value, regs, mo.a * 2 + mo.b, int(bool(mo.flag & 0x20000000)), mo.alt_drop)
    L.mm_select_sub(None, mo.pri_ratio, ri.io.k * 2, mo.best_n, 1, int(mo.max_gap * 0.8), C.byref(n), regs)
    return regs, n.value, out, ac._snap_regs(regs, n.value)[0], np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint64)), shape=(n_out, 2)).copy()


def own_anchors(refs, reads, threads=4):
    with mm.SeedIndex(refs, k=K, w=W, hpc=False, threads=threads) as ix:
        mid_occ = ix.mid_occ()
        recs = [ix.matches(s, mid_occ) for s in reads]
    return mm.collect_seeds_host(0, recs, threads=threads) if recs else []


def ref_batch(refs, reads, preset="splice", anchors=None, **opt_kw):
    """A batch through the harness: dict(opt, k, hpc, refs, reads, regs, anchors) -- the call's input -- `want`: per read (regs, aln, words), and
    the values mm_set_opt(preset) left (before the departure and the overrides)."""
    ri = RefIndex(refs, preset, **opt_kw)
    try:
        anchors = own_anchors(refs, reads) if anchors is None else anchors
        regs_in, a_in, want = [], [], []
        for r, (s, a) in enumerate(zip(reads, anchors)):
            regs, n, a_ptr, snap_r, snap_a = ref_prepare(ri, s, a, r)
            regs_in.append(snap_r); a_in.append(snap_a)
            want.append(ac.ref_align(ri, s, regs, n, a_ptr))
        b = dict(opt=opt_from_ref(ri.mo), k=K, hpc=False, refs=[bytes(s) for s in refs], reads=[bytes(s) for s in reads], regs=regs_in, anchors=a_in)
        return b, want, ri.preset_values
    finally:
        ri.close()


def run_host(b, threads=4):
    return mm.align_regs_splice_host(b["opt"], b["k"], b["hpc"], b["refs"], b["reads"], b["regs"], b["anchors"], threads=threads)


def run_gpu(eng, b):
    return eng.align_regs_splice(b["opt"], b["k"], b["hpc"], b["refs"], b["reads"], b["regs"], b["anchors"])


def sub_batch(b, want, idx):
    """The reads idx of a batch, in that order."""
    c = dict(b)
    for k in ("reads", "regs", "anchors"):
        c[k] = [b[k][i] for i in idx]
    return c, [want[i] for i in idx]


def concat(batches):
    """Batches over the same references and options as one."""
    c = dict(batches[0][0])
    for k in ("reads", "regs", "anchors"):
        c[k] = [x for b, _ in batches for x in b[k]]
    return c, [w for _, want in batches for w in want]


# ---------------------------------------------------------------- the committed fixtures
def _opt_dict(o):
    d = {k: getattr(o.base, k) for k, _ in mm.AlignOpt._fields_}
    d.update({k: getattr(o, k) for k, _ in mm.AlignSpliceOpt._fields_[1:]})
    return d


def save_genome(refs):
    ends = np.cumsum([0] + [len(s) for s in refs]).astype(np.int64)
    np.savez_compressed(os.path.join(GOLD, "genome.npz"), refs=np.frombuffer(b"".join(refs), np.uint8), ref_end=ends)


def load_genome():
    z = np.load(os.path.join(GOLD, "genome.npz"))
    return [z["refs"][int(z["ref_end"][i]):int(z["ref_end"][i + 1])].tobytes() for i in range(len(z["ref_end"]) - 1)]


def save_batch(name, b, want, preset_values):
    cat = lambda xs, dt: np.concatenate(xs) if len(xs) else np.zeros(0, dt)
    ends = lambda xs: np.cumsum([0] + [len(x) for x in xs]).astype(np.int64)
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), opt=json.dumps(_opt_dict(b["opt"])), preset_values=json.dumps(preset_values), k=b["k"],
                        reads=np.frombuffer(b"".join(b["reads"]), np.uint8), read_end=ends(b["reads"]),
                        regs=cat(b["regs"], mm.REG_DTYPE), reg_end=ends(b["regs"]), anchors=cat(b["anchors"], np.uint64).reshape(-1, 2), a_end=ends(b["anchors"]),
                        w_regs=cat([w[0] for w in want], mm.REG_DTYPE), w_aln=cat([w[1] for w in want], mm.ALN_DTYPE), w_end=ends([w[0] for w in want]),
                        w_words=cat([w[2] for w in want], np.uint32), w_word_end=ends([w[2] for w in want]))


_genome = None


def load_batch(name):
    """(batch, want, the values mm_set_opt(preset) left in the reference's mm_mapopt_t)"""
    global _genome
    if _genome is None:
        _genome = load_genome()
    z = np.load(os.path.join(GOLD, name + ".npz"))
    cut = lambda arr, end: [z[arr][int(z[end][i]):int(z[end][i + 1])] for i in range(len(z[end]) - 1)]
    d = json.loads(str(z["opt"]))
    own = {k for k, _ in mm.AlignSpliceOpt._fields_[1:]}
    o = mm.align_splice_opt("splice", **d)
    assert _opt_dict(o) == d and own <= set(d)
    b = dict(opt=o, k=int(z["k"]), hpc=False, refs=_genome, reads=[x.tobytes() for x in cut("reads", "read_end")], regs=cut("regs", "reg_end"), anchors=cut("anchors", "a_end"))
    want = list(zip(cut("w_regs", "w_end"), cut("w_aln", "w_end"), cut("w_words", "w_word_end")))
    return b, want, json.loads(str(z["preset_values"]))


def dump_batch(path, b, want):
    """A batch as the flat file tests/tools/splice_replay.cpp reads, with a digest (FNV-1a) of the expected record offsets, records, trans_strand
    values and words, and one of the text (cg + cs, then MD; offsets and bytes) this project's host form gives for those records."""
    ends = lambda xs: np.cumsum([0] + [len(x) for x in xs]).astype(np.int64)
    regs = np.concatenate(b["regs"]) if b["regs"] else np.zeros(0, mm.REG_DTYPE)
    anchors = np.concatenate([np.asarray(a, np.uint64).reshape(-1, 2) for a in b["anchors"]]) if b["anchors"] else np.zeros((0, 2), np.uint64)
    h = 1469598103934665603
    for blob in (ends([w[0] for w in want]).tobytes(), b"".join(w[0].tobytes() for w in want), b"".join(w[1]["trans_strand"].astype("<i4").tobytes() for w in want),
                 b"".join(w[2].tobytes() for w in want)):
        for byte in blob:
            h = ((h ^ byte) * 1099511628211) & (2**64 - 1)
    ht = 1469598103934665603
    flat = mm.flatten_aligned(want)
    for what in (mm.TEXT_CG | mm.TEXT_CS, mm.TEXT_MD):
        off, text = mm.aln_text_splice_host(what, b["refs"], b["reads"], *flat)
        for byte in off.tobytes() + text:
            ht = ((ht ^ byte) * 1099511628211) & (2**64 - 1)
    with open(path, "wb") as f:
        f.write(np.array([b["k"], 0, len(b["refs"]), len(b["reads"]), len(regs), len(anchors)], np.int64).tobytes())
        f.write(np.array([h], np.uint64).tobytes() + np.array([C.sizeof(mm.AlignSpliceOpt)], np.int64).tobytes())
        f.write(bytes(b["opt"]))
        f.write(np.array([ht], np.uint64).tobytes())
        f.write(np.array([len(s) for s in b["refs"]], np.int32).tobytes() + np.array([len(s) for s in b["reads"]], np.int32).tobytes())
        f.write(ends(b["regs"]).tobytes() + ends(b["anchors"]).tobytes() + regs.tobytes() + anchors.tobytes() + b"".join(b["refs"]) + b"".join(b["reads"]))


# ---------------------------------------------------------------- the tag text of spliced records
def build_text(segs, seed=0, rev=False, lead=(0, 0), tail=(0, 0)):
    """aln_text_cases.build with a further segment kind: ("N", n), an intron of n target bases (format.c:179-184, 212-213) -- in cs "~", its
    first two bases, n, its last two; in MD nothing, and the run of matches stays open across it.  Returns the same dict."""
    rng = np.random.default_rng(seed)
    L = np.frombuffer(b"ACGT", np.uint8)
    t, q, words, cs, csl, md = [], [], [], [], [], []
    run, brk = 0, True

    def word(op, n):
        nonlocal brk
        if words and not brk and words[-1][0] == op == 0:
            words[-1][1] += n
        else:
            words.append([op, n])
        brk = False
    for kind, n in segs:
        if kind == "W":
            brk = True
        elif kind == "=":
            b = L[rng.integers(0, 4, n)].tobytes()
            t.append(b); q.append(b); cs.append(b":%d" % n); csl.append(b"=" + b); run += n
            word(0, n)
        elif kind == "X":
            for _ in range(n):
                x = int(rng.integers(0, 4)); y = (x + int(rng.integers(1, 4))) % 4
                t.append(b"ACGT"[x:x + 1]); q.append(b"ACGT"[y:y + 1])
                e = b"*" + b"acgt"[x:x + 1] + b"acgt"[y:y + 1]
                cs.append(e); csl.append(e); md.append(b"%d" % run + b"ACGT"[x:x + 1]); run = 0
            word(0, n)
        elif kind == "I":
            b = L[rng.integers(0, 4, n)].tobytes()
            q.append(b); cs.append(b"+" + b.lower()); csl.append(b"+" + b.lower())
            word(1, n); brk = True
        elif kind == "D":
            b = L[rng.integers(0, 4, n)].tobytes()
            t.append(b); cs.append(b"-" + b.lower()); csl.append(b"-" + b.lower()); md.append(b"%d^" % run + b); run = 0
            word(2, n); brk = True
        elif kind == "N":
            b = L[rng.integers(0, 4, n)].tobytes()
            t.append(b)
            e = b"~" + b[:2].lower() + b"%d" % n + b[-2:].lower()
            cs.append(e); csl.append(e)
            word(3, n); brk = True
        else:
            raise ValueError(kind)
    if run:
        md.append(b"%d" % run)
    t, q = b"".join(t), b"".join(q)
    pad = lambda n: L[rng.integers(0, 4, n)].tobytes()
    ref = pad(lead[0]) + t + pad(tail[0])
    read = pad(lead[1]) + q + pad(tail[1])
    reg = np.zeros(1, mm.REG_DTYPE)
    reg["rs"], reg["re"], reg["qs"], reg["qe"] = lead[0], lead[0] + len(t), lead[1], lead[1] + len(q)
    if rev:
        read = bytes(read).translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]
        reg["qs"], reg["qe"], reg["flags"] = tail[1], tail[1] + len(q), 1 << 10
    w = np.array([n << 4 | op for op, n in words], np.uint32)
    return dict(ref=ref, read=read, reg=reg, words=w, cg=mm.cigar_string(w).encode(), cs=b"".join(cs), cs_long=b"".join(csl), md=b"".join(md))


# records built by hand: N first after a run of matches, before a mismatch, two introns one base apart, beside I and D, the shortest and a long one
TEXT_CASES = {
    "n_first_after_a_run": [("=", 30), ("N", 500), ("=", 20)],
    "n_then_mismatch": [("=", 12), ("N", 90), ("X", 2), ("=", 9)],
    "two_introns_one_base_apart": [("=", 25), ("N", 300), ("=", 1), ("N", 400), ("=", 25)],
    "n_next_to_i_and_d": [("=", 10), ("I", 3), ("N", 120), ("D", 2), ("=", 10), ("D", 4), ("N", 80), ("I", 2), ("=", 7)],
    "n_of_length_2": [("=", 8), ("N", 2), ("=", 8)],
    "n_of_length_3": [("=", 8), ("N", 3), ("X", 1), ("=", 8)],
    "n_of_length_100000": [("=", 40), ("X", 1), ("=", 5), ("N", 100_000), ("=", 33)],
    "n_between_two_words_of_matches": [("=", 6), ("W", 0), ("=", 5), ("N", 64), ("=", 4), ("W", 0), ("=", 3)],
    "no_intron": [("=", 20), ("X", 1), ("I", 2), ("=", 20), ("D", 3), ("=", 5)],
}


def text_recs():
    out = []
    for k, (name, segs) in enumerate(TEXT_CASES.items()):
        for rev in (False, True):
            out.append(build_text(segs, seed=k, rev=rev, lead=(3, 5), tail=(4, 2)))
    return out


TEXT_BATCHES = ("default", "hq")          # the fixture batches whose records' cs / MD strings the reference's mm_gen_cs_or_MD gave are recorded


def golden_text_args(name):
    """The records and words the reference left for a fixture batch, as aln_text_splice_* takes them."""
    b, want, _ = load_batch(name)
    return (b["refs"], b["reads"]) + mm.flatten_aligned(want)


def save_texts(name, texts):
    arrs = {}
    for m, xs in texts.items():
        arrs[m] = np.frombuffer(b"".join(xs), np.uint8); arrs[m + "_off"] = np.cumsum([0] + [len(x) for x in xs]).astype(np.int64)
    np.savez_compressed(os.path.join(GOLD, f"text_{name}.npz"), **arrs)


def load_texts(name):
    """mode (cs, cs_long, md) -> list of bytes, one per record, without the tag's name."""
    z = np.load(os.path.join(GOLD, f"text_{name}.npz"))
    return {m: [z[m].tobytes()[int(z[m + "_off"][i]):int(z[m + "_off"][i + 1])] for i in range(len(z[m + "_off"]) - 1)] for m in ("cs", "cs_long", "md")}


# ---------------------------------------------------------------- the mapper: the reference program's PAF for one set of reads
PAF_VARIANTS = {"c": ["-c"], "cs": ["-c", "--cs"], "cs_long": ["-c", "--cs=long"], "md": ["-c", "--MD"]}          # name -> minimap2's flags
PAF_KW = {"c": dict(), "cs": dict(cs="short"), "cs_long": dict(cs="long"), "md": dict(md=True)}                      # ... and map_splice's keywords
PAF_OPTIONS = ["-t", "1", "--max-chain-skip=2147483647", "-x", "splice", "--cap-sw-mem=100000000"]


def paf_reads():
    """[(name, sequence)]: the `default` batch's reads and twenty more random ones, about 120."""
    refs, batches = fixture_batches()
    rng = np.random.default_rng(78)
    gs = genes()[1]
    reads = list(batches["default"][0]) + [_b(random_read(rng, refs, gs)) for _ in range(20)]
    return [(f"read{i:03d}", s) for i, s in enumerate(reads)]


def save_pafs(reads, pafs):
    np.savez_compressed(os.path.join(GOLD, "pafs.npz"), reads=np.frombuffer(b"".join(s for _, s in reads), np.uint8),
                        read_end=np.cumsum([0] + [len(s) for _, s in reads]).astype(np.int64), **{v: np.frombuffer(t.encode(), np.uint8) for v, t in pafs.items()})


def load_pafs():
    """(reference names and sequences, reads as (name, sequence), variant -> PAF text)"""
    z = np.load(os.path.join(GOLD, "pafs.npz"))
    reads = [(f"read{i:03d}", z["reads"][int(z["read_end"][i]):int(z["read_end"][i + 1])].tobytes()) for i in range(len(z["read_end"]) - 1)]
    return [(f"ref{i}", s) for i, s in enumerate(load_genome())], reads, {v: z[v].tobytes().decode() for v in PAF_VARIANTS}


def golden_meta():
    return json.load(open(os.path.join(GOLD, "meta.json")))


def default_names():
    """What every read of the `default` batch was built for (planted_reads' names, then "random"), as recorded with the fixtures."""
    return golden_meta()["default_names"]


def golden_names():
    return sorted(golden_meta()["batches"])
