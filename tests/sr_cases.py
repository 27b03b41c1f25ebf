"""Cases for short single-end reads (minimap2 -x sr): its options, the heap order of seed collection (map.c:229-293), the alignment of hits under MM_F_SR and the mapper's PAF: the
simulated read set, what the reference program printed for it and what its mm_align_skeleton returned (tests/golden/sr, made by tests/tools/gen_golden_sr.py), how this project's calls
are made on it, crafted matches and crafted single-chain batches for the ungapped first pass.
Test infrastructure only: imported by tests/test_sr_cpu.py, tests/test_gpu_sr.py and tests/tools/gen_golden_sr.py."""
import json
import os
import subprocess
import tempfile

import numpy as np

import golden_io
import orc
import mm2gb_amd as mm
import sim_reads

GOLD = os.path.join(golden_io.GOLD, "sr")
SIM_SEED = 3
LENGTHS = (80, 100, 150, 250, 750)
TANDEM = (10_000, 25, 60)            # start, copies, unit: reads inside it carry one minimizer value at several places -- seeds that share a cr list
FAMILY = (12, 400)                   # copies, length of the interspersed repeat family
WAVE_HITS = 1024                     # seed_heap.h HEAP_WAVE_HITS: one wave sorts a read of at most this many hits
# the fields of mm_mapopt_t that mm2gb_map_opt_t has a field for, and those of -x sr it has none for (recorded so that the calls to come can be held to them)
OPT_FIELDS = ("flag", "min_chain_score", "pri_ratio", "occ_dist", "bw", "bw_long", "max_gap", "max_gap_ref", "min_cnt", "best_n", "mask_level", "min_mid_occ", "max_mid_occ", "mid_occ",
              "mid_occ_frac", "q_occ_frac", "max_max_occ", "max_chain_iter", "rmq_inner_dist", "rmq_size_cap", "rmq_rescue_size", "rmq_rescue_ratio", "chain_gap_scale",
              "chain_skip_scale", "seed")
REF_ONLY_FIELDS = ("max_occ", "max_frag_len", "a", "b", "q", "e", "q2", "e2", "zdrop", "zdrop_inv", "end_bonus", "min_dp_max")
DROPS = (2_000, 40_000, 47_500)     # where the reads with a substituted middle come from (unique sequence)
INVERTED = (5_000, 56_000, 300)      # a stretch and where its reverse complement lies: reads from either have anchors of both strands
REF_EXE = os.path.join(orc.REF_DIR, "minimap2_cpu")
F_2_IO_THREADS = 0x8000              # MM_F_2_IO_THREADS: the reference program's file reading, nothing a library call looks at


def genome(rng):
    """60 kb with a 25 x 60-base tandem array, a 12-copy 400-base family (copies about 1 % diverged) and a 300-base inverted repeat."""
    g = sim_reads.BASES[rng.integers(0, 4, 60_000)].copy()
    st, copies, unit = TANDEM
    g[st:st + copies * unit] = np.tile(sim_reads.BASES[rng.integers(0, 4, unit)], copies)
    fam = sim_reads.BASES[rng.integers(0, 4, FAMILY[1])]
    for c in range(FAMILY[0]):
        cp = fam.copy()
        mut = rng.random(len(cp)) < 0.01
        cp[mut] = sim_reads.BASES[rng.integers(0, 4, int(mut.sum()))]
        at = 14_000 + c * 3_500
        g[at:at + len(cp)] = cp
    g[INVERTED[1]:INVERTED[1] + INVERTED[2]] = sim_reads.revcomp(g[INVERTED[0]:INVERTED[0] + INVERTED[2]])
    return g


def sim_set(seed=SIM_SEED):
    """(genome bytes, [(name, bytes)]): about 200 reads of 80, 100, 150, 250 and 750 bases from both strands at 0.5-2 % error, eight of them from inside the tandem
    array and eight from inside the repeat family, four from the inverted repeat, a few with an N, one of 30 bases and one that is not from the genome."""
    rng = np.random.default_rng(seed)
    g = genome(rng)
    reads = []

    def add(tag, st, n):
        s = sim_reads.mutate(rng, g[st:st + n], float(rng.uniform(0.005, 0.02)))
        if rng.random() < 0.5:
            s = sim_reads.revcomp(s)
        if rng.random() < 0.04:
            s = s.copy()
            s[int(rng.integers(0, len(s)))] = ord("N")
        reads.append((f"{tag}{len(reads)}_{st}_{n}", s.tobytes()))
    for r in range(184):
        n = LENGTHS[r % len(LENGTHS)]
        add("read", int(rng.integers(0, len(g) - n)), n)
    t0, copies, unit = TANDEM
    for r in range(8):
        n = (100, 150, 250, 750)[r % 4]
        add("tandem", t0 + int(rng.integers(0, copies * unit - min(n, 600))), n)
    for r in range(8):
        add("family", 14_000 + int(rng.integers(0, FAMILY[0])) * 3_500 + int(rng.integers(0, 150)), (150, 250)[r % 2])
    for r in range(4):
        add("inverted", INVERTED[r % 2] + 20 * r, (150, 250)[r // 2])
    add("tiny", 30_000, 30)
    reads.append(("stray", sim_reads.BASES[rng.integers(0, 4, 150)].tobytes()))
    for r, st in enumerate(DROPS):       # 250 bases as the genome has them but for the middle 40, every one substituted (no indel): one diagonal, and the fill over it z-drops
        s = g[st:st + 250].copy()
        s[105:145] = sim_reads.BASES[(np.searchsorted(sim_reads.BASES, s[105:145]) + 1 + r % 3) % 4]
        reads.append((f"drop{len(reads)}_{st}_250", (sim_reads.revcomp(s) if r == 1 else s).tobytes()))
    return g.tobytes(), reads


_gold = None


def gold():
    """The committed fixture (seeds.npz: one JSON document, compressed): {"genome": sequence, "reads": [[name, sequence]], "options": {"map": ..., "ref_only": ..., "index": ...},
    "seeds": {read name: {"rep_len": n, "sd": [[strand, reference position, query position, span]]}}} -- the SD lines of minimap2 -x sr --print-seeds in their order."""
    global _gold
    if _gold is None:
        _gold = json.loads(np.load(os.path.join(GOLD, "seeds.npz"))["doc"].tobytes().decode("utf-8"))
    return _gold


def reads():
    return [(n, s.encode()) for n, s in gold()["reads"]]


_index = None


def index():
    """The genome's SeedIndex at the preset's k and w, kept for the process (host-built)."""
    global _index
    if _index is None:
        _index = mm.SeedIndex([gold()["genome"].encode()], threads=4, **mm.preset_sr())
    return _index


def matches(seqs, mid_occ=None):
    """Every read's matches from this project's host seeding at the preset's thresholds: the records the seed collection calls take."""
    o = mm.map_opt_sr()
    return [index().matches(s, o.mid_occ if mid_occ is None else mid_occ, o.max_max_occ, o.occ_dist, o.q_occ_frac) for s in seqs]


def sd_rows(anchors):
    """An (m,2) uint64 anchor array as the SD lines' fields: [strand, reference position, query position, span] (one reference sequence: no name)."""
    a = np.asarray(anchors, dtype=np.uint64).reshape(-1, 2)
    return [[int(x >> 63), int(x & 0xffffffff), int(y & 0xffffffff), int(y >> 32 & 0xff)] for x, y in ((int(x), int(y)) for x, y in a)]


def has_equal_cr(m):
    """Two of a read's hits carry the same index entry (among one seed's they are distinct)."""
    h = np.asarray(m["hits"], dtype=np.uint64)
    return len(np.unique(h)) < len(h)


def own_options():
    o = mm.map_opt_sr()
    return json.loads(json.dumps(dict(map={k: getattr(o, k) for k in OPT_FIELDS}, index=mm.preset_sr())))


def ref_options():
    """mm_set_opt(NULL) + mm_set_opt("sr") of the built reference (oracle/_ref).  MM_F_2_IO_THREADS is left out of the flag; max_chain_skip is what main.c:316-318 forces."""
    import ctypes as C
    import align_cases as ac
    L = ac.ref_lib()
    io, mo = ac._IdxOpt(), ac.MapOpt()
    assert L.mm_set_opt(None, C.byref(io), C.byref(mo)) == 0 and L.mm_set_opt(b"sr", C.byref(io), C.byref(mo)) == 0
    m = {k: getattr(mo, k) for k in OPT_FIELDS}
    m["flag"] &= ~F_2_IO_THREADS
    return json.loads(json.dumps(dict(map=m, ref_only={k: getattr(mo, k) for k in REF_ONLY_FIELDS}, index=dict(k=io.k, w=io.w, hpc=bool(io.flag & 1)))))


def record_seeds(genome, reads):
    """{read name: {"rep_len": n, "sd": [[strand, rpos, qpos, span]]}} from the program's stderr: QR opens a read, RS its anchors (the first RS block of a read is
    the round at mid_occ; the rescue round prints none)."""
    exe = REF_EXE
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "ref.fa"), "wb") as fh:
            fh.write(b">ref\n" + genome + b"\n")
        with open(os.path.join(d, "reads.fa"), "wb") as fh:
            for name, s in reads:
                fh.write(b">" + name.encode() + b"\n" + s + b"\n")
        err = subprocess.run([exe, "-t", "1", "-x", "sr", "--print-seeds", os.path.join(d, "ref.fa"), os.path.join(d, "reads.fa")], check=True, capture_output=True).stderr.decode()
    out, cur = {}, None
    for ln in err.splitlines():
        f = ln.split("\t")
        if f[0] == "QR":
            cur = out.setdefault(f[1], dict(rep_len=None, sd=[], blocks=0))
        elif f[0] == "RS":
            cur["blocks"] += 1
            if cur["blocks"] == 1:
                cur["rep_len"] = int(f[1])
        elif f[0] == "SD" and cur["blocks"] == 1:
            assert f[1] == "ref"
            cur["sd"].append([int(f[3] == "-"), int(f[2]), int(f[4]), int(f[5])])
    assert all(v["blocks"] == 1 for v in out.values())
    return {k: dict(rep_len=v["rep_len"], sd=v["sd"]) for k, v in out.items()}


# ---------------------------------------------------------------- the mapper's runs
# run: (the reference program's arguments, this project's option overrides, map_sr's overrides); ALIGNED: the runs with base-level alignment (map_sr gets the genome too)
ALIGNED = ("sr.c", "sr.cs", "sr.csmd")
RUNS = {
    "sr": (["-x", "sr"], {}, {}),
    "sr.c": (["-x", "sr", "-c"], {}, dict(align=True)),
    "sr.cs": (["-x", "sr", "-c", "--cs"], {}, dict(align=True, cs="short")),
    "sr.csmd": (["-x", "sr", "--cs=long", "--MD", "-c"], {}, dict(align=True, cs="long", md=True)),
    "sr.f4_50": (["-x", "sr", "-f", "4,50"], dict(mid_occ=4), dict(max_occ=50)),        # mid_occ 4, max_occ 50: the repeat family's reads go through the rescue
    "sr.f4_4": (["-x", "sr", "-f", "4,4"], dict(mid_occ=4), dict(max_occ=4)),             # max_occ = mid_occ: no rescue -- what the rescue is worth shows against it
    "sr.2nd": (["-x", "sr", "--secondary=yes"], dict(flag=0x1000 | 0x2000 | 0x400000), {}),   # MM_F_NO_PRINT_2ND cleared: for comparison with "sr"
    "sr.sorted": (["-x", "sr", "--heap-sort=no"], dict(flag=0x1000 | 0x2000 | 0x4000), {}),   # MM_F_HEAP_SORT cleared: anchors through radix_sort_128x
}


def record_paf(genome, reads, args):
    """What the reference program prints for a run."""
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "ref.fa"), "wb") as fh:
            fh.write(b">ref\n" + genome + b"\n")
        with open(os.path.join(d, "reads.fa"), "wb") as fh:
            for name, s in reads:
                fh.write(b">" + name.encode() + b"\n" + s + b"\n")
        return subprocess.run([REF_EXE, "-t", "1"] + args + [os.path.join(d, "ref.fa"), os.path.join(d, "reads.fa")], check=True, capture_output=True).stdout.decode()


_pafs = None


def golden_paf(run):
    """The committed PAFs (pafs.npz: one JSON document, compressed): {run: text}."""
    global _pafs
    if _pafs is None:
        _pafs = json.loads(np.load(os.path.join(GOLD, "pafs.npz"))["doc"].tobytes().decode("utf-8"))
    return _pafs[run]


def map_run(engine, run, stream=False, align_on_device=0, text_on_device=0, **fields):
    """A recorded run through this project's mapper: (PAF text, stats).  stream: through map_reads_stream in chunks of about 5000 bases."""
    _, opt_kw, sr_kw = RUNS[run]
    opt = mm.map_opt_sr(host_threads=4, **dict(opt_kw, **fields))
    if sr_kw.get("align"):
        sr_kw = dict(sr_kw, refs=[gold()["genome"].encode()], align_on_device=align_on_device, text_on_device=text_on_device)
    if stream:
        return mm.map_reads_stream([engine], index(), ["ref"], reads(), opt=opt, k=mm.preset_sr()["k"], chunk_bases=5_000, align=mm.map_sr(**sr_kw))
    return mm.map_reads(engine, index(), ["ref"], reads(), opt=opt, k=mm.preset_sr()["k"], align=mm.map_sr(**sr_kw))


# ---------------------------------------------------------------- alignment of hits under MM_F_SR: the reference's mm_align_skeleton through ctypes
class SrRef:
    """mm_idx_str on the genome at the preset's k and w, and mm_set_opt("sr")'s options after mm_mapopt_update, max_chain_skip as main.c:316-318 forces it."""

    def __init__(self, refs, **opt_kw):
        import ctypes as C
        import align_cases as ac
        L = ac.ref_lib()
        self.refs = [bytes(s) for s in refs]
        self._seqs = (C.c_char_p * len(self.refs))(*self.refs)
        self._names = (C.c_char_p * len(self.refs))(*[f"ref{k}".encode() for k in range(len(self.refs))])
        self.io, self.mo = ac._IdxOpt(), ac.MapOpt()
        assert L.mm_set_opt(None, C.byref(self.io), C.byref(self.mo)) == 0 and L.mm_set_opt(b"sr", C.byref(self.io), C.byref(self.mo)) == 0
        self.mi = L.mm_idx_str(self.io.w, self.io.k, self.io.flag & 1, self.io.bucket_bits, len(self.refs), self._seqs, self._names)
        L.mm_mapopt_update(C.byref(self.mo), self.mi)
        self.mo.max_chain_skip = 2**31 - 1
        for k, v in opt_kw.items():
            setattr(self.mo, k, v)

    def close(self):
        import align_cases as ac
        if self.mi:
            ac.ref_lib().mm_idx_destroy(self.mi)
            self.mi = None


def sr_ref_prepare(ri, read, anchors, r_id):
    """align_cases.ref_prepare with the gaps of map.c:678-686: mg_lchain_dp, mm_gen_regs, mm_set_parent, mm_select_sub on this project's heap-order anchors."""
    import ctypes as C
    import align_cases as ac
    L, mo = ac.ref_lib(), ri.mo
    a = np.ascontiguousarray(anchors, dtype=np.uint64).reshape(-1, 2)
    none = (None, 0, None, np.zeros(0, mm.REG_DTYPE), np.zeros((0, 2), np.uint64))
    if len(a) == 0:
        return none
    n_u, u_ptr = C.c_int(0), C.c_void_p(0)
    buf = ac._libc.malloc(a.nbytes)
    C.memmove(buf, a.ctypes.data, a.nbytes)
    pen_gap, pen_skip = np.float32(mo.chain_gap_scale * 0.01 * ri.io.k), np.float32(mo.chain_skip_scale * 0.01 * ri.io.k)
    qlen = len(read)
    max_x = mo.max_gap_ref if mo.max_gap_ref > 0 else max(mo.max_frag_len - qlen if mo.max_frag_len > 0 else mo.max_gap, mo.max_gap)
    out = L.mg_lchain_dp(max_x, max(qlen, mo.max_gap), mo.bw, mo.max_chain_skip, mo.max_chain_iter, mo.min_cnt, mo.min_chain_score, pen_gap, pen_skip, 0, 1, len(a), buf,
                         C.byref(n_u), C.byref(u_ptr), None)
    if n_u.value == 0:
        return none
    regs = L.mm_gen_regs(None, ac.read_hash(r_id), qlen, n_u.value, u_ptr, out, 0)
    n_out = int((np.ctypeslib.as_array(C.cast(u_ptr, C.POINTER(C.c_uint64)), shape=(n_u.value,)) & 0xffffffff).sum())
    ac._libc.free(u_ptr)
    n = C.c_int(n_u.value)
    L.mm_set_parent(None, mo.mask_level, mo.mask_len, n.value, regs, mo.a * 2 + mo.b, int(bool(mo.flag & 0x20000000)), mo.alt_drop)
    L.mm_select_sub(None, mo.pri_ratio, ri.io.k * 2, mo.best_n, 1, int(mo.max_gap * 0.8), C.byref(n), regs)
    return regs, n.value, out, ac._snap_regs(regs, n.value)[0], np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint64)), shape=(n_out, 2)).copy()


def sr_ref_batch(genome, seqs, **opt_kw):
    """Reads through the reference: (the alignment calls' input as a dict, per read (regs, aln, words) as mm_align_skeleton left them)."""
    import align_cases as ac
    ri = SrRef([genome], **opt_kw)
    try:
        o = mm.map_opt_sr()
        with mm.SeedIndex([genome], threads=4, **mm.preset_sr()) as ix:
            m = [ix.matches(s, o.mid_occ, o.max_max_occ, o.occ_dist, o.q_occ_frac) for s in seqs]
        anchors, _ = mm.collect_seeds_heap_host(o.flag, m)
        regs_in, a_in, want = [], [], []
        for r, (s, a) in enumerate(zip(seqs, anchors)):
            regs, n, a_ptr, snap_r, snap_a = sr_ref_prepare(ri, s, a, r)
            regs_in.append(snap_r); a_in.append(snap_a)
            want.append(ac.ref_align(ri, s, regs, n, a_ptr))
        return dict(opt=ac.opt_from_ref(ri.mo), k=ri.io.k, hpc=False, refs=[bytes(genome)], reads=[bytes(s) for s in seqs], regs=regs_in, anchors=a_in), want
    finally:
        ri.close()


def run_sr_host(b, threads=4):
    return mm.align_regs_sr_host(b["opt"], b["k"], b["hpc"], b["refs"], b["reads"], b["regs"], b["anchors"], threads=threads)


def run_sr_gpu(eng, b):
    return eng.align_regs_sr(b["opt"], b["k"], b["hpc"], b["refs"], b["reads"], b["regs"], b["anchors"])


def save_aligned(path, batch, want):
    """aln.npz: the alignment calls' records and anchors in, and the reference's records, alignment rows and CIGAR words out, every read's end to end with offsets."""
    cat = lambda xs, dt, shape=(0,): np.concatenate(xs) if len(xs) else np.zeros(shape, dt)
    off = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)
    np.savez_compressed(path, reg_off=off(batch["regs"]), regs=cat(batch["regs"], mm.REG_DTYPE), a_off=off(batch["anchors"]), anchors=cat(batch["anchors"], np.uint64, (0, 2)),
                        want_off=off([w[0] for w in want]), want_regs=cat([w[0] for w in want], mm.REG_DTYPE), want_aln=cat([w[1] for w in want], mm.ALN_DTYPE),
                        word_off=off([w[2] for w in want]), want_words=cat([w[2] for w in want], np.uint32))


def golden_aligned():
    """(batch, want) of the committed aln.npz for the fixture's reads and the preset's alignment options."""
    z = np.load(os.path.join(GOLD, "aln.npz"))
    cut = lambda a, off: [a[off[i]:off[i + 1]] for i in range(len(off) - 1)]
    batch = dict(opt=mm.align_sr_opt(), k=mm.preset_sr()["k"], hpc=False, refs=[gold()["genome"].encode()], reads=[s for _, s in reads()],
                 regs=cut(z["regs"], z["reg_off"]), anchors=cut(z["anchors"], z["a_off"]))
    want = list(zip(cut(z["want_regs"], z["want_off"]), cut(z["want_aln"], z["want_off"]), cut(z["want_words"], z["word_off"])))
    return batch, want


# ---------------------------------------------------------------- crafted single-chain batches for the ungapped first pass
def _bases(rng, n):
    return sim_reads.BASES[rng.integers(0, 4, n)].copy()


def _other(x, by=1):
    return sim_reads.BASES[(np.searchsorted(sim_reads.BASES, x) + by) % 4]


def chain_case(rng, length, edit=None, lead=30, tail=30):
    """One read with one chain on one diagonal whose stretch is `length` columns: the read is lead + length + tail bases of the reference (which starts 50 bases earlier),
    edit(query stretch, target stretch) changes either in place.  Anchors are caller-made: one of span `length` up to 255 columns, two colinear ones beyond (the second
    ends the stretch; spans 200 and min(length - 200, 255)).  Returns (reference, read, record, anchors)."""
    t = _bases(rng, 50 + lead + length + tail + 50)
    q = t[50:50 + lead + length + tail].copy()
    if edit:
        edit(q[lead:lead + length], t[50 + lead:50 + lead + length])
    qe, te = lead + length - 1, 50 + lead + length - 1           # the stretch's last column
    if length <= 255:
        a = [[te, length << 32 | qe]]
    else:
        a = [[te - (length - 200), 200 << 32 | (qe - (length - 200))], [te, min(length - 200, 255) << 32 | qe]]
    a = np.asarray(a, np.uint64)
    reg = np.zeros(1, mm.REG_DTYPE)
    reg["id"], reg["cnt"], reg["rid"], reg["score"], reg["score0"], reg["as_"] = 0, len(a), 0, min(length, 255), min(length, 255), 0
    reg["qs"], reg["qe"], reg["rs"], reg["re"], reg["parent"], reg["subsc"] = lead, lead + length, 50 + lead, 50 + lead + length, 0, 0
    reg["mlen"], reg["blen"], reg["div"], reg["hash"] = length, length, -1.0, 7
    return t.tobytes(), q.tobytes(), reg, a


def ungapped_cases(rng):
    """name -> chain_case: the stretch lengths at which k_al_ungapped's 64-column steps begin and end, a drop across a step's boundary, the walk's tie at the maximum,
    every column a mismatch, N in the query, the target and both, and drops of exactly zdrop and zdrop + 1 (a 2, b 8, zdrop 100: see the comments)."""
    out = {}
    for n in (1, 63, 64, 65, 128, 129, 255, 300, 1000):
        out[f"len{n}"] = chain_case(rng, n)
    # columns 56..71 mismatch: 16 x 8 = 128 below the maximum, across the first step's boundary; the score then climbs past the old maximum
    out["drop_across_64"] = chain_case(rng, 200, lambda q, t: q.__setitem__(slice(56, 72), _other(q[56:72])))

    def tie(q, t):                       # one mismatch (-8), four matches (+8): at column 14 the score equals the maximum held at column 9 -- the maximum moves forward (align.c:44) --,
        q[10] = _other(q[10]); q[15:35] = _other(q[15:35])          # and the deep drop that follows at once is measured from column 14, not 9
    out["tie_at_max"] = chain_case(rng, 120, tie)
    out["all_mismatch"] = chain_case(rng, 70, lambda q, t: q.__setitem__(slice(None), _other(q)))
    out["n_query"] = chain_case(rng, 100, lambda q, t: q.__setitem__(slice(30, 33), ord("N")))
    out["n_target"] = chain_case(rng, 100, lambda q, t: t.__setitem__(slice(60, 66), ord("N")))

    def n_both(q, t):
        q[40:44] = ord("N"); t[42:50] = ord("N"); q[70] = ord("N"); t[70] = ord("N")
    out["n_both"] = chain_case(rng, 130, n_both)
    # twelve mismatches and four N-columns (-1 each under the real matrix): 12 x 8 + 4 = 100 below the maximum: not a drop (strict >); one more N-column: 101, a drop
    def drop100(q, t):
        q[50:62] = _other(q[50:62]); q[62:66] = ord("N")
    def drop101(q, t):
        q[50:62] = _other(q[50:62]); q[62:67] = ord("N")
    out["drop_100"] = chain_case(rng, 150, drop100)
    out["drop_101"] = chain_case(rng, 150, drop101)
    return out


def ungapped_batch(cases):
    """The cases as one batch of the alignment calls: one reference sequence and one read per case."""
    names = list(cases)
    regs = []
    for i, n in enumerate(names):
        g = cases[n][2].copy()
        g["rid"] = i
        regs.append(g)
    anchors = [cases[n][3] + np.asarray([[i << 32, 0]], np.uint64) for i, n in enumerate(names)]
    return dict(opt=mm.align_sr_opt(min_cnt=1), k=21, hpc=False, refs=[cases[n][0] for n in names], reads=[cases[n][1] for n in names], regs=regs, anchors=anchors)


# ---------------------------------------------------------------- crafted matches
def seed(n, q_pos, strand=0, span=21, tandem=False):
    """One mm2gb_seed_t row: n hits, the minimizer's last base at q_pos on `strand`."""
    return [n, q_pos << 1 | strand, span, (1 << 31) if tandem else 0]


def hit(pos, strand=0, rid=0):
    return rid << 32 | pos << 1 | strand


def read_of(seeds, lists, qlen):
    return dict(seeds=np.asarray(seeds, np.uint32).reshape(-1, 4), hits=np.asarray([h for l in lists for h in l], np.uint64), qlen=qlen)


def crafted_reads(rng):
    """name -> read: what the device form can get wrong, at the smallest sizes -- no seed, one hit, three seeds on one five-hit list (the heap's own tie order), a
    tie between a forward and a reverse seed, a read just under, at and just over the one-wave bound (distinct cr), one over it with a tie, seeds without hits."""
    out = {}
    out["no_seed"] = read_of([], [], 100)
    out["one_hit"] = read_of([seed(1, 40)], [[hit(5_000)]], 100)
    five = [hit(p) for p in (900, 2_000, 2_060, 7_000, 7_500)]
    out["three_on_one_list"] = read_of([seed(5, 30), seed(5, 90), seed(5, 150), seed(2, 170, 1)], [five, five, five, [hit(1_000), hit(6_000)]], 250)
    out["tie_across_strands"] = read_of([seed(3, 30), seed(3, 90, 1), seed(0, 95), seed(1, 120)], [five[:3], five[:3], [], [hit(2_030)]], 150)

    def many(n, n_seeds, tie=False):
        pos = np.sort(rng.choice(np.arange(100, 2_000_000), n, replace=False))
        owner = rng.integers(0, n_seeds, n)
        lists = [[hit(int(p), int(p) & 1) for p in pos[owner == s]] for s in range(n_seeds)]
        if tie:
            lists[1] = sorted(set(lists[1]) | set(lists[0][-3:]))          # three cr that two seeds share
        seeds = [seed(len(l), 25 + 7 * s, s & 1) for s, l in enumerate(lists)]
        return read_of(seeds, lists, 25 + 7 * n_seeds + 10)
    out["wave_minus_1"] = many(WAVE_HITS - 1, 40)
    out["wave_exact"] = many(WAVE_HITS, 40)
    out["wave_plus_1"] = many(WAVE_HITS + 1, 40)
    out["long_tied"] = many(WAVE_HITS + 300, 9, tie=True)
    out["odd_65"] = many(65, 5)
    return out


def heap_literal(rd, flag=0, ref_len=None, ref_rank=None):
    """map.c:229-293 with ksort.h:43-59 in plain Python on one read of the seed collection calls' input: the anchors as an (m,2) uint64 array."""
    seeds = np.asarray(rd["seeds"], np.uint32).reshape(-1, 4)
    hits = [int(h) for h in rd["hits"]]
    off = np.concatenate([[0], np.cumsum(seeds[:, 0])]).astype(int)
    qlen, names = rd["qlen"], "q_rank" in rd and flag & (mm.F_NO_DIAG | mm.F_NO_DUAL)
    heap = [[hits[off[i]], i, 0] for i in range(len(seeds)) if seeds[i][0] > 0]

    def down(i, n):
        tmp = heap[i]
        k = 2 * i + 1
        while k < n:
            if k != n - 1 and heap[k][0] > heap[k + 1][0]:
                k += 1
            if heap[k][0] > tmp[0]:
                break
            heap[i] = heap[k]
            i, k = k, 2 * k + 1
        heap[i] = tmp
    for i in range(len(heap) // 2 - 1, -1, -1):
        down(i, len(heap))
    fwd, rev, n = [], [], len(heap)
    while n > 0:
        r, i, k = heap[0]
        cnt, q_pos, span, seg_tandem = (int(v) for v in seeds[i])
        span &= 0x7fffffff
        same = (r & 1) == (q_pos & 1)
        skip = is_self = False
        if names:
            rid = r >> 32
            if flag & mm.F_NO_DIAG and rd["q_rank"] == ref_rank[rid] and ref_len[rid] == qlen:
                if (r & 0xffffffff) >> 1 == q_pos >> 1:
                    skip = True
                elif same:
                    is_self = True
            if flag & mm.F_NO_DUAL and rd["q_rank"] > ref_rank[rid]:
                skip = True
        if not skip and flag & (0x100000 | 0x200000):              # MM_F_FOR_ONLY | MM_F_REV_ONLY
            skip = bool(flag & 0x200000) if same else bool(flag & 0x100000)
        if not skip:
            x = (r & 0xffffffff00000000) | (r & 0xffffffff) >> 1
            y = span << 32 | (q_pos >> 1 if same else qlen - ((q_pos >> 1) + 1 - span) - 1)
            y |= (seg_tandem & 0x7fffffff) << 48 | (1 << 42 if seg_tandem >> 31 else 0) | (1 << 43 if is_self else 0)
            (fwd if same else rev).append([x if same else x | 1 << 63, y])
        if k < cnt - 1:
            heap[0] = [hits[off[i] + k + 1], i, k + 1]
        else:
            heap[0] = heap[n - 1]
            n -= 1
        if n > 0:
            down(0, n)
    return np.asarray(fwd + rev, dtype=np.uint64).reshape(-1, 2)


def dump_batch(path, flag, batch):
    """The file tests/tools/sr_replay.cpp replays: the batch's arrays as the C call takes them, then what the plain-Python restatement gives for it."""
    seeds = np.concatenate([np.asarray(r["seeds"], np.uint32).reshape(-1, 4) for r in batch])
    seed_off = np.concatenate([[0], np.cumsum([len(r["seeds"]) for r in batch])]).astype(np.int64)
    hit_off = np.concatenate([[0], np.cumsum(seeds[:, 0])]).astype(np.int64)
    hits = np.concatenate([np.asarray(r["hits"], np.uint64) for r in batch])
    want = [heap_literal(r, flag) for r in batch]
    want_off = np.concatenate([[0], np.cumsum([len(a) for a in want])]).astype(np.int64)
    head = np.asarray([len(batch), len(seeds), len(hits), int(want_off[-1]), flag, sum(has_equal_cr(r) for r in batch)], np.int64)
    with open(path, "wb") as fh:
        for a in (head, seed_off, seeds, hit_off, hits, np.asarray([r["qlen"] for r in batch], np.int32), want_off, np.concatenate(want).astype(np.uint64)):
            fh.write(np.ascontiguousarray(a).tobytes())
