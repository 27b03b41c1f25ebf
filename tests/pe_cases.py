"""Cases for paired-end short reads (minimap2 -x sr r1.fq r2.fq without -c): fragments of two mates seeded and chained as one query, the rescue when the best chain lacks a
mate, mm_select_sub_multi, mm_seg_gen and the PAF lines: the simulated pairs on two contigs, what the reference program printed for them and what its exported mm_select_sub_multi
and mm_seg_gen returned (tests/golden/pe, made by tests/tools/gen_golden_pe.py), how this project's calls are made on them, and crafted records, anchors and fragments.
Test infrastructure only: imported by tests/test_pe_cpu.py, tests/test_gpu_pe.py and tests/tools/gen_golden_pe.py."""
import ctypes as C
import json
import os
import subprocess
import tempfile

import numpy as np

import golden_io
import orc
import mm2gb_amd as mm
import sim_reads

GOLD = os.path.join(golden_io.GOLD, "pe")
SIM_SEED = 5
CONTIGS = (("ctgA", 40_000), ("ctgB", 20_000))
FAMILY_LEN = 400
FAMILY_AT = ((0, [3_000 + c * 3_000 for c in range(12)]), (1, [2_000 + c * 4_500 for c in range(4)]))     # (contig, starts of the repeat family's copies): 12 + 4
MATE_LENS = ((150, 150), (100, 100), (250, 250), (80, 80), (150, 100), (80, 250), (100, 150), (250, 80))     # both mates' lengths: six distinct sums
REF_EXE = os.path.join(orc.REF_DIR, "minimap2_cpu")
K = 21


def genome(rng):
    """Two contigs of 40 kb and 20 kb with a 400-base repeat family of 12 + 4 copies (about 1 % diverged)."""
    fam = sim_reads.BASES[rng.integers(0, 4, FAMILY_LEN)]
    ctg = [sim_reads.BASES[rng.integers(0, 4, n)].copy() for _, n in CONTIGS]
    for c, starts in FAMILY_AT:
        for at in starts:
            cp = fam.copy()
            mut = rng.random(len(cp)) < 0.01
            cp[mut] = sim_reads.BASES[rng.integers(0, 4, int(mut.sum()))]
            ctg[c][at:at + len(cp)] = cp
    return ctg


def sim_set(seed=SIM_SEED):
    """([contig bytes], [(name, bytes)]): about 110 fragments, mates interleaved.  Random pairs of 80, 100, 150 and 250 bases (eight combinations), inserts from just above the
    longer mate up to 700, either mate first on the forward strand, 1 % error; and by name: fam* (one mate inside a copy of the repeat family, the other in unique sequence
    beside it, on both contigs), overlap (insert = mate length), far (mates 29 kb apart), cross (mates on different contigs), stray (second mate random), tiny (second mate 30
    bases), withn (a mate containing N), lone (a single read between two pairs) and plain (a pair whose names carry no /1 /2)."""
    rng = np.random.default_rng(seed)
    g = genome(rng)
    reads = []

    def mate(c, st, n, rev):
        s = sim_reads.mutate(rng, g[c][st:st + n], 0.01)
        return sim_reads.revcomp(s) if rev else s

    def pair(tag, c1, st1, n1, c2, st2, n2, flip, suffix=True):
        """Mate 1 forward at (c1, st1), mate 2 reverse at (c2, st2): the layout of a fragment read from its left end; flip: read from its right end instead."""
        m1, m2 = mate(c1, st1, n1, False), mate(c2, st2, n2, True)
        if flip:
            m1, m2 = m2, m1
        name = f"{tag}{len(reads) // 2}"
        reads.append((name + ("/1" if suffix else ""), m1.tobytes()))
        reads.append((name + ("/2" if suffix else ""), m2.tobytes()))

    def insert_pair(tag, c, st, n1, n2, insert, flip, suffix=True):
        pair(tag, c, st, n1, c, st + insert - n2, n2, flip, suffix)
    for r in range(84):
        n1, n2 = MATE_LENS[r % len(MATE_LENS)]
        insert = int(rng.integers(max(n1, n2) + 1, 701))
        c = int(rng.integers(0, 2))
        insert_pair("pair", c, int(rng.integers(0, CONTIGS[c][1] - insert)), n1, n2, insert, bool(rng.integers(0, 2)))
    for c, starts in FAMILY_AT:                          # one mate inside a copy (150 bases from its 100th base), the other in the unique sequence behind or before it
        for i, at in enumerate(starts[:8] if c == 0 else starts):
            if i % 2 == 0:
                insert_pair(f"fam{c}_", c, at + 100, 150, 150, 550 + 10 * i, bool(i & 2))       # the repeat mate first
            else:
                insert_pair(f"fam{c}_", c, at + 250 - 520, 150, 150, 520, bool(i & 2))         # the unique mate first: the second ends with the copy's 250th base
    insert_pair("overlap", 0, 21_700, 150, 150, 150, False)
    pair("far", 0, 5_000, 150, 0, 34_000, 150, False)
    pair("cross", 0, 26_000, 150, 1, 12_500, 150, False)
    insert_pair("pair", 1, 7_000, 150, 150, 400, False)
    reads.append(("lone", mate(0, 13_000, 150, False).tobytes()))
    insert_pair("pair", 0, 16_500, 100, 100, 350, True)
    name = f"stray{len(reads) // 2}"
    reads.append((name + "/1", mate(1, 9_000, 150, False).tobytes()))
    reads.append((name + "/2", sim_reads.BASES[rng.integers(0, 4, 150)].tobytes()))
    insert_pair("tiny", 0, 29_000, 150, 30, 300, False)
    insert_pair("withn", 1, 15_000, 150, 150, 380, False)
    s = bytearray(reads[-1][1])
    s[70] = ord("N")
    reads[-1] = (reads[-1][0], bytes(s))
    insert_pair("plain", 0, 37_000, 100, 150, 450, False, suffix=False)
    return [x.tobytes() for x in g], reads


_gold = None


def gold():
    """The committed fixture (pe.npz, key doc: one JSON document): {"contigs": [[name, sequence]], "reads": [[name, sequence]], "options": ..., "pafs": {run: text}, "se": text,
    "seeds": [{"rep_len": n, "sd": [[contig, strand, rpos, qpos, span]]} per fragment]}."""
    global _gold
    if _gold is None:
        _gold = json.loads(np.load(os.path.join(GOLD, "pe.npz"))["doc"].tobytes().decode("utf-8"))
    return _gold


def reads():
    return [(n, s.encode()) for n, s in gold()["reads"]]


def contigs():
    return [(n, s.encode()) for n, s in gold()["contigs"]]


def fragments(rd=None):
    """The fixture's reads as fragments: [[(name, sequence)]] by this project's frag_offsets."""
    rd = reads() if rd is None else rd
    off = mm.frag_offsets([n for n, _ in rd])
    return [rd[off[f]:off[f + 1]] for f in range(len(off) - 1)]


def oriented(frag, pe_ori=1):
    """A fragment's sequences as they are mapped: mate j of a two-mate fragment reverse-complemented when pe_ori says so (map.c:1169-1171)."""
    seqs = [s for _, s in frag]
    if len(seqs) == 2:
        seqs = [revcomp(s) if (j == 0 and pe_ori >> 1 & 1) or (j == 1 and pe_ori & 1) else s for j, s in enumerate(seqs)]
    return seqs


_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def revcomp(s):
    return bytes(s).translate(_COMP)[::-1]


_index = None


def index():
    global _index
    if _index is None:
        _index = mm.SeedIndex([s for _, s in contigs()], threads=4, **mm.preset_sr())
    return _index


def matches_frag(frags, mid_occ=None, pe_ori=1, ix=None):
    o = mm.map_opt_sr()
    return [(ix or index()).matches_frag(oriented(f, pe_ori), o.mid_occ if mid_occ is None else mid_occ, o.max_max_occ, o.occ_dist, o.q_occ_frac) for f in frags]


def sd_rows(anchors):
    """An (m,2) uint64 anchor array as the SD lines' fields: [contig, strand, reference position, query position, span]."""
    a = np.asarray(anchors, dtype=np.uint64).reshape(-1, 2)
    return [[int(x >> 32 & 0x7fffffff), int(x >> 63), int(x & 0xffffffff), int(y & 0xffffffff), int(y >> 32 & 0xff)] for x, y in ((int(x), int(y)) for x, y in a)]


# ---------------------------------------------------------------- the reference program's runs
# run: (the program's arguments, this project's option overrides, map_sr's overrides)
RUNS = {
    "pe": (["-x", "sr"], {}, {}),
    "pe.f4_50": (["-x", "sr", "-f", "4,50"], dict(mid_occ=4), dict(max_occ=50)),            # the rescue round fires where the best chain holds one mate only
    "pe.f4_4": (["-x", "sr", "-f", "4,4"], dict(mid_occ=4), dict(max_occ=4)),                 # max_occ = mid_occ: no rescue
    "pe.2nd": (["-x", "sr", "--secondary=yes"], dict(flag=0x1000 | 0x2000 | 0x400000), {}),   # MM_F_NO_PRINT_2ND cleared
    "pe.sorted": (["-x", "sr", "--heap-sort=no"], dict(flag=0x1000 | 0x2000 | 0x4000), {}),   # MM_F_HEAP_SORT cleared
}
# (the program has no option for pe_ori: no "pe.rf" run.  main.c:316-318 sets max_chain_skip to INT32_MAX under MM_F_SR, so that is what every run was made with: the
# fixture records it under options.max_chain_skip and the tests map with it)


def _write_inputs(d, ctg, rd):
    with open(os.path.join(d, "ref.fa"), "wb") as fh:
        for n, s in ctg:
            fh.write(b">" + n.encode() + b"\n" + s + b"\n")
    with open(os.path.join(d, "reads.fa"), "wb") as fh:
        for n, s in rd:
            fh.write(b">" + n.encode() + b"\n" + s + b"\n")


def record_paf(ctg, rd, args, two_files=None):
    """What the reference program prints for a run on the interleaved file; two_files: (reads1, reads2) given as two files instead."""
    with tempfile.TemporaryDirectory() as d:
        _write_inputs(d, ctg, rd)
        files = [os.path.join(d, "reads.fa")]
        if two_files:
            files = []
            for k, part in enumerate(two_files):
                files.append(os.path.join(d, f"r{k + 1}.fa"))
                with open(files[-1], "wb") as fh:
                    for n, s in part:
                        fh.write(b">" + n.encode() + b"\n" + s + b"\n")
        return subprocess.run([REF_EXE, "-t", "1"] + args + [os.path.join(d, "ref.fa")] + files, check=True, capture_output=True).stdout.decode()


def record_seeds(ctg, rd):
    """Per fragment {"rep_len": n, "sd": [[contig, strand, rpos, qpos, span]]} from the stderr of --print-seeds: QR opens a fragment, the first RS block is the round at
    mid_occ (the rescue round prints a second one, left out)."""
    ids = {n: i for i, (n, _) in enumerate(ctg)}
    with tempfile.TemporaryDirectory() as d:
        _write_inputs(d, ctg, rd)
        err = subprocess.run([REF_EXE, "-t", "1", "-x", "sr", "--print-seeds", os.path.join(d, "ref.fa"), os.path.join(d, "reads.fa")], check=True, capture_output=True).stderr.decode()
    out, cur = [], None
    for ln in err.splitlines():
        f = ln.split("\t")
        if f[0] == "QR":
            cur = dict(name=f[1], rep_len=None, sd=[], blocks=0)
            out.append(cur)
        elif f[0] == "RS":
            cur["blocks"] += 1
            if cur["blocks"] == 1:
                cur["rep_len"] = int(f[1])
        elif f[0] == "SD" and cur["blocks"] == 1:
            cur["sd"].append([ids[f[1]], int(f[3] == "-"), int(f[2]), int(f[4]), int(f[5])])
    return out


def golden_paf(run):
    return gold()["pafs"][run]


def map_run(engine, run, stream=False, rd=None, pe_ori=1, **fields):
    """A recorded run through this project's mapper on the fixture's fragments: (PAF text, stats)."""
    _, opt_kw, sr_kw = RUNS[run]
    fields.setdefault("max_chain_skip", gold()["options"]["max_chain_skip"])
    opt = mm.map_opt_sr(host_threads=4, **dict(opt_kw, **fields))
    rd = reads() if rd is None else rd
    names = [n for n, _ in contigs()]
    kw = dict(opt=opt, k=K, align=mm.map_sr(**sr_kw), frags=mm.frag_offsets([n for n, _ in rd]), pe_ori=pe_ori)
    if stream:
        return mm.map_reads_stream([engine], index(), names, rd, chunk_bases=5_000, **kw)
    return mm.map_reads(engine, index(), names, rd, **kw)


def worth_having(pafs, se):
    """What makes the set worth having, asserted by the generator on a fresh set and by the CPU suite on the committed one: {condition: bool}."""
    rows = {run: [ln.split("\t") for ln in text.splitlines()] for run, text in pafs.items()}
    one = {}                                            # a mate's single-end line, where it has exactly one
    for f in (ln.split("\t") for ln in se.splitlines()):
        one.setdefault(f[0], []).append(f)
    moved = [f[0] for f in rows["pe"] if len(one.get(f[0], [])) == 1 and (one[f[0]][0][5] != f[5] or one[f[0]][0][11] != f[11])
             and sum(g[0] == f[0] for g in rows["pe"]) == 1]
    n_p = {}
    for f in rows["pe"]:
        if "tp:A:P" in f:
            n_p[f[0]] = n_p.get(f[0], 0) + 1
    return {"1 a mate's line differs from single-end in target or mapq": bool(moved),
            "2 -f 4,50 and -f 4,4 differ": pafs["pe.f4_50"] != pafs["pe.f4_4"],
            "3 a line with cm:i:1": any("cm:i:1" in f for f in rows["pe"]),
            "4 a mate with two tp:A:P lines": any(v >= 2 for v in n_p.values()),
            "5 --secondary=yes prints tp:A:S lines": any("tp:A:S" in f for f in rows["pe.2nd"])}


# ---------------------------------------------------------------- mm_select_sub_multi and mm_seg_gen of the built reference, through ctypes
class _Seg(C.Structure):
    """mm_seg_t (mmpriv.h:48-52)."""
    _fields_ = [("n_u", C.c_int), ("n_a", C.c_int), ("u", C.c_void_p), ("a", C.c_void_p)]


def frag_hash(f):
    return (f * 2654435761 + 97) & 0xffffffff


def max_dist_x(o, sr, qlen_sum):
    return o.max_gap_ref if o.max_gap_ref > 0 else max(sr.max_frag_len - qlen_sum if sr.max_frag_len > 0 else o.max_gap, o.max_gap)


def ref_post(anchors, qlens, f_id, mo, k):
    """A two-mate fragment's heap-order anchors through the reference: mg_lchain_dp at n_seg = 2, mm_gen_regs with qlen_sum, mm_set_parent, then mm_select_sub_multi and
    mm_seg_gen.  Returns dict(regs_in, regs_kept, anchors, seg=[(records, anchors) per mate]) of numpy snapshots (REG_DTYPE records, (m,2) uint64 anchors)."""
    import align_cases as ac
    L = ac.ref_lib()
    L.mm_select_sub_multi.restype = None
    L.mm_select_sub_multi.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int), C.c_void_p]
    L.mm_seg_gen.restype = C.POINTER(_Seg)
    L.mm_seg_gen.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    a = np.ascontiguousarray(anchors, dtype=np.uint64).reshape(-1, 2)
    empty = dict(regs_in=np.zeros(0, mm.REG_DTYPE), regs_kept=np.zeros(0, mm.REG_DTYPE), anchors=np.zeros((0, 2), np.uint64),
                 seg=[(np.zeros(0, mm.REG_DTYPE), np.zeros((0, 2), np.uint64)) for _ in qlens])
    if len(a) == 0:
        return empty
    qsum = int(sum(qlens))
    ql = (C.c_int * 2)(*qlens)
    n_u, u_ptr = C.c_int(0), C.c_void_p(0)
    buf = ac._libc.malloc(a.nbytes)
    C.memmove(buf, a.ctypes.data, a.nbytes)
    pen_gap, pen_skip = np.float32(mo.chain_gap_scale * 0.01 * k), np.float32(mo.chain_skip_scale * 0.01 * k)
    max_x = mo.max_gap_ref if mo.max_gap_ref > 0 else max(mo.max_frag_len - qsum if mo.max_frag_len > 0 else mo.max_gap, mo.max_gap)
    out = L.mg_lchain_dp(max_x, max(qsum, mo.max_gap), mo.bw, mo.max_chain_skip, mo.max_chain_iter, mo.min_cnt, mo.min_chain_score, pen_gap, pen_skip, 0, len(qlens), len(a), buf,
                         C.byref(n_u), C.byref(u_ptr), None)
    if n_u.value == 0:
        return empty
    regs = L.mm_gen_regs(None, frag_hash(f_id), qsum, n_u.value, u_ptr, out, 0)
    n_out = int((np.ctypeslib.as_array(C.cast(u_ptr, C.POINTER(C.c_uint64)), shape=(n_u.value,)) & 0xffffffff).sum())
    ac._libc.free(u_ptr)
    kept_a = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint64)), shape=(n_out, 2)).copy()
    n = C.c_int(n_u.value)
    L.mm_set_parent(None, mo.mask_level, mo.mask_len, n.value, regs, mo.a * 2 + mo.b, int(bool(mo.flag & 0x20000000)), mo.alt_drop)
    regs_in = ac._snap_regs(regs, n.value)[0]
    L.mm_select_sub_multi(None, mo.pri_ratio, 0.2, 0.7, max_x, k * 2, mo.best_n, len(qlens), ql, C.byref(n), regs)
    regs_kept = ac._snap_regs(regs, n.value)[0]
    n_regs, seg_regs = (C.c_int * 2)(), (C.c_void_p * 2)()
    seg = L.mm_seg_gen(None, frag_hash(f_id), len(qlens), ql, n.value, regs, n_regs, seg_regs, out)
    per = []
    for s in range(len(qlens)):
        sa = np.ctypeslib.as_array(C.cast(seg[s].a, C.POINTER(C.c_uint64)), shape=(seg[s].n_a, 2)).copy() if seg[s].n_a else np.zeros((0, 2), np.uint64)
        per.append((ac._snap_regs(seg_regs[s], n_regs[s])[0], sa))
    return dict(regs_in=regs_in, regs_kept=regs_kept, anchors=kept_a, seg=per)


def save_post(path, posts, qlens):
    """post.npz: per two-mate fragment the records before and after mm_select_sub_multi, its kept anchors, and per mate mm_seg_gen's records and anchors, end to end."""
    cat = lambda xs, dt, shape=(0,): np.concatenate(xs) if len(xs) else np.zeros(shape, dt)
    off = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)
    seg_r = [p["seg"][s][0] for p in posts for s in range(2)]
    seg_a = [p["seg"][s][1] for p in posts for s in range(2)]
    np.savez_compressed(path, qlens=np.asarray(qlens, np.int32).reshape(-1, 2), in_off=off([p["regs_in"] for p in posts]), regs_in=cat([p["regs_in"] for p in posts], mm.REG_DTYPE),
                        kept_off=off([p["regs_kept"] for p in posts]), regs_kept=cat([p["regs_kept"] for p in posts], mm.REG_DTYPE),
                        a_off=off([p["anchors"] for p in posts]), anchors=cat([p["anchors"] for p in posts], np.uint64, (0, 2)),
                        seg_r_off=off(seg_r), seg_regs=cat(seg_r, mm.REG_DTYPE), seg_a_off=off(seg_a), seg_anchors=cat(seg_a, np.uint64, (0, 2)))


def golden_post():
    """The committed post.npz as lists per two-mate fragment: dict(qlens, regs_in, regs_kept, anchors, seg=[(records, anchors)] * 2)."""
    z = np.load(os.path.join(GOLD, "post.npz"))
    cut = lambda a, off: [a[off[i]:off[i + 1]] for i in range(len(off) - 1)]
    seg_r, seg_a = cut(z["seg_regs"], z["seg_r_off"]), cut(z["seg_anchors"], z["seg_a_off"])
    n = len(z["qlens"])
    return [dict(qlens=[int(v) for v in z["qlens"][f]], regs_in=r_in, regs_kept=r_k, anchors=a, seg=[(seg_r[2 * f + s], seg_a[2 * f + s]) for s in range(2)])
            for f, (r_in, r_k, a) in enumerate(zip(cut(z["regs_in"], z["in_off"]), cut(z["regs_kept"], z["kept_off"]), cut(z["anchors"], z["a_off"])))][:n]


# ---------------------------------------------------------------- crafted records and anchors
def reg(i, parent, score, rid, rev, rs, re, qs, qe, cnt=5, as_=0):
    r = np.zeros(1, mm.REG_DTYPE)
    r["id"], r["parent"], r["score"], r["score0"], r["rid"], r["rs"], r["re"], r["qs"], r["qe"], r["cnt"], r["as_"] = i, parent, score, score, rid, rs, re, qs, qe, cnt, as_
    r["flags"] = (1 << 10) if rev else 0
    r["div"], r["mlen"], r["blen"], r["hash"] = -1.0, qe - qs, qe - qs, 1000 - i
    return r


def select_literal(regs, qlens, max_gap_ref, pri_ratio, pri1, pri2, min_diff, best_n):
    """pe.c:6-43 in plain Python on REG_DTYPE records: the indices that stay (the squeeze in place included: r[parent] is read from the array as squeezed so far)."""
    r = [dict(parent=int(x["parent"]), score=int(x["score"]), rev=int(x["flags"]) >> 10 & 1, rid=int(x["rid"]), rs=int(x["rs"]), re=int(x["re"]), qs=int(x["qs"]),
              qe=int(x["qe"]), src=i) for i, x in enumerate(regs)]
    n_segs = len(qlens)
    max_dist = qlens[0] + qlens[1] + max_gap_ref if n_segs == 2 else 0
    k = n_2nd = 0
    for i in range(len(r)):
        q = r[i]
        if q["parent"] == i:
            keep = True
        elif q["score"] + min_diff >= r[q["parent"]]["score"]:
            keep = True
        else:
            p = r[q["parent"]]
            if p["rev"] == q["rev"] and p["rid"] == q["rid"] and q["re"] - p["rs"] < max_dist and p["re"] - q["rs"] < max_dist:
                keep = q["score"] >= np.float32(p["score"]) * np.float32(pri1)
            else:
                par_both = n_segs == 2 and p["qs"] < qlens[0] < p["qe"]
                chi_both = n_segs == 2 and q["qs"] < qlens[0] < q["qe"]
                keep = q["score"] >= np.float32(p["score"]) * np.float32(pri_ratio if chi_both or chi_both == par_both else pri2)
        if keep and q["parent"] != i:
            n_2nd += 1
            if n_2nd > best_n:
                keep = False
        if keep:
            r[k] = q
            k += 1
    return [x["src"] for x in r[:k]]


def anchor(rpos, qpos, seg, rev=False, rid=0, span=21):
    return [(1 << 63 if rev else 0) | rid << 32 | rpos, seg << 48 | span << 32 | qpos]


def seg_literal(regs, anchors, qlens):
    """hit.c:331-375 in plain Python: per mate (u, anchors) -- u = score << 32 | the mate's anchors of every record that has some, the anchors with y in the mate's own
    coordinates -- before mm_gen_regs orders the chains."""
    a = np.asarray(anchors, np.uint64).reshape(-1, 2)
    acc = [0, qlens[0]] if len(qlens) == 2 else [0]
    qsum = sum(qlens)
    out = []
    for s in range(len(qlens)):
        u, sa = [], []
        for x in regs:
            n = 0
            for j in range(int(x["cnt"])):
                ax, ay = int(a[int(x["as_"]) + j][0]), int(a[int(x["as_"]) + j][1])
                if ay >> 48 & 0xff != s:
                    continue
                ay -= qsum - (qlens[s] + acc[s]) if ax >> 63 else acc[s]
                sa.append([ax, ay])
                n += 1
            if n:
                u.append(int(x["score"]) << 32 | n)
        out.append((u, np.asarray(sa, np.uint64).reshape(-1, 2)))
    return out


# ---------------------------------------------------------------- crafted fragments for the device seeding
W = 11
TANDEM_UNIT, TANDEM_COPIES = 31, 24


def crafted_genome(seed=17):
    """A 30 kb sequence: random, but for a 24 x 31-base tandem array at 8000 and eight copies of a 300-base repeat from 12000 on, 1500 apart."""
    rng = np.random.default_rng(seed)
    g = sim_reads.BASES[rng.integers(0, 4, 30_000)].copy()
    g[8_000:8_000 + TANDEM_UNIT * TANDEM_COPIES] = np.tile(sim_reads.BASES[rng.integers(0, 4, TANDEM_UNIT)], TANDEM_COPIES)
    rep = sim_reads.BASES[rng.integers(0, 4, 300)]
    for c in range(8):
        g[12_000 + 1_500 * c:12_300 + 1_500 * c] = rep
    return g.tobytes()


def boundary_twin(g):
    """Two mates cut from one stretch so that mate 0's last minimizer and mate 1's first are the same k-mer: neighbours of equal value in the joint list, in neither mate's own."""
    for a in range(1_000, 1_400):
        m0 = g[a:a + 100]
        sk0 = mm.sketch(m0, W, K)
        st = a + (int(sk0[-1][1] & 0xffffffff) >> 1) - K + 1
        m1 = g[st:st + 100]
        sk1 = mm.sketch(m1, W, K)
        own = lambda sk: any(int(sk[i][0]) >> 8 == int(sk[i + 1][0]) >> 8 for i in range(len(sk) - 1))
        if len(sk1) and int(sk1[0][0]) >> 8 == int(sk0[-1][0]) >> 8 and not own(sk0) and not own(sk1):
            return [m0, m1]
    raise AssertionError("no such pair of mates in the stretch")


def crafted_frags():
    """(genome, {name: (mates as they are mapped, seed options)}): the smallest shapes at which the fragment view can go wrong."""
    g = crafted_genome()
    opt = dict(mid_occ=1000, max_max_occ=4095, occ_dist=500, q_occ_frac=0.01)
    low = dict(opt, mid_occ=4, max_max_occ=20, occ_dist=50)             # the repeat's minimizers (8 copies) are high-occurrence ones
    out = {}
    out["first_mate_below_k"] = ([g[2_000:2_010], g[2_300:2_400]], opt)
    out["second_mate_below_k"] = ([g[3_000:3_100], g[3_300:3_312]], opt)
    out["both_below_k"] = ([g[3_500:3_515], g[3_600:3_620]], opt)
    out["empty_first_mate"] = ([b"", g[3_700:3_800]], opt)
    out["twin_across_boundary"] = (boundary_twin(g), opt)
    # mate 0 ends inside a copy of the repeat and mate 1 begins inside another: one streak of dropped minimizers runs across the boundary
    out["streak_across_boundary"] = ([g[11_900:12_150], g[13_650:13_900]], low)
    out["streak_fills_both"] = ([g[12_020:12_280], g[15_020:15_280]], low)
    # either mate holds each of the tandem unit's minimizers about 8 times (<= mid_occ 10), the joint list about 16 times: seed.c:5-30 fires for the fragment alone
    out["q_filter_joint_only"] = ([g[8_000:8_000 + 8 * TANDEM_UNIT + 10], g[8_000 + 10 * TANDEM_UNIT:8_000 + 18 * TANDEM_UNIT + 10]], dict(opt, mid_occ=10, max_max_occ=50, occ_dist=50))
    out["single"] = ([g[20_000:20_150]], opt)
    out["single_in_repeat"] = ([g[16_500:16_800]], low)
    return g, out


def dump_replay(path):
    """The file tests/tools/pe_replay.cpp replays: the fixture as the host calls take it, and what they must give."""
    o, sr = mm.map_opt_sr(), mm.map_sr()
    frags, gp = fragments(), golden_post()
    rd = [(n, s) for f in frags for (n, _), s in zip(f, oriented(f))]
    m = matches_frag(frags)
    ids = [i for i, f in enumerate(frags) if len(f) == 2]
    off = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)
    cat = lambda xs, dt, shape=(0,): np.ascontiguousarray(np.concatenate(xs) if sum(len(x) for x in xs) else np.zeros(shape, dt))
    seg_r = [p["seg"][s][0] for p in gp for s in range(2)]
    seg_a = [p["seg"][s][1] for p in gp for s in range(2)]
    regs_in, regs_kept, anchors = cat([p["regs_in"] for p in gp], mm.REG_DTYPE), cat([p["regs_kept"] for p in gp], mm.REG_DTYPE), cat([p["anchors"] for p in gp], np.uint64, (0, 2))
    head = np.asarray([len(contigs()), len(rd), len(frags), K, W, o.mid_occ, o.max_max_occ, o.occ_dist, len(gp), len(regs_in), len(regs_kept), len(anchors),
                       sum(len(x) for x in seg_r), sum(len(x) for x in seg_a), 2 * K, o.best_n], np.int64)

    def strings(xs):
        return [np.asarray([len(x) for x in xs], np.int32)] + [np.frombuffer(bytes(x), np.uint8) for x in xs]
    parts = [head, np.asarray([o.q_occ_frac, o.pri_ratio, 0.2, 0.7], np.float32)] + strings([s for _, s in contigs()]) + strings([n.encode() for n, _ in rd]) + strings([s for _, s in rd])
    parts += [mm.frag_offsets([n for n, _ in rd]).astype(np.int32), np.asarray([len(x["seeds"]) for x in m], np.int32), np.asarray([x["rep_len"] for x in m], np.int32),
              np.asarray([len(x["hits"]) for x in m], np.int64)]
    parts += [np.asarray([p["qlens"] for p in gp], np.int32), np.full(len(gp), 2, np.int32), np.asarray([max_dist_x(o, sr, sum(p["qlens"])) for p in gp], np.int32),
              np.asarray([frag_hash(i) for i in ids], np.uint32), off([p["regs_in"] for p in gp]), off([p["regs_kept"] for p in gp]), off([p["anchors"] for p in gp]),
              regs_in, regs_kept, anchors, off(seg_r), off(seg_a), cat(seg_r, mm.REG_DTYPE), cat(seg_a, np.uint64, (0, 2))]
    with open(path, "wb") as fh:
        for a in parts:
            fh.write(np.ascontiguousarray(a).tobytes())
