"""Cases for the text of the alignment tags (mm2gb_aln_text_*): records built from a list of segments together with the text they must give,
the committed fixtures (tests/golden/paf_aln/text_*.npz: what the reference's mm_gen_cs_or_MD printed for the records of tests/golden/align)
and the reference's mm_gen_cs_or_MD through ctypes (oracle/_ref/libminimap2ref.so, where it is built).  Test infrastructure only: imported by
tests/test_aln_text_cpu.py, tests/test_gpu_aln_text.py, tests/tools/gen_golden_paf_aln.py and profiles/aln_text_rate.py."""
import ctypes as C
import os

import numpy as np

import align_cases as ac
import golden_io
import mm2gb_amd as mm

GOLD = os.path.join(golden_io.GOLD, "paf_aln")
BATCHES = ["ont", "pb", "small_mat", "end_bonus", "inv_pair"]
# name -> (what, is_MD, no_iden): the three forms mm_gen_cs_or_MD has
MODES = {"cs": (mm.TEXT_CS, 0, 1), "cs_long": (mm.TEXT_CS | mm.TEXT_CS_LONG, 0, 0), "md": (mm.TEXT_MD, 1, 0)}
TAG = {"cs": b"\tcs:Z:", "cs_long": b"\tcs:Z:", "md": b"\tMD:Z:"}
WHATS = [mm.TEXT_CG, mm.TEXT_CS, mm.TEXT_CS | mm.TEXT_CS_LONG, mm.TEXT_MD, mm.TEXT_CG | mm.TEXT_CS, mm.TEXT_CG | mm.TEXT_CS | mm.TEXT_CS_LONG, mm.TEXT_CG | mm.TEXT_MD,
         mm.TEXT_CS | mm.TEXT_MD, mm.TEXT_CG | mm.TEXT_CS | mm.TEXT_CS_LONG | mm.TEXT_MD, 0]
_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def revcomp(s):
    return bytes(s).translate(_COMP)[::-1]


# ---------------------------------------------------------------- records from segments
def build(segs, seed=0, rev=False, lead=(0, 0), tail=(0, 0)):
    """One record from segments, with the text it must give.  A segment is (kind, n): "=" n matching bases, "X" n mismatches, "I" / "D" an
    insertion / a deletion of n bases, "W" (n ignored) a word boundary between two M words.  Two "=" follow each other only across a "W".
    lead / tail: unrelated bases before and after the stretch in (target, query).  Returns dict(ref, read, reg, words, cg, cs, cs_long, md)."""
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
    if rev:                                                       # the read as sequenced is the other strand: qs counts from its own start
        read = revcomp(read)
        reg["qs"], reg["qe"], reg["flags"] = tail[1], tail[1] + len(q), 1 << 10
    w = np.array([n << 4 | op for op, n in words], np.uint32)
    return dict(ref=ref, read=read, reg=reg, words=w, cg=mm.cigar_string(w).encode(), cs=b"".join(cs), cs_long=b"".join(csl), md=b"".join(md))


def random_segs(rng, n_cols, match=40):
    """Segments of about n_cols columns: match runs of about `match` bases between mismatches, insertions and deletions, now and then a second M word."""
    segs, n = [], 0
    while n < n_cols:
        k = int(rng.geometric(1.0 / match))
        segs.append(("=", k)); n += k
        u = rng.random()
        kind, k = ("X", int(rng.integers(1, 3))) if u < 0.5 else ("I", int(rng.integers(1, 6))) if u < 0.72 else ("D", int(rng.integers(1, 6))) if u < 0.94 else ("W", 0)
        segs.append((kind, k)); n += k
    return segs


def batch(recs):
    """Records of build() as one call's arguments: every record on a reference and a read of its own.  Returns (refs, reads, regs, read_of_reg, aln, cigar)."""
    regs = np.concatenate([r["reg"] for r in recs]) if recs else np.zeros(0, mm.REG_DTYPE)
    aln = np.zeros(len(recs), mm.ALN_DTYPE)
    at = 0
    for i, r in enumerate(recs):
        regs["rid"][i] = i
        if r.get("no_cigar"):
            aln["cigar_off"][i] = -1
            continue
        aln["cigar_off"][i], aln["n_cigar"][i] = at, len(r["words"])
        at += len(r["words"])
    cigar = np.concatenate([r["words"] for r in recs if not r.get("no_cigar")]) if at else np.zeros(0, np.uint32)
    return [r["ref"] for r in recs], [r["read"] for r in recs], regs, np.arange(len(recs), dtype=np.int32), aln, cigar


def expected(recs, what):
    """The text the records of build() must give for `what`, record by record."""
    out = []
    for r in recs:
        s = b""
        if not r.get("no_cigar"):
            if what & mm.TEXT_CG:
                s += b"\tcg:Z:" + r["cg"]
            if what & mm.TEXT_MD:
                s += b"\tMD:Z:" + r["md"]
            elif what & mm.TEXT_CS:
                s += b"\tcs:Z:" + (r["cs_long"] if what & mm.TEXT_CS_LONG else r["cs"])
        out.append(s)
    return out


def split(off, text):
    return [text[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]


def assert_texts(got, want, what):
    assert len(got) == len(want), f"{what}: {len(got)} records against {len(want)}"
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    if bad:
        g, w = got[bad[0]], want[bad[0]]
        at = next((k for k in range(min(len(g), len(w))) if g[k] != w[k]), min(len(g), len(w)))
        raise AssertionError(f"{what}: {len(bad)} records differ, first record {bad[0]} at byte {at} (lengths {len(g)} / {len(w)}): got {g[max(at - 20, 0):at + 20]!r} want {w[max(at - 20, 0):at + 20]!r}")


# ---------------------------------------------------------------- the fixtures
def golden_args(name):
    """The records and words the reference left for a fixture batch of tests/golden/align, as aln_text_* takes them."""
    b, want = ac.load_batch(name)
    return (b["refs"], b["reads"]) + mm.flatten_aligned(want)


def load_texts(name):
    """mode -> list of bytes, one per record (empty for a record without a CIGAR), without the tag's name."""
    z = np.load(os.path.join(GOLD, f"text_{name}.npz"))
    return {m: split(z[m + "_off"], z[m].tobytes()) for m in MODES}


def want_for(args, texts, what):
    """What a call must return for `what`, from the recorded texts and the cg rule."""
    _, _, regs, _, aln, cigar = args
    out = []
    for i in range(len(regs)):
        s = b""
        if aln["cigar_off"][i] >= 0:
            if what & mm.TEXT_CG:
                s += b"\tcg:Z:" + mm.cigar_string(cigar[int(aln["cigar_off"][i]):int(aln["cigar_off"][i] + aln["n_cigar"][i])]).encode()
            m = "md" if what & mm.TEXT_MD else "cs_long" if what & mm.TEXT_CS and what & mm.TEXT_CS_LONG else "cs" if what & mm.TEXT_CS else None
            if m:
                s += TAG[m] + texts[m][i]
        out.append(s)
    return out


# ---------------------------------------------------------------- the reference through ctypes
class _Reg1(C.Structure):
    _fields_ = [("head", C.c_uint8 * 72), ("p", C.c_void_p)]


def ref_texts(refs, reads, regs, read_of_reg, aln, cigar):
    """mm_gen_cs_or_MD (format.c:251) on every record: mode -> list of bytes."""
    L = ac.ref_lib()
    L.mm_gen_cs_or_MD.restype = C.c_int
    L.mm_gen_cs_or_MD.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_int]
    ri = ac.RefIndex(refs, "map-ont")
    out = {m: [] for m in MODES}
    buf, cap = C.c_void_p(0), C.c_int(0)
    try:
        for i in range(len(regs)):
            if aln["cigar_off"][i] < 0:
                for m in MODES:
                    out[m].append(b"")
                continue
            w = np.ascontiguousarray(cigar[int(aln["cigar_off"][i]):int(aln["cigar_off"][i] + aln["n_cigar"][i])], np.uint32)
            extra = C.create_string_buffer(bytes(ac._Extra(len(w), int(aln["dp_score"][i]), int(aln["dp_max"][i]), int(aln["dp_max2"][i]), 0, len(w))) + w.tobytes())
            r1 = _Reg1()
            C.memmove(r1.head, regs[i:i + 1].tobytes(), 72)
            r1.p = C.addressof(extra)
            for m, (_, is_md, no_iden) in MODES.items():
                n = L.mm_gen_cs_or_MD(None, C.byref(buf), C.byref(cap), ri.mi, C.byref(r1), bytes(reads[int(read_of_reg[i])]), is_md, no_iden, 0)
                out[m].append(C.string_at(buf.value, n))
    finally:
        ac._libc.free(buf)
        ri.close()
    return out
