"""Cases for the = / X rewrite (mm2gb_cigar_eqx_*): records built from a list of segments together with the words they must give, and the
committed vectors (tests/golden/sam/eqx_*.npz: the words mm_align_skeleton left under MM_F_EQX for the batches of tests/golden/align, recorded by
tests/tools/gen_golden_sam.py).  Test infrastructure only: imported by tests/test_eqx_cpu.py, tests/test_gpu_eqx.py, tests/tools/gen_golden_sam.py
and profiles/eqx_rate.py."""
import os

import numpy as np

import align_cases as ac
import aln_text_cases as at
import golden_io
import mm2gb_amd as mm

GOLD = os.path.join(golden_io.GOLD, "sam")
BATCHES = at.BATCHES
SLICE, WG = 2048, 256          # the device form's cuts and rounds (Engine.cigar_eqx_info)
M, I, D, N, EQ, X = 0, 1, 2, 3, 7, 8


def w(n, op):
    return n << 4 | op


def build(segs, seed=0, rev=False, lead=(0, 0), tail=(0, 0)):
    """One record from segments, with the words it gives and the words it must give.  A segment is (kind, n): "=" n matching bases, "X" n
    mismatches, "n" n columns of N against N (a match), "I" / "D" an insertion / a deletion, "N" an intron of n bases, "W" (n ignored) a boundary
    between two M words.  Consecutive "=" / "X" / "n" segments lie in one M word; runs of one equality merge inside a word and never across words.
    Returns dict(ref, read, reg, words, want)."""
    rng = np.random.default_rng(seed)
    L = np.frombuffer(b"ACGT", np.uint8)
    t, q, words, want = [], [], [], []
    open_m = False          # the last word is an M word that the next column joins
    last_eq = None          # ... and the equality of its last run
    def column_run(n, eq):
        nonlocal open_m, last_eq
        if open_m:
            words[-1] += n << 4
        else:
            words.append(w(n, M))
        if open_m and last_eq == eq:
            want[-1] += n << 4
        else:
            want.append(w(n, EQ if eq else X))
        open_m, last_eq = True, eq
    for kind, n in segs:
        if kind == "W":
            open_m = False
        elif kind == "=":
            b = L[rng.integers(0, 4, n)].tobytes()
            t.append(b); q.append(b); column_run(n, True)
        elif kind == "n":
            t.append(b"N" * n); q.append(b"N" * n); column_run(n, True)
        elif kind == "X":
            x = rng.integers(0, 4, n); y = (x + rng.integers(1, 4, n)) % 4
            t.append(L[x].tobytes()); q.append(L[y].tobytes()); column_run(n, False)
        elif kind == "I":
            q.append(L[rng.integers(0, 4, n)].tobytes()); words.append(w(n, I)); want.append(w(n, I)); open_m = False
        elif kind in ("D", "N"):
            t.append(L[rng.integers(0, 4, n)].tobytes()); words.append(w(n, D if kind == "D" else N)); want.append(words[-1]); open_m = False
        else:
            raise ValueError(kind)
    t, q = b"".join(t), b"".join(q)
    pad = lambda n: L[rng.integers(0, 4, n)].tobytes()
    ref = pad(lead[0]) + t + pad(tail[0])
    read = pad(lead[1]) + q + pad(tail[1])
    reg = np.zeros(1, mm.REG_DTYPE)
    reg["rs"], reg["re"], reg["qs"], reg["qe"] = lead[0], lead[0] + len(t), lead[1], lead[1] + len(q)
    if rev:                                                       # the read as sequenced is the other strand: qs counts from its own start
        read = at.revcomp(read)
        reg["qs"], reg["qe"], reg["flags"] = tail[1], tail[1] + len(q), 1 << 10
    return dict(ref=ref, read=read, reg=reg, words=np.array(words, np.uint32), want=np.array(want, np.uint32))


def batch(recs):
    """Records of build() as one call's arguments (aln_text_cases.batch)."""
    return at.batch(recs)


def split(aln, words):
    return [words[int(a["cigar_off"]):int(a["cigar_off"]) + int(a["n_cigar"])] if a["cigar_off"] >= 0 else None for a in aln]


def assert_words(got, want, what):
    """got: (aln, words) of a call; want: per record the expected words (None: no CIGAR)"""
    g = split(*got)
    assert len(g) == len(want), f"{what}: {len(g)} records against {len(want)}"
    at_word = 0
    for i, (x, y) in enumerate(zip(g, want)):
        if y is None:
            assert x is None, f"{what}: record {i} has no CIGAR and got words"
            continue
        assert int(got[0]["cigar_off"][i]) == at_word, f"{what}: record {i}: its words do not follow the record before"
        at_word += len(y)
        if not np.array_equal(x, y):
            k = next((k for k in range(min(len(x), len(y))) if x[k] != y[k]), min(len(x), len(y)))
            show = lambda v: " ".join(f"{int(u) >> 4}{'MIDNSHP=X'[int(u) & 0xf]}" for u in v[max(k - 3, 0):k + 4])
            raise AssertionError(f"{what}: record {i}: {len(x)} words against {len(y)}, first difference at word {k}: got [{show(x)}] want [{show(y)}]")


# the shapes at which the device form can go wrong (cuts every SLICE columns, rounds of WG): name -> segments
def crafted():
    out = {
        "one_run_5000": [("=", 5000)],
        "flip_at_2047": [("=", 2047), ("X", 1), ("=", 2952)],
        "flip_at_2048": [("=", 2048), ("X", 1), ("=", 2951)],
        "flip_at_255": [("=", 255), ("X", 1), ("=", 4744)],
        "flip_at_256": [("=", 256), ("X", 1), ("=", 4743)],
        "m_begins_at_2048_after_i": [("=", 2040), ("I", 8), ("=", 300)],
        "i_straddles_a_cut": [("=", 2040), ("I", 20), ("=", 300)],
        "d_straddles_a_cut": [("X", 2045), ("D", 9), ("=", 2100)],
        "alternating_4100": [("=" if k % 2 == 0 else "X", 1) for k in range(4100)],
        "n_words_around_a_cut": [("=", 2047), ("N", 150), ("=", 1), ("N", 90), ("=", 2100), ("X", 3), ("N", 64), ("=", 40)],
        "long_mismatch_over_cuts": [("=", 10), ("X", 4500), ("=", 3)],
        "words_meet_at_a_cut": [("=", 2048), ("W", 0), ("=", 2048), ("W", 0), ("X", 5)],
    }
    return out


def golden_args(name):
    return at.golden_args(name)


def golden_splice_args():
    """The records and words the reference left for the `default` batch of tests/golden/splice."""
    import splice_cases
    return splice_cases.golden_text_args("default")


def load_words(name):
    """Per record of the batch the recorded = / X words (None for a record without a CIGAR)."""
    z = np.load(os.path.join(GOLD, f"eqx_{name}.npz"))
    return [None if z["n"][i] < 0 else z["words"][int(z["off"][i]):int(z["off"][i]) + int(z["n"][i])] for i in range(len(z["n"]))]


def ref_words(refs, reads, preset, anchors=None, **over):
    """mm_align_skeleton with MM_F_EQX set (oracle/_ref/libminimap2ref.so): (regs, read_of_reg, aln, cigar) flat, as flatten_aligned gives them."""
    ri = ac.RefIndex(refs, preset)
    flag = ri.mo.flag
    ri.close()
    _, want = ac.ref_batch(refs, reads, preset, anchors=anchors, flag=flag | mm.F_EQX, **over)
    return mm.flatten_aligned(want)
