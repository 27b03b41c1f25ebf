"""A reference with satellite arrays and a microsatellite, reads on them, and numpy models, for tests/test_hiocc_cpu.py and
tests/test_gpu_hiocc.py: minimizers that occur 10^3 to 10^5 times, where the radix select of the device's mid_occ, the bit-by-bit select of
the match thinning, the max_max_occ rule and the copy of long occurrence runs first do something.  tests/tools/gen_golden_hiocc.py recorded
the reference on exactly these sequences (tests/golden/hiocc; meta.json pins them by md5).  No GPU needed."""
import functools
import glob
import hashlib
import json
import os

import numpy as np

import golden_io
import sim_reads

B = sim_reads.BASES
HIOCC = os.path.join(golden_io.GOLD, "hiocc")
INT32_MAX = 2**31 - 1
CHR_NAMES = ["chr1", "chr2"]
# the option sets of the match selection (SeedIndex.matches / Engine.collect_matches keywords); "default" and "no thinning" get the index's
# own mid_occ.  THINNING: the sets in which seeding.cpp's thin_out runs (occ_dist > 0 and max_max_occ > mid_occ)
SETS = {"default": dict(), "wide thinning": dict(mid_occ=10, max_max_occ=1 << 20, occ_dist=100), "cap of 128": dict(mid_occ=300, occ_dist=20),
        "mid 50": dict(mid_occ=50), "q filter": dict(mid_occ=5, q_occ_frac=0.01), "no thinning": dict(occ_dist=0),
        "everything kept": dict(mid_occ=1 << 30, max_max_occ=1 << 30, occ_dist=0, q_occ_frac=0.0)}
THINNING = ("default", "wide thinning", "cap of 128", "mid 50", "q filter")
UNFILTERED = SETS["everything kept"]


def satellite(rng, unit_len, copies, div):
    """copies of one random unit in tandem, every base replaced by a random one with probability div."""
    arr = np.tile(B[rng.integers(0, 4, unit_len)], copies)
    mut = rng.random(len(arr)) < div
    arr[mut] = B[rng.integers(0, 4, int(mut.sum()))]
    return arr


@functools.lru_cache(maxsize=None)
def _sequences():
    rng = np.random.default_rng(41)

    def flank(n):
        return B[rng.integers(0, 4, n)]

    # chr1: a 171-mer array (3000 units, 3 % diverged), (AC)n of 140 kb, a 37-mer array (6000 units, 1 %); chr2: a 171-mer array of another
    # unit, 10 % diverged: its minimizers are rare
    chr1 = np.concatenate([flank(60_000), satellite(rng, 171, 3000, .03), flank(60_000), np.tile(np.frombuffer(b"AC", np.uint8), 70_000),
                           flank(30_000), satellite(rng, 37, 6000, .01), flank(30_000)])
    chr2 = np.concatenate([flank(50_000), satellite(rng, 171, 800, .10), flank(50_000)])
    sat, ac, sat37 = 60_000, 60_000 + 3000 * 171 + 60_000, 60_000 + 3000 * 171 + 60_000 + 140_000 + 30_000
    loci = ((sat + 20_000, 12_000),                   # wholly inside the 171-mer array
            (sat - 3_000, 9_000),                     # entering it from the left flank
            (sat + 3000 * 171 - 4_000, 8_000),        # leaving it on the right
            (ac - 2_000, 6_000),                      # 2 kb before (AC)n, ending inside it
            (sat37 + 5_000, 7_000))                   # inside the 37-mer array
    reads = []
    for k, (st, ln) in enumerate(loci):
        r = sim_reads.mutate(rng, chr1[st:st + ln], 0.08)
        reads += [(f"r{k}f", r), (f"r{k}r", sim_reads.revcomp(r))]
    reads.append(("c2", sim_reads.mutate(rng, chr2[52_000:60_000], 0.05)))
    return [chr1, chr2], reads


def genome():
    """The two reference sequences as bytes."""
    return [c.tobytes() for c in _sequences()[0]]


def reads():
    """The 11 reads as (name, bytes): r0f r0r ... r4f r4r on chr1 (each locus and its reverse complement), c2 on chr2."""
    return [(n, s.tobytes()) for n, s in _sequences()[1]]


C2 = 10                     # the chr2 read
UNITS37 = (8, 9)            # the reads inside the 37-mer array


def write_fastas(ref_fa, reads_fa):
    chrs, rd = _sequences()
    sim_reads.write_fasta(ref_fa, list(zip(CHR_NAMES, chrs)))
    sim_reads.write_fasta(reads_fa, rd)


def md5_of(path):
    return hashlib.md5(open(path, "rb").read()).hexdigest()


def meta():
    return json.load(open(os.path.join(HIOCC, "meta.json")))


def sha(arr):
    return hashlib.sha256(np.ascontiguousarray(arr).tobytes()).hexdigest()


def load(path):
    """tests/golden/hiocc/sat_K.npz: what the reference's mm_collect_matches returned for read K -- seeds, mini_pos, rep_len in full, of the
    hits and of the anchors made from them their number and the SHA-256 of their bytes."""
    z = np.load(path)
    m = json.loads(bytes(z["meta"]).decode())
    return dict(m, seeds=z["seeds"], mini_pos=z["mini_pos"])


@functools.lru_cache(maxsize=None)
def fixtures():
    """read number -> record."""
    out = {}
    for p in sorted(glob.glob(os.path.join(HIOCC, "sat_*.npz"))):
        g = load(p)
        out[g["read"]] = g
    return out


def same_as_recorded(m, g, what):
    """A match record (SeedIndex.matches / Engine.collect_matches) against a fixture."""
    assert m["qlen"] == g["qlen"], what
    assert np.array_equal(m["seeds"], g["seeds"]), f"{what}: seeds ({len(m['seeds'])} vs {len(g['seeds'])})"
    assert np.array_equal(m["mini_pos"], g["mini_pos"]) and m["rep_len"] == g["rep_len"], f"{what}: mini_pos / rep_len"
    assert len(m["hits"]) == g["n_hits"] and sha(m["hits"]) == g["hits_sha256"], f"{what}: hits"


def mid_occ_model(first, frac, lo, hi):
    """mm2gb_index_mid_occ (csrc/seeding.cpp) in numpy, from the index's `first` array."""
    cnt = np.sort(np.diff(np.asarray(first, np.int64)).astype(np.uint32))
    n = len(cnt)
    occ = INT32_MAX
    if float(np.float32(frac)) > 0 and n:
        kth = int((1.0 - float(np.float32(frac))) * n) & 0xffffffff
        occ = int(cnt[min(kth, n - 1)]) + 1
    if occ < lo:
        occ = lo
    if hi > lo and occ > hi:
        occ = hi
    return occ


def rank_fracs(n):
    """(rank, frac) with (1 - frac) * n = rank + 0.5: every rank of up to 200 keys, otherwise 200 evenly spaced ranks and the top 40."""
    ranks = np.arange(n) if n <= 200 else np.unique(np.concatenate([np.linspace(0, n - 1, 200).astype(np.int64), np.arange(n - 40, n)]))
    return [(int(r), (n - int(r) - 0.5) / n) for r in ranks]


def streaks(all_matches, qlen, mid_occ, occ_dist):
    """The maximal runs of matches with n > mid_occ in one read's unfiltered matches (ix.matches(s, **UNFILTERED)), as thin_out of
    csrc/seeding.cpp sees them: (lengths, keep, largest n) with keep = min(int((pe - ps) / occ_dist + .499), 128), pe and ps the read
    positions of the matches after and before the run (the read's ends where there is none)."""
    n = all_matches["seeds"][:, 0].astype(np.int64)
    q = (all_matches["seeds"][:, 1] >> 1).astype(np.int64)
    hi = np.concatenate([[False], n > mid_occ, [False]])
    start, end = np.flatnonzero(hi[1:] & ~hi[:-1]), np.flatnonzero(~hi[1:] & hi[:-1])
    lens, keep, nmax = [], [], []
    for i, j in zip(start, end):
        ps, pe = (q[i - 1] if i > 0 else 0), (q[j] if j < len(n) else qlen)
        lens.append(j - i)
        keep.append(min(int((pe - ps) / occ_dist + .499), 128))
        nmax.append(int(n[i:j].max()))
    return np.array(lens, np.int64), np.array(keep, np.int64), np.array(nmax, np.int64)


def streak_figures(all_by_read, qlens, mid_occ, occ_dist):
    """Over all reads: dict(longest, n_long (> 256 matches), thinned (0 < keep < len), capped (keep == 128), dropped (keep <= 0), n_max)."""
    parts = [streaks(m, ql, mid_occ, occ_dist) for m, ql in zip(all_by_read, qlens)]
    lens, keep, nmax = (np.concatenate([p[k] for p in parts]) for k in range(3))
    return dict(longest=int(lens.max()), n_long=int((lens > 256).sum()), thinned=int(((keep > 0) & (keep < lens)).sum()),
                capped=int((keep == 128).sum()), dropped=int((keep <= 0).sum()), n_max=int(nmax.max()))


def without_q_filtered(sketch, all_matches, mid_occ, q_occ_frac):
    """The unfiltered matches of a read less those whose minimizer value the q-occurrence filter removes (seed.c:5-30: a value that occurs
    c times among the read's n minimizers, c > mid_occ and c > n * q_occ_frac).  sketch: mm.sketch of the read."""
    _, inv, c = np.unique(sketch[:, 0], return_inverse=True, return_counts=True)
    c = c[inv]
    gone = (c > mid_occ) & (c.astype(np.float32) > np.float32(len(sketch)) * np.float32(q_occ_frac)) if len(sketch) > mid_occ else np.zeros(len(c), bool)
    stay = ~np.isin(all_matches["seeds"][:, 1], (sketch[gone, 1] & np.uint64(0xffffffff)).astype(np.uint32))
    return dict(all_matches, seeds=all_matches["seeds"][stay])


def dropped_by_max_max_occ_alone(all_by_read, kept_by_read, mid_occ, max_max_occ, occ_dist):
    """Matches of a thinning set that the streak selection would have kept and `n > max_max_occ` removed: the n of the unfiltered matches
    above max_max_occ that are among their streak's `keep` smallest by (n, position).  kept_by_read: the set's own matches, to prove that
    they are gone."""
    found = 0
    for all_m, kept in zip(all_by_read, kept_by_read):
        n = all_m["seeds"][:, 0].astype(np.int64)
        if len(n) < 2:
            continue
        q = all_m["seeds"][:, 1]
        lens, keep, _ = streaks(all_m, all_m["qlen"], mid_occ, occ_dist)
        hi = np.concatenate([[False], n > mid_occ, [False]])
        start = np.flatnonzero(hi[1:] & ~hi[:-1])
        for i, ln, kp in zip(start, lens, keep):
            if kp <= 0:
                continue
            order = np.lexsort((np.arange(ln), n[i:i + ln]))[:kp]
            chosen = i + order[n[i + order] > max_max_occ]
            assert not np.isin(q[chosen], kept["seeds"][:, 1]).any()
            found += len(chosen)
    return found
