"""Batches larger than the grids of the kernels that give a read to a wave and let the wave stride on (DESIGN: "Batches beyond one pass of a capped grid").  With
W = 32 x compute units -- the waves of k_seed_compact, k_seed_pack, k_sort_x, k_gen_regs, k_heap_sort_wave, k_heap_emit and k_heap_pack -- a full batch holds
N = max(2 W, 16384) + 37 tiny reads: every wave takes a second read, 37 waves a third; k_seed_offsets goes round 17 times at 256 CUs, k_m_rep_len (16384 blocks) and
k_m_select (8192 blocks) take a second step.  The hard reads of a batch (one just over a size class, one with equal keys) lie at W - 1, W, 2 W - 1, 2 W and N - 1: the
last and first read of a wave's pass; an empty read lies at 0, W + 1 and N - 2 with a read whose hits are all dropped beside it.  The smaller batches of the
kernel-level tests (N = W: the grid exactly full, N = W + 1: one wave with a second read) are the full batch's first W and W + 1 reads.
Every batch is built once, from whole arrays.  Test infrastructure only: imported by tests/test_scale_cpu.py, tests/test_gpu_scale.py and tests/tools/gen_golden_scale.py."""
import json
import os

import numpy as np

import golden_io
import orc
import sr_cases as sc
import synth_cases as syn
import mm2gb_amd as mm
from test_gpu_formats import random_matches

GOLD = os.path.join(golden_io.GOLD, "scale")
CU_CPU = 256                          # the compute units the host-side tests size their batches by (an MI355X's)
REF_EXE = sc.REF_EXE
INF = 2**31 - 1
U64 = np.uint64


def sizes(cu):
    """(W, N) for a device of `cu` compute units."""
    w = 32 * cu
    return w, max(2 * w, 16384) + 37


def special(w, n):
    """(hard, blank, dropped): the indices below n of the hard reads, of the empty reads, and of the reads whose hits are all dropped (an empty read's neighbour)."""
    hard = list(dict.fromkeys(i for i in (w - 1, w, 2 * w - 1, 2 * w, n - 1) if 0 <= i < n))
    blank = [i for i in (0, w + 1, n - 2) if 0 <= i < n and i not in hard]
    dropped = []
    for i in blank:
        j = i + 1 if i + 1 < n and i + 1 not in hard + blank else i - 1
        assert 0 <= j < n and j not in hard + blank + dropped
        dropped.append(j)
    return hard, blank, dropped


def where(r, w):
    """A read index as the failure messages give it: relative to W."""
    return f"read {r} (= {r // w} W + {r % w}; W = {w})"


def first_difference(got_off, got, want_off, want, w, what):
    """Two batches of per-read rows laid end to end with their offsets: None where they are equal, otherwise a message that names the first differing read relative to W."""
    if np.array_equal(got_off, want_off) and np.array_equal(got[:int(got_off[-1])], want):
        return None
    for r in range(len(want_off) - 1):
        a, b = got[int(got_off[r]):int(got_off[r + 1])], want[int(want_off[r]):int(want_off[r + 1])]
        if got_off[r] != want_off[r] or a.shape != b.shape or not np.array_equal(a, b):
            return f"{what}: {where(r, w)}: offset {int(got_off[r])} for {int(want_off[r])}, {len(a)} rows for {len(b)}"
    return f"{what}: the totals differ ({int(got_off[-1])} for {int(want_off[-1])})"


def offsets(counts):
    off = np.zeros(len(counts) + 1, np.int64)
    np.cumsum(counts, out=off[1:])
    return off


def lay(rows, shape=(0, 2), dt=np.uint64):
    """Per-read arrays end to end: (offsets, rows)."""
    return offsets([len(x) for x in rows]), (np.concatenate(rows) if len(rows) else np.zeros(shape, dt))


# ---------------------------------------------------------------- 1. Engine.collect_seeds
N_REF = 7
SEED_POOL = 4_096
SEED_QLENS = (3_000, 4_000, 5_000, 9_000)                               # the reads' lengths: a length taken from another read shows in every reverse-strand anchor
SEED_QLEN = min(SEED_QLENS)                                             # (the seeds' positions lie below it: they fit every read)
SEED_REF_LEN = [3_000, 5_000, 3_000, 4_000, 9_000, 3_000, 6_000]        # every read length is some sequence's: MM_F_NO_DIAG's test can pass
HARD_QLENS = (3_000, 5_000, 4_000, 9_000, 3_000)                        # the hard reads' lengths in turn
SEED_REF_OF_LEN = {3_000: 0, 4_000: 3, 5_000: 1, 9_000: 4}              # a sequence of each read length
SEED_REF_RANK = [4, 1, 0, 5, 2, 2, 3]                                   # (two sequences of one name)
SEED_FLAGS = {"none": 0, "rev_only": orc.MM_F_REV_ONLY, "no_diag_no_dual": orc.MM_F_NO_DIAG | orc.MM_F_NO_DUAL}


def _cut_hits(seeds, hits, n_hits):
    """The leading seeds of random_matches' output that hold exactly n_hits hits (the last one's list shortened)."""
    cum = np.cumsum(seeds[:, 0].astype(np.int64))
    k = int(np.searchsorted(cum, n_hits)) + 1
    assert k <= len(seeds)
    seeds = seeds[:k].copy()
    seeds[-1, 0] -= np.uint32(cum[k - 1] - n_hits)
    return seeds, hits[:n_hits].copy()


def _same_strand(seeds, hits):
    """Every hit on its seed's strand: MM_F_REV_ONLY drops them all."""
    own = np.repeat(seeds[:, 1] & np.uint32(1), seeds[:, 0].astype(np.int64)).astype(U64)
    return (hits & ~U64(1)) | own


def seed_batch(w, n, seed=101):
    """dict(reads, ref_len, ref_rank, lost): n reads of 0-6 seeds with 0-5 hits as test_gpu_formats.random_matches makes them (one call makes a pool of SEED_POOL
    seeds, which the reads' seeds are drawn from with their hits).  A read's length is one of SEED_QLENS at random, so that neighbours in a wave's passes differ in it (it
    enters every reverse-strand query position and MM_F_NO_DIAG's test); half the reads carry the name of a sequence of their own length.  Three tenths of the reads
    (lost[r]) have every hit on its seed's strand and a name above every reference's: MM_F_REV_ONLY and MM_F_NO_DUAL drop all their hits.  Hard reads: 65 hits, and 40
    hits at one position of a sequence of the read's length (equal x on either strand); their lengths are 3000, 5000, 4000, 9000, 3000 in turn: those at W - 1 and W,
    and a hard read and the read W before it, differ."""
    rng = np.random.default_rng(seed)
    hard, blank, dropped = special(w, n)
    n_seeds = rng.integers(0, 7, n)
    n_seeds[blank] = 0
    n_seeds[dropped] = 4
    pool_seeds, pool_hits = random_matches(rng, SEED_POOL, SEED_QLEN, N_REF, 5, SEED_REF_LEN)
    pool_off = offsets(pool_seeds[:, 0].astype(np.int64))
    pick = rng.integers(0, SEED_POOL, int(n_seeds.sum()))
    seeds = pool_seeds[pick]
    seed_off = offsets(n_seeds)
    hit_off = offsets(seeds[:, 0].astype(np.int64))
    per = seeds[:, 0].astype(np.int64)
    hits = pool_hits[np.repeat(pool_off[pick], per) + np.arange(int(hit_off[-1])) - np.repeat(hit_off[:-1], per)]
    lost = rng.random(n) < 0.3                           # (nearly a quarter of them have no hit to lose)
    lost[dropped] = True
    lost[blank] = lost[hard] = False
    hits = np.where(np.repeat(np.repeat(lost, n_seeds), seeds[:, 0].astype(np.int64)), _same_strand(seeds, hits), hits)
    qlen = np.asarray(SEED_QLENS)[rng.integers(0, len(SEED_QLENS), n)]
    qlen[blank] = SEED_QLEN
    for k, r in enumerate(hard):                        # the read W before a hard read is of another length than it
        if r >= w and r - w not in hard:
            qlen[r - w] = SEED_QLENS[(SEED_QLENS.index(HARD_QLENS[k % 5]) + 1) % len(SEED_QLENS)]
    own_name = np.asarray([SEED_REF_RANK[SEED_REF_OF_LEN[int(v)]] for v in SEED_QLENS])[np.searchsorted(SEED_QLENS, qlen)]
    q_rank = np.where(lost, N_REF, np.where(rng.random(n) < 0.5, own_name, rng.integers(0, N_REF, n)))
    s0, s1 = seed_off[:-1], seed_off[1:]
    reads = [dict(seeds=seeds[s0[r]:s1[r]], hits=hits[hit_off[s0[r]]:hit_off[s1[r]]], qlen=int(qlen[r]), q_rank=int(q_rank[r])) for r in range(n)]
    for k, r in enumerate(hard):
        sd, ht = random_matches(rng, 60, SEED_QLEN, N_REF, 5, SEED_REF_LEN)
        length = HARD_QLENS[k % 5]
        rid = SEED_REF_OF_LEN[length]
        if k % 2 == 0:
            sd, ht = _cut_hits(sd, ht, 65)
        else:
            sd, ht = _cut_hits(sd, ht, 40)
            ht = (ht & U64(1)) | U64(rid << 32 | 1_234 << 1)
        reads[r] = dict(seeds=sd, hits=ht, qlen=length, q_rank=int(SEED_REF_RANK[rid]))
    for r in dropped:                                   # (seven hits for certain: the body's reads may have none)
        sd, ht = _cut_hits(*random_matches(rng, 60, SEED_QLEN, N_REF, 5, SEED_REF_LEN), 7)
        reads[r] = dict(seeds=sd, hits=_same_strand(sd, ht), qlen=int(qlen[r]), q_rank=N_REF)
    return dict(reads=reads, ref_len=SEED_REF_LEN, ref_rank=SEED_REF_RANK, lost=lost)


def seed_want(batch, flag):
    """Every read's anchors by the oracle's collect_seed_hits."""
    out = []
    for rd in batch["reads"]:
        out.append(orc.collect_seeds(flag, rd["qlen"], rd["seeds"], offsets(rd["seeds"][:, 0].astype(np.int64)), rd["hits"], q_rank=rd["q_rank"], ref_len=batch["ref_len"],
                                     ref_rank=batch["ref_rank"]))
    return out


def collect_seeds_raw(engine, flag, reads, ref_len=None, ref_rank=None):
    """mm2gb_collect_seeds_gpu as Engine.collect_seeds calls it, with the offsets it returned: (anchor_off, anchors end to end)."""
    R, seed_off, seeds, hit_off, hits, qlen, q_rank, rl, rr, n_ref, ptr = mm._seed_arrays(reads, ref_len, ref_rank)
    a_off = np.zeros(R + 1, np.int64)
    out = np.zeros((max(len(hits), 1), 2), np.uint64)
    mm._check(mm.lib().mm2gb_collect_seeds_gpu(engine._h, int(flag), R, seed_off.ctypes.data, seeds.ctypes.data, hit_off.ctypes.data, hits.ctypes.data, qlen.ctypes.data, ptr(q_rank), n_ref,
                                               ptr(rl), ptr(rr), a_off.ctypes.data, out.ctypes.data))
    return a_off, out


# ---------------------------------------------------------------- 2. Engine.collect_seeds_heap
HEAP_FLAGS = {"none": 0, "rev_only": orc.MM_F_REV_ONLY}
N_LONG, N_LONG_TIED = 200, 3
TIED_SHARE = 0.04                     # of the small reads: with the three long ones between 1 % and 10 % of the batch


def long_read(rng, n, n_seeds, tie=False):
    """sr_cases.crafted_reads' `many` from whole arrays: n hits at ascending distinct positions dealt to n_seeds seeds; tie: three cr that two seeds share."""
    pos = 100 + np.cumsum(rng.integers(1, 1_500, n))
    owner = rng.integers(0, n_seeds, n)
    cr = (pos.astype(U64) << U64(1)) | (pos & 1).astype(U64)
    lists = [cr[owner == s] for s in range(n_seeds)]
    if tie:
        lists[1] = np.union1d(lists[1], lists[0][-3:])
    seeds = [sc.seed(len(l), 25 + 7 * s, s & 1) for s, l in enumerate(lists)]
    return dict(seeds=np.asarray(seeds, np.uint32).reshape(-1, 4), hits=np.concatenate(lists).astype(U64), qlen=25 + 7 * n_seeds + 10)


def heap_batch(w, n, seed=202):
    """dict(reads, tied, long): n reads in sr_cases.read_of's form (rows of sr_cases.seed, hits of sr_cases.hit): 0-6 seeds with 0-5 hits, every seed's list
    ascending and distinct as an index's is; TIED_SHARE of them with one list on two seeds; N_LONG reads of 1025-1400 hits spread evenly (rocPRIM's segmented sort
    gets as many segments between ranges it must not touch), N_LONG_TIED of them tied; at the hard indices sr_cases.crafted_reads' wave_exact, wave_plus_1 and odd_65,
    none of them tied; the dropped reads have every hit on its seed's strand.  tied[r]: the read has two equal cr."""
    rng = np.random.default_rng(seed)
    hard, blank, dropped = special(w, n)
    n_seeds = rng.integers(0, 7, n)
    n_seeds[blank] = 0
    n_seeds[dropped] = 4
    seed_off = offsets(n_seeds)
    ns = int(seed_off[-1])
    n_hits = rng.integers(0, 6, ns)
    n_hits[rng.random(ns) < 0.2] = 0
    share = np.flatnonzero((rng.random(n) < TIED_SHARE) & (n_seeds >= 2))
    share = share[~np.isin(share, hard + blank + dropped)]
    first = seed_off[share]
    n_hits[first] = np.maximum(n_hits[first], 2)
    n_hits[first + 1] = n_hits[first]
    hit_off = offsets(n_hits)
    nh = int(hit_off[-1])
    owner = np.repeat(np.arange(ns), n_hits)
    # ascending and distinct inside a seed: sorted random positions with the place in the list below them
    val = rng.integers(100, 1 << 26, nh)
    val = val[np.lexsort((val, owner))]
    pos = val * 8 + (np.arange(nh) - hit_off[owner])
    strand = rng.integers(0, 2, nh)
    hits = (pos.astype(U64) << U64(1)) | strand.astype(U64)
    for s in first:
        hits[hit_off[s + 1]:hit_off[s + 2]] = hits[hit_off[s]:hit_off[s + 1]]
    span = rng.integers(15, 29, ns)
    qlen = rng.integers(80, 251, n)
    q_pos = rng.integers(span, np.repeat(qlen, n_seeds))
    seeds = np.zeros((ns, 4), np.uint32)
    seeds[:, 0], seeds[:, 1], seeds[:, 2], seeds[:, 3] = n_hits, q_pos << 1 | rng.integers(0, 2, ns), span, rng.integers(0, 2, ns) << 31
    lose = np.zeros(n, bool)
    lose[dropped] = True
    hits = np.where(np.repeat(np.repeat(lose, n_seeds), n_hits), _same_strand(seeds, hits), hits)
    s0, s1 = seed_off[:-1], seed_off[1:]
    reads = [dict(seeds=seeds[s0[r]:s1[r]], hits=hits[hit_off[s0[r]]:hit_off[s1[r]]], qlen=int(qlen[r])) for r in range(n)]
    crafted = sc.crafted_reads(rng)
    for k, r in enumerate(hard):
        reads[r] = crafted[("wave_exact", "wave_plus_1", "odd_65", "odd_65", "wave_plus_1")[k % 5]]
    taken = set(hard + blank + dropped)
    at = [r for r in (np.arange(N_LONG) * n // N_LONG + 11).tolist() if r < n and r not in taken]
    for k, r in enumerate(at):
        reads[r] = long_read(rng, int(rng.integers(sc.WAVE_HITS + 1, 1_401)), int(rng.integers(9, 41)), tie=k in (1, len(at) // 2, len(at) - 2)[:N_LONG_TIED])
    tied = np.asarray([sc.has_equal_cr(rd) for rd in reads])
    return dict(reads=reads, tied=tied, long=at)


# ---------------------------------------------------------------- 3. Engine.sort_seeds and Engine.gen_regs
def sort_batch(w, n, seed=303):
    """(anchors, offsets): reads of 0-40 unsorted anchors on a dozen reference positions (equal x frequent); at the hard indices 65, 5000 (about 16 per x), 40 with
    one x, 64 and 65 anchors; empty reads at the blank ones."""
    rng = np.random.default_rng(seed)
    hard, blank, dropped = special(w, n)
    cnt = rng.integers(0, 41, n)
    width = np.full(n, 12)
    cnt[blank] = 0
    for k, r in enumerate(hard):
        cnt[r], width[r] = ((65, 12), (5_000, 300), (40, 1), (64, 12), (65, 12))[k % 5]
    tot = int(cnt.sum())
    wide = np.repeat(width, cnt)
    rev = np.where(wide == 1, 0, rng.integers(0, 2, tot))
    a = syn.pack(np.full(tot, 2), rev, 7_000 + rng.integers(0, wide), rng.integers(0, 50_000, tot))
    return np.ascontiguousarray(a), offsets(cnt)


def sort_want(a, off):
    return np.concatenate([orc.radix_sort_x(a[off[r]:off[r + 1]]) for r in range(len(off) - 1)] + [np.zeros((0, 2), np.uint64)])


def chain_batch(w, n, seed=404):
    """dict(chains=[(u, a)], u_off, a_off, u, a, qlen, hashes): chains handed to mm_gen_regs as they are, no chaining before.  0-5 chains a read, 65, 64, 5 of one score,
    64 and 65 at the hard indices, none at the blank ones; 1-6 anchors a chain with spans of 5-28 mixed inside it and steps of 1-60 on either axis (steps above
    and below the span: both branches of the matching length), a quarter of the chains beginning in the reference's first ten bases (the start clamped to 0), both
    strands, scores of 40-42 (the hash of the first anchor orders the equal ones)."""
    rng = np.random.default_rng(seed)
    hard, blank, dropped = special(w, n)
    n_ch = rng.integers(0, 6, n)
    n_ch[blank] = 0
    one_score = []
    for k, r in enumerate(hard):
        n_ch[r] = (65, 64, 5, 64, 65)[k % 5]
        if k % 5 == 2:
            one_score.append(r)
    u_off = offsets(n_ch)
    nc = int(u_off[-1])
    cnt = rng.integers(1, 7, nc)
    c_off = offsets(cnt)
    na = int(c_off[-1])
    chain = np.repeat(np.arange(nc), cnt)
    begins = np.arange(na) == c_off[chain]
    span = rng.integers(5, 29, na)
    near = rng.random(nc) < 0.25
    x0 = np.where(near, rng.integers(0, 10, nc), rng.integers(100, 50_000, nc))
    y0 = span[c_off[:-1]] - 1 + rng.integers(0, 200, nc)
    dx, dy = np.where(begins, 0, rng.integers(1, 61, na)), np.where(begins, 0, rng.integers(1, 61, na))
    cx, cy = np.cumsum(dx), np.cumsum(dy)
    x = x0[chain] + cx - cx[c_off[chain]]
    y = y0[chain] + cy - cy[c_off[chain]]
    a = syn.pack(np.repeat(rng.integers(0, 4, nc), cnt), np.repeat(rng.integers(0, 2, nc), cnt), x, y, qspan=span)
    score = rng.integers(40, 43, nc)
    read_of_chain = np.repeat(np.arange(n), n_ch)
    score[np.isin(read_of_chain, one_score)] = 41
    u = (score.astype(U64) << U64(32)) | cnt.astype(U64)
    a_off = c_off[u_off]
    qlen = np.full(n, 100, np.int64)
    np.maximum.at(qlen, read_of_chain[chain], y + 1)
    qlen = (qlen + rng.integers(0, 100, n)).astype(np.int32)
    hashes = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    chains = [(u[u_off[r]:u_off[r + 1]], a[a_off[r]:a_off[r + 1]]) for r in range(n)]
    return dict(chains=chains, u_off=u_off, a_off=a_off, u=u, a=np.ascontiguousarray(a), qlen=qlen, hashes=hashes, span=span, dx=dx, dy=dy, near=near)


def regs_want(b, is_qstrand, n=None):
    n = len(b["chains"]) if n is None else n
    return np.concatenate([orc.gen_regs(b["chains"][r][0], b["chains"][r][1], int(b["qlen"][r]), int(b["hashes"][r]), is_qstrand) for r in range(n)] + [np.zeros(0, orc.REG_DTYPE)])


# ---------------------------------------------------------------- 4. Engine.collect_matches
MATCH_OPTS = {"q0": dict(mid_occ=2, max_max_occ=8, occ_dist=50, q_occ_frac=0.0), "q1e-4": dict(mid_occ=2, max_max_occ=8, occ_dist=50, q_occ_frac=1e-4)}
REP_LEN_GRID = 16_384                 # k_m_rep_len's blocks, one read each
SELECT_GRID = 8_192                   # k_m_select's blocks, one streak each


def match_reads(w, n, seed=505):
    """n reads of 80-150 bases cut from the short-read fixture's genome, two thirds of them from inside its tandem array (each carries one streak of matches above
    mid_occ = 2 that is thinned); 150 bases of the array at the hard indices; an empty read, an all-N read and a read shorter than k at the blank ones."""
    rng = np.random.default_rng(seed)
    hard, blank, dropped = special(w, n)
    g = np.frombuffer(sc.gold()["genome"].encode(), np.uint8)
    t0, copies, unit = sc.TANDEM
    length = rng.integers(80, 151, n)
    inside = rng.random(n) < 2 / 3
    length[hard], inside[hard] = 150, True
    st = np.where(inside, t0 + rng.integers(0, copies * unit - length + 1), rng.integers(0, len(g) - length))
    reads = [g[s:s + m].tobytes() for s, m in zip(st.tolist(), length.tolist())]
    odd = [b"", b"N" * 120, b"ACGTACGTACGTACG"]
    for k, r in enumerate(blank):
        reads[r] = odd[k % 3]
    for k, r in enumerate(dropped):
        reads[r] = odd[(k + 1) % 3]
    return reads


def host_matches(reads, **kw):
    ix = sc.index()
    return [ix.matches(s, **kw) for s in reads]


def thinned_streaks(unfiltered, mid_occ, occ_dist):
    """How many streaks k_m_streaks lists for k_m_select (seed_kernels.hip: streak_of), counted from the host's unfiltered matches (mid_occ = 2^30, q_occ_frac = 0):
    in a read of at least two matches a maximal run of matches with more than mid_occ occurrences, of which keep = min(int((pe - ps) / occ_dist + .499), 128) survive
    (ps: the position of the match before the run or 0, pe: of the match after it or the read's length); it counts where 0 < keep < its length."""
    cnt = np.asarray([len(m["seeds"]) for m in unfiltered])
    off = offsets(cnt)
    tot = int(off[-1])
    if tot == 0:
        return 0
    occ = np.concatenate([m["seeds"][:, 0] for m in unfiltered]).astype(np.int64)
    q = np.concatenate([m["seeds"][:, 1] for m in unfiltered]).astype(np.int64) >> 1
    read = np.repeat(np.arange(len(cnt)), cnt)
    qlen = np.asarray([m["qlen"] for m in unfiltered])
    high = occ > mid_occ
    first_of_read, last_of_read = np.arange(tot) == off[read], np.arange(tot) == off[read + 1] - 1
    begins = high & (first_of_read | ~np.concatenate([[False], high[:-1]]))
    ends = high & (last_of_read | ~np.concatenate([high[1:], [False]]))
    b, e = np.flatnonzero(begins), np.flatnonzero(ends) + 1
    assert len(b) == len(e)
    ps = np.where(first_of_read[b], 0, q[np.maximum(b - 1, 0)])
    pe = np.where(last_of_read[e - 1], qlen[read[b]], q[np.minimum(e, tot - 1)])
    keep = np.minimum(((pe - ps) / occ_dist + .499).astype(np.int64), 128)
    return int(((cnt[read[b]] >= 2) & (keep > 0) & (keep < e - b)).sum())


# ---------------------------------------------------------------- 5., 6. the mappers on the short-read fixture's reads, c times over
def copies(n):
    return -(-n // 209)


def paf_difference(got, one, c, w, what):
    """None where `got` is c copies of the text `one`; otherwise the first differing line and its read's index in the batch (from the expected line's place: copy x 209
    + the read's place in the set) modulo 209 and modulo W."""
    if got == one * c:
        return None
    names = [nm for nm, _ in sc.reads()]
    g, x = got.splitlines(), one.splitlines() * c
    at = next((i for i, (a, b) in enumerate(zip(g, x)) if a != b), min(len(g), len(x)))
    line = x[at] if at < len(x) else g[at]
    r = min(at // len(one.splitlines()), c - 1) * 209 + names.index(line.split("\t")[0])
    return (f"{what}: line {at} of {len(g)} (expected {len(x)}), read {r} (mod 209: {r % 209}, mod W: {r % w}; W = {w})\n got  {g[at] if at < len(g) else '(none)'}\n"
            f" want {x[at] if at < len(x) else '(none)'}")


def map_sr(engine, run, reads, align_on_device=0, text_on_device=0, **fields):
    """sr_cases.map_run on `reads` instead of the fixture's: (PAF text, stats)."""
    _, opt_kw, sr_kw = sc.RUNS[run]
    opt = mm.map_opt_sr(host_threads=4, **dict(opt_kw, **fields))
    if sr_kw.get("align"):
        sr_kw = dict(sr_kw, refs=[sc.gold()["genome"].encode()], align_on_device=align_on_device, text_on_device=text_on_device)
    return mm.map_reads(engine, sc.index(), ["ref"], reads, opt=opt, k=mm.preset_sr()["k"], align=mm.map_sr(**sr_kw))


def map_long(engine, run, reads, **fields):
    """A run of LONG_RUNS through this project's mapper on `reads`: (PAF text, stats)."""
    _, kw, own = LONG_RUNS[run]
    return mm.map_reads(engine, long_index(run), ["ref"], reads, opt=mm.map_opt(**{**own, "max_chain_skip": INF, "host_threads": 4, **fields}), k=kw["k"])


LONG_RUNS = {         # run: (the reference program's arguments, the index parameters, this project's option fields)
    "ont": ([], dict(k=15, w=10, hpc=False), {}),
    "pb": (["-x", "map-pb"], dict(k=19, w=10, hpc=True), {}),
    "ont.nolj": (["--no-long-join"], dict(k=15, w=10, hpc=False), dict(flag=mm.F_NO_LJOIN)),
    "pb.nolj": (["-x", "map-pb", "--no-long-join"], dict(k=19, w=10, hpc=True), dict(flag=mm.F_NO_LJOIN)),
}
SKIP_ARG = f"--max-chain-skip={INF}"
_long = None
_long_index = {}


def long_paf(run):
    """The committed texts (tests/golden/scale/scale.npz: one JSON document, compressed): {run: what minimap2 -t 1 <arguments> --max-chain-skip=2147483647 printed for the
    short-read fixture's genome and its 209 reads}."""
    global _long
    if _long is None:
        _long = json.loads(np.load(os.path.join(GOLD, "scale.npz"))["doc"].tobytes().decode("utf-8"))
    return _long[run]


def long_index(run):
    kw = LONG_RUNS[run][1]
    key = (kw["k"], kw["hpc"])
    if key not in _long_index:
        _long_index[key] = mm.SeedIndex([sc.gold()["genome"].encode()], threads=4, **kw)
    return _long_index[key]


def long_doc_bytes(doc):
    """The fixture's bytes for a document: np.savez_compressed's layout with the member's time stamp fixed, so that the same document gives the same file."""
    import io
    import zipfile
    member, out = io.BytesIO(), io.BytesIO()
    np.lib.format.write_array(member, np.frombuffer(json.dumps(doc, sort_keys=True).encode("utf-8"), dtype=np.uint8), allow_pickle=False)
    with zipfile.ZipFile(out, "w", zipfile.ZIP_DEFLATED) as z:
        z.writestr(zipfile.ZipInfo("doc.npy", date_time=(1980, 1, 1, 0, 0, 0)), member.getvalue(), zipfile.ZIP_DEFLATED)
    return out.getvalue()


def record_long(times=1):
    """{run: text} from the reference program on `times` copies of the 209 reads."""
    genome, reads = sc.gold()["genome"].encode(), sc.reads() * times
    return {run: sc.record_paf(genome, reads, args + [SKIP_ARG]) for run, (args, _, _) in LONG_RUNS.items()}
