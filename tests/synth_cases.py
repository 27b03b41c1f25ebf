"""Seeded synthetic anchor sets for parity tests (numpy; small/medium sizes).

Anchor packing follows lchain.c:140-143 / mmpriv.h:18-24:
    x = rev<<63 | rid<<32 | ref_pos        y = seg_id<<48 | flags<<40 | q_span<<32 | query_pos
Every generator returns an (n, 2) uint64 array sorted by x, which is what map.c:329 hands to chaining.
"""
import numpy as np


def pack(rid, rev, rpos, qpos, qspan=15, sid=0, flags=0):
    rid = np.asarray(rid, dtype=np.uint64)
    rev = np.asarray(rev, dtype=np.uint64)
    rpos = np.asarray(rpos, dtype=np.uint64)
    qpos = np.asarray(qpos, dtype=np.uint64)
    qspan = np.broadcast_to(np.asarray(qspan, dtype=np.uint64), rpos.shape)
    sid = np.broadcast_to(np.asarray(sid, dtype=np.uint64), rpos.shape)
    flags = np.broadcast_to(np.asarray(flags, dtype=np.uint64), rpos.shape)
    x = (rev << np.uint64(63)) | (rid << np.uint64(32)) | rpos
    y = (sid << np.uint64(48)) | (flags << np.uint64(40)) | (qspan << np.uint64(32)) | qpos
    return np.stack([x, y], axis=1)


def sort_by_x(a):
    return a[np.argsort(a[:, 0], kind="stable")]


def noise(n, seed, n_rid=24, span=100_000_000, qlen=50_000):
    rng = np.random.default_rng(seed)
    return sort_by_x(pack(rng.integers(0, n_rid, n), rng.integers(0, 2, n), rng.integers(0, span, n),
                          rng.integers(15, qlen, n)))


def colinear(n, seed, rid=3, rev=0, r0=1_000_000, q0=100, max_gap=33, indel_p=0.125, qspan=15):
    """A true chain: gaps U[1,max_gap], occasional small indels on either axis."""
    rng = np.random.default_rng(seed)
    step = rng.integers(1, max_gap + 1, n)
    dx = step + np.where(rng.random(n) < indel_p, rng.integers(0, 20, n), 0)
    dy = step + np.where(rng.random(n) < indel_p, rng.integers(0, 20, n), 0)
    return pack(np.full(n, rid), np.full(n, rev), r0 + np.cumsum(dx), q0 + np.cumsum(dy), qspan=qspan)


def repeat_block(n, seed, rid=3, rev=0, r0=2_000_000, q0=5_000, xwin=4000, ywin=6000):
    """Dense block: many anchors inside one max_dist_x window (saturates max_iter when n > max_iter)."""
    rng = np.random.default_rng(seed)
    return pack(np.full(n, rid), np.full(n, rev), r0 + rng.integers(0, xwin, n), q0 + rng.integers(0, ywin, n))


def read_like(length, seed, with_repeat=True):
    """One ONT-like read: chain + 3x noise + optional repeat block (small-scale SURVEY 8d recipe)."""
    rng = np.random.default_rng(seed)
    n_true = max(4, int(0.06 * length))
    parts = [colinear(n_true, seed + 1, q0=50), noise(3 * n_true, seed + 2, qlen=max(length, 32))]
    if with_repeat:
        parts.append(repeat_block(int(rng.integers(200, 1500)), seed + 3, r0=1_000_000 + int(rng.integers(0, 17 * n_true)),
                                  q0=int(rng.integers(15, max(16, length - 6000)))))
    return sort_by_x(np.concatenate(parts))


def rescue_case(n_noise=9000, seed=7, n_chain=60):
    """a chain, then > max_iter noise anchors packed inside max_dist_x, then the chain goes on.
    With max_iter < n_noise the window of the first post-noise chain anchor no longer reaches the chain's
    last anchor, and only the max_ii rescue (lchain.c:190-201) links across."""
    rng = np.random.default_rng(seed)
    first = colinear(n_chain, seed, r0=1_000_000, q0=1000, max_gap=20, indel_p=0.0)
    xe = int(first[-1, 0] & np.uint64(0xffffffff))
    ye = int(first[-1, 1] & np.uint64(0xffffffff))
    # noise sits just after the chain end in x but far away in y, so it scores low and never chains with it
    nx = xe + 1 + np.sort(rng.integers(0, 2500, n_noise))
    ny = rng.integers(20_000, 60_000, n_noise)
    mid = pack(np.full(n_noise, 3), np.zeros(n_noise, np.int64), nx, ny)
    second = colinear(n_chain, seed + 1, r0=xe + 2600, q0=ye + 2600, max_gap=20, indel_p=0.0)
    return sort_by_x(np.concatenate([first, mid, second]))


def grid_ties(nx=40, ny=12, step=20):
    """Anchors on a regular lattice: lots of exactly equal candidate scores (tie-break coverage)."""
    gx, gy = np.meshgrid(np.arange(nx) * step + 5000, np.arange(ny) * step + 100, indexing="ij")
    return sort_by_x(pack(np.full(gx.size, 1), np.zeros(gx.size, np.int64), gx.ravel(), gy.ravel()))


def two_segments(n, seed):
    """Paired-end-like: seg_id 0/1 mixed on the same reference region (n_seg = 2 branches of comput_sc)."""
    rng = np.random.default_rng(seed)
    a = colinear(n, seed, r0=50_000, q0=10, max_gap=9)
    sid = rng.integers(0, 2, n).astype(np.uint64)
    a[:, 1] |= sid << np.uint64(48)
    # duplicate a few reference positions across segments to hit the dr == 0 bonus branch (lchain.c:132)
    dup = a[:: max(1, n // 10)].copy()
    dup[:, 1] ^= np.uint64(1) << np.uint64(48)
    dup[:, 1] += np.uint64(3)
    return sort_by_x(np.concatenate([a, dup]))


def variable_span(n, seed):
    """HPC-like seeds: q_span varies per anchor."""
    rng = np.random.default_rng(seed)
    a = colinear(n, seed, max_gap=25)
    span = rng.integers(9, 40, n).astype(np.uint64)
    a[:, 1] = (a[:, 1] & ~(np.uint64(0xff) << np.uint64(32))) | (span << np.uint64(32))
    return sort_by_x(np.concatenate([a, noise(n // 2, seed + 5, n_rid=4, span=200_000, qlen=30_000)]))


def multi_read_batch(n_reads, seed, min_len=2_000, max_len=30_000):
    """Concatenated reads + offsets (the micro-batch layout handed to the GPU path)."""
    rng = np.random.default_rng(seed)
    reads = [read_like(int(rng.integers(min_len, max_len)), seed * 1000 + r, with_repeat=(r % 3 == 0)) for r in range(n_reads)]
    off = np.zeros(n_reads + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(r) for r in reads])
    return np.concatenate(reads), off


def fuzz_case(rng):
    """One random batch and one random set of chaining parameters for the seeded fuzz test and tests/fuzz_soak.py:
    mixtures of chains, noise, repeat blocks, duplicated positions, empty reads, reads repeated or overlapping an earlier
    read of the batch; window limits around the tile (64) and ring sizes.  Returns (anchors, read offsets, parameter dict)."""
    reads = []
    for _ in range(int(rng.integers(1, 7))):
        kind = int(rng.integers(0, 7))
        seed = int(rng.integers(1, 1 << 30))
        if kind == 0:
            reads.append(np.zeros((0, 2), np.uint64))
        elif kind == 1:
            reads.append(noise(int(rng.integers(1, 400)), seed, n_rid=int(rng.integers(1, 4)), span=int(rng.integers(2_000, 200_000)), qlen=20_000))
        elif kind == 2:
            reads.append(read_like(int(rng.integers(1_000, 25_000)), seed))
        elif kind == 3:
            reads.append(sort_by_x(np.concatenate([repeat_block(int(rng.integers(100, 3000)), seed, xwin=int(rng.integers(50, 5000)), ywin=int(rng.integers(50, 7000))),
                                                   colinear(int(rng.integers(10, 800)), seed + 1, max_gap=int(rng.integers(2, 60)))])))
        elif kind == 4:
            reads.append(variable_span(int(rng.integers(50, 900)), seed))
        elif kind == 5:
            reads.append(grid_ties(nx=int(rng.integers(3, 50)), ny=int(rng.integers(2, 14)), step=int(rng.integers(1, 40))))
        elif reads and len(reads[-1]):
            prev = reads[-1]                       # a read over the same region: a slice of the previous one
            lo = int(rng.integers(0, len(prev)))
            reads.append(prev[lo:lo + int(rng.integers(1, len(prev) - lo + 1))].copy())
        else:
            reads.append(colinear(int(rng.integers(1, 300)), seed))
    off = np.zeros(len(reads) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(r) for r in reads])
    a = np.concatenate(reads) if off[-1] else np.zeros((0, 2), np.uint64)
    kw = dict(max_iter=int(rng.choice([1, 7, 63, 64, 65, 200, 1000, 5000])), bw=int(rng.choice([0, 1, 50, 500, 3000])),
              max_dist_x=int(rng.choice([10, 500, 5000, 20000])), max_dist_y=int(rng.choice([10, 500, 5000, 20000])),
              pen_gap=np.float32(rng.choice([0.0, 0.12, 0.19, 1.5])), pen_skip=np.float32(rng.choice([0.0, 0.0, 0.01, 0.3])),
              min_cnt=int(rng.integers(1, 5)), min_sc=int(rng.choice([1, 20, 40, 100])))
    return a, off, kw


# ---------------------------------------------------------------- inputs for the per-pair score builds (cDNA, segments, bw beyond the table)

SEG_MASK = np.uint64(0xff) << np.uint64(48)


def spliced(n_exons, seed, exon=(4, 60), intron=(70, 150_000), qins_p=0.2, noise_n=0, rid=3, rev=0, r0=1_000_000, q0=100):
    """A transcript-like read: exons are colinear runs of exon[0]..exon[1] anchors with small indels; consecutive exons are joined
    either by an intron -- a jump in x only, log-uniform in `intron` (dr >> dq: the min(lin, log) branch of the cDNA penalty,
    lchain.c:136) -- or, with probability qins_p, by a jump of 30-1500 in y only (dq > dr: the lin + .5 log branch).  noise_n anchors
    are spread over the read's span on the same rid and strand, so that they compete inside the same windows."""
    rng = np.random.default_rng(seed)
    xs, ys = [], []
    x, y = r0, q0
    for e in range(n_exons):
        n = int(rng.integers(exon[0], exon[1] + 1))
        step = rng.integers(1, 34, n)
        dx = step + np.where(rng.random(n) < 0.125, rng.integers(0, 12, n), 0)
        dy = step + np.where(rng.random(n) < 0.125, rng.integers(0, 12, n), 0)
        ex, ey = x + np.cumsum(dx), y + np.cumsum(dy)
        xs.append(ex); ys.append(ey)
        x, y = int(ex[-1]), int(ey[-1])
        if rng.random() < qins_p:
            y += int(rng.integers(30, 1501))
        else:
            x += int(np.exp(rng.uniform(np.log(intron[0]), np.log(intron[1]))))
    xs, ys = np.concatenate(xs), np.concatenate(ys)
    if noise_n:
        xs = np.concatenate([xs, rng.integers(r0, x + 1, noise_n)])
        ys = np.concatenate([ys, rng.integers(q0, y + 1, noise_n)])
    return sort_by_x(pack(np.full(len(xs), rid), np.full(len(xs), rev), xs, ys))


def qins_chain(n_blocks, seed, ins=(60, 100), rid=3, r0=1_000_000, q0=100):
    """Blocks on one diagonal each, separated by query-side insertions of ins[0]..ins[1] bases (dq > dr, dd = the insertion).  Long
    blocks (15-40 anchors) build a score up, runs of short ones (1-3 anchors) between them lose more at each insertion than they gain:
    with a steep pen_gap and bw >= ins[1] the DP still links through (f stays above a fresh start), but the chain's score falls by more
    than bw on the way -- the drop at which mg_chain_backtrack cuts a chain (lchain.c:36-47) unless is_cdna lifts max_drop to INT32_MAX."""
    rng = np.random.default_rng(seed)
    xs, ys = [], []
    x, y = r0, q0
    for b in range(n_blocks):
        n = int(rng.integers(15, 41)) if b % 5 == 0 else int(rng.integers(1, 4))
        step = rng.integers(15, 26, n)
        bx, by = x + np.cumsum(step), y + np.cumsum(step)
        xs.append(bx); ys.append(by)
        x, y = int(bx[-1]), int(by[-1]) + int(rng.integers(ins[0], ins[1] + 1))
    xs, ys = np.concatenate(xs), np.concatenate(ys)
    return pack(np.full(len(xs), rid), np.zeros(len(xs), np.int64), xs, ys)


def jump_chain(jumps, seed, n=400, rid=3, r0=1_000_000, q0=100):
    """len(jumps) + 1 blocks of n anchors, each exactly on one diagonal, joined by jumps of exactly jumps[k] bases, alternately on x
    and on y: every pair across one jump has dd == jumps[k], so the links the DP accepts say exactly where dd > bw starts."""
    rng = np.random.default_rng(seed)
    xs, ys = [], []
    x, y = r0, q0
    for b in range(len(jumps) + 1):
        step = rng.integers(1, 34, n)
        bx, by = x + np.cumsum(step), y + np.cumsum(step)
        xs.append(bx); ys.append(by)
        x, y = int(bx[-1]), int(by[-1])
        if b < len(jumps):
            if b % 2 == 0:
                x += int(jumps[b])
            else:
                y += int(jumps[b])
    xs, ys = np.concatenate(xs), np.concatenate(ys)
    return pack(np.full(len(xs), rid), np.zeros(len(xs), np.int64), xs, ys)


def with_segments(a, n_seg, seed, share=1.0):
    """Segment ids 0 .. n_seg-1 on a share of a read's anchors (the others keep id 0), and, like two_segments, a few reference positions
    duplicated into another segment (the dr == 0 bonus branch, lchain.c:132)."""
    rng = np.random.default_rng(seed)
    a = a.copy()
    n = len(a)
    if n == 0:
        return a
    a[:, 1] &= ~SEG_MASK
    sid = np.where(rng.random(n) < share, rng.integers(0, n_seg, n), 0).astype(np.uint64)
    a[:, 1] |= sid << np.uint64(48)
    dup = a[:: max(1, n // 10)].copy()
    dsid = (((dup[:, 1] & SEG_MASK) >> np.uint64(48)) + np.uint64(1)) % np.uint64(n_seg)
    dup[:, 1] = (dup[:, 1] & ~SEG_MASK) | (dsid << np.uint64(48))
    dup[:, 1] += np.uint64(3)
    return sort_by_x(np.concatenate([a, dup]))


def sparse_stretch(n, seed, gap=10_000, n_runs=4, rid=5):
    """A stretch of isolated anchors, `gap` apart on the reference and anywhere on the query, with a few runs of 2-7 anchors at 20 / 20:
    no window holds more than a few anchors, which is what the planner's sparse list is made of (two planning blocks and more of it
    hold a chunk of nothing else)."""
    rng = np.random.default_rng(seed)
    dx = np.full(n, gap, np.int64)
    y = rng.integers(1000, 50_000, n)
    for _ in range(n_runs):
        pos = int(rng.integers(1, n))
        for k in range(pos, min(n, pos + int(rng.integers(1, 7)))):
            dx[k] = 20
            y[k] = y[k - 1] + 20
    return pack(np.full(n, rid), np.zeros(n, np.int64), 1000 + np.cumsum(dx), y)


SPLICE_KW = dict(is_cdna=1, bw=200_000, max_dist_x=200_000, max_dist_y=2_000)
GENERAL_CLASSES = "abcdefg"


def fuzz_case_general(rng, it):
    """Like fuzz_case, for the score builds fuzz_case never reaches.  Reads are drawn from spliced / qins_chain / jump_chain, the older
    kinds, stretches of isolated anchors (sparse_stretch: chunks for the planner's sparse list) and slices of earlier reads; the parameter class is cycled by the iteration index (GENERAL_CLASSES[it % 7]), so every class
    occurs in any 7 consecutive iterations whatever the seed:
      a  the splice preset (is_cdna, bw = max_dist_x = 200 000, max_dist_y = 2 000)      b  is_cdna with bw in {0, 100, 500}
      c  n_seg in {2, 3} with segment ids                                                 d  n_seg > 1 and is_cdna
      e  n_seg = 1, table-sized bw, segment ids on some anchors (the device's fall-back)  f  bw in {5119, 9000, 200000} (no table)
      g  pen_skip > 0 (no table)
    Returns (anchors, read offsets, parameter dict)."""
    cls = GENERAL_CLASSES[it % len(GENERAL_CLASSES)]
    reads = []
    for _ in range(int(rng.integers(1, 7))):
        kind = int(rng.integers(0, 10))
        seed = int(rng.integers(1, 1 << 30))
        if kind == 0:
            reads.append(np.zeros((0, 2), np.uint64))
        elif kind == 8:
            reads.append(sparse_stretch(int(rng.integers(1100, 3000)), seed, rid=int(rng.integers(0, 4))))
        elif kind == 1:
            reads.append(spliced(int(rng.integers(1, 40)), seed, noise_n=int(rng.choice([0, 0, 300, 2000]))))
        elif kind == 2:
            reads.append(spliced(int(rng.integers(2, 25)), seed, exon=(1, 12), intron=(70, 300_000), qins_p=0.5, noise_n=int(rng.integers(0, 200))))
        elif kind == 3:
            reads.append(qins_chain(int(rng.integers(1, 60)), seed, ins=(int(rng.integers(1, 60)), int(rng.integers(60, 600)))))
        elif kind == 4:
            base = int(rng.choice([90, 490, 2990, 5110, 8990]))
            reads.append(jump_chain(base + rng.integers(0, 20, int(rng.integers(1, 6))), seed, n=int(rng.integers(5, 200))))
        elif kind == 5:
            reads.append(read_like(int(rng.integers(1_000, 15_000)), seed))
        elif kind == 6:
            reads.append(sort_by_x(np.concatenate([repeat_block(int(rng.integers(100, 3000)), seed, xwin=int(rng.choice([300, 5000, 150_000])), ywin=int(rng.choice([400, 1800, 7000]))),
                                                   spliced(int(rng.integers(1, 12)), seed + 1, r0=2_000_000, q0=5_000)])))
        elif kind == 7:
            reads.append(grid_ties(nx=int(rng.integers(3, 50)), ny=int(rng.integers(2, 14)), step=int(rng.integers(1, 40))))
        elif reads and len(reads[-1]):
            prev = reads[-1]                       # a read over the same region: a slice of the previous one
            lo = int(rng.integers(0, len(prev)))
            reads.append(prev[lo:lo + int(rng.integers(1, len(prev) - lo + 1))].copy())
        else:
            reads.append(variable_span(int(rng.integers(50, 900)), seed))
    n_seg = int(rng.choice([2, 3])) if cls in "cd" else 1
    if cls in "cde":
        ids = 2 if cls == "e" else n_seg
        tagged = [with_segments(r, ids, int(rng.integers(1, 1 << 30)), share=float(rng.choice([1.0, 0.5, 0.05]))) if (cls != "e" or rng.random() < 0.5) else r for r in reads]
        if cls == "e" and not any(np.any(t[:, 1] & SEG_MASK) for t in tagged):      # class e always carries an id somewhere: a lone anchor if need be
            tagged.append(pack([3], [0], [77], [99], sid=1))
        reads = tagged
    off = np.zeros(len(reads) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(r) for r in reads])
    a = np.concatenate(reads) if off[-1] else np.zeros((0, 2), np.uint64)
    dist = lambda: int(rng.choice([500, 5000, 20000, 200_000]))
    kw = dict(max_iter=int(rng.choice([1, 7, 63, 64, 65, 200, 1000, 5000])), bw=int(rng.choice([0, 1, 50, 500, 3000])), max_dist_x=dist(), max_dist_y=dist(),
              pen_gap=np.float32(rng.choice([0.0, 0.12, 0.19, 1.5])), pen_skip=np.float32(rng.choice([0.0, 0.0, 0.01, 0.3])),
              min_cnt=int(rng.integers(1, 5)), min_sc=int(rng.choice([1, 20, 40, 100])), is_cdna=0, n_seg=n_seg)
    if cls == "a":
        kw.update(SPLICE_KW)
    elif cls == "b":
        kw.update(is_cdna=1, bw=int(rng.choice([0, 100, 500])))
    elif cls == "d":
        kw.update(is_cdna=1)
        if rng.random() < 0.5:
            kw.update(SPLICE_KW)
    elif cls == "e":
        kw.update(pen_skip=np.float32(0.0), bw=int(rng.choice([50, 500, 3000, 5118])))
    elif cls == "f":
        kw.update(pen_skip=np.float32(0.0), bw=int(rng.choice([5119, 9000, 200_000])))
    elif cls == "g":
        kw.update(pen_skip=np.float32(rng.choice([0.01, 0.3])))
    return a, off, kw
