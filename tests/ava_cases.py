"""Cases for read-against-read overlap (minimap2 -x ava-ont, -x ava-pb, -X): the simulated read sets, the runs recorded from the reference program
(tests/golden/ava, made by tests/tools/gen_golden_ava.py), how this project's mapper is called on them, and crafted inputs for mm_est_err's walk.
Test infrastructure only: imported by tests/test_ava_cpu.py, tests/test_gpu_ava.py and tests/tools/gen_golden_ava.py."""
import json
import os

import numpy as np

import golden_io
import mm2gb_amd as mm
import sim_reads

GOLD = os.path.join(golden_io.GOLD, "ava")
INF = 2**31 - 1
SKIPS = {"s25": 25, "inf": INF}
# run: (query set, target set, the reference program's arguments, this project's options and index parameters)
RUNS = {
    "a.ava-ont": ("a", "a", ["-x", "ava-ont"]),
    "b.ava-pb": ("a", "a", ["-x", "ava-pb"]),                # the same reads, homopolymer-compressed minimizers
    "a.X": ("a", "a", ["-x", "map-ont", "-X"]),              # bw_long > bw: MM_F_NO_LJOIN alone keeps stage 4 out
    "c.ava-ont": ("cq", "ct", ["-x", "ava-ont"]),
    "c.ava-pb": ("cq", "ct", ["-x", "ava-pb"]),
    "c.X": ("cq", "ct", ["-x", "map-ont", "-X"]),
}
X_BITS = mm.F_NO_DIAG | mm.F_NO_DUAL | mm.F_NO_LJOIN | mm.F_ALL_CHAINS
OPT_FIELDS = ("flag", "min_chain_score", "pri_ratio", "occ_dist", "bw", "bw_long", "max_gap", "max_gap_ref", "min_cnt", "best_n", "mask_level", "min_mid_occ", "max_mid_occ",
              "mid_occ_frac", "q_occ_frac", "max_max_occ", "max_chain_iter", "rmq_inner_dist", "rmq_size_cap", "rmq_rescue_size", "rmq_rescue_ratio", "chain_gap_scale",
              "chain_skip_scale", "seed")
SIM_SEED = 5


def run_setup(run, **fields):
    """(map options, index keywords) of a recorded run."""
    kind = run.split(".")[1]
    if kind == "X":
        return mm.map_opt(flag=X_BITS, **fields), dict(k=15, w=10, hpc=False)
    return mm.map_opt_ava(kind, **fields), mm.preset_ava(kind)


# ---------------------------------------------------------------- the read sets
def genome(rng):
    """30 kb with a 1.5 kb tandem array (off-diagonal hits of a read on itself: MM_SEED_SELF) and a 2 kb inverted repeat (reverse-strand hits of a read on itself)."""
    g = sim_reads.BASES[rng.integers(0, 4, 30_000)].copy()
    unit = sim_reads.BASES[rng.integers(0, 4, 60)]
    g[6_000:7_500] = np.tile(unit, 25)
    g[22_000:24_000] = sim_reads.revcomp(g[14_000:16_000])
    return g


def read_at(rng, g, st, n, err, flip):
    s = sim_reads.mutate(rng, g[st:st + n], err)
    return sim_reads.revcomp(s) if flip else s


def sim_sets(seed=SIM_SEED):
    """{"a": [(name, bytes)], "cq": ..., "ct": ...}.  a: 40 reads of 2-8 kb, both strands, 5-10 % error, and one that is not from the genome.
    cq / ct: the traps of the name tests, queries against targets that share only some names (see tests/test_ava_cpu.py::test_name_traps_in_fixture)."""
    rng = np.random.default_rng(seed)
    g = genome(rng)
    a = []
    for r in range(40):
        n = int(rng.integers(2_000, 8_000))
        st = int(rng.integers(0, len(g) - n))
        a.append((f"read{r}", read_at(rng, g, st, n, float(rng.uniform(0.05, 0.10)), bool(rng.random() < 0.5)).tobytes()))
    a.append(("stray", sim_reads.BASES[rng.integers(0, 4, 3_000)].tobytes()))
    mk = lambda st, n, flip=False: read_at(rng, g, st, n, 0.06, flip).tobytes()
    dup = mk(1_000, 4_000)
    same_t, same_q = mk(9_000, 4_500), mk(10_000, 5_200)
    n_same = min(len(same_t), len(same_q))
    read10 = mk(3_000, 6_000)
    ct = [("read10", read10), ("r1", mk(12_000, 5_000)), ("r10", mk(16_500, 5_000, True)), ("dup", dup + mk(5_000, 700)), ("dup", dup), ("same", same_t[:n_same]),
          ("ré", mk(20_000, 5_000)), ("zz", mk(24_500, 5_000))]
    cq = [("read9", mk(2_000, 5_000)), ("read10", read10), ("r1", mk(13_000, 5_000)), ("r10", mk(17_000, 5_000)), ("dup", dup), ("same", same_q[:n_same]),
          ("ré", mk(21_000, 5_000, True)), ("aa", mk(25_000, 4_000))]
    return dict(a=a, cq=cq, ct=ct)


_gold = None


def gold():
    """The committed fixture (ava.npz: one JSON document, compressed): {"sets": {name: [[name, sequence]]}, "paf": {"<run>.<skip>": text}, "options": {preset: {...}}}."""
    global _gold
    if _gold is None:
        _gold = json.loads(np.load(os.path.join(GOLD, "ava.npz"))["doc"].tobytes().decode("utf-8"))
    return _gold


def read_set(name):
    return [(n, s.encode()) for n, s in gold()["sets"][name]]


def golden_paf(run, skip):
    return gold()["paf"][f"{run}.{skip}"]


_index = {}


def index_for(run):
    """The targets' SeedIndex of a run, kept for the process (host-built)."""
    _, tgt, _ = RUNS[run]
    _, kw = run_setup(run)
    key = (tgt, tuple(sorted(kw.items())))
    if key not in _index:
        _index[key] = mm.SeedIndex([s for _, s in read_set(tgt)], threads=4, **kw)
    return _index[key]


def map_run(engine, run, skip, stream=False, **fields):
    qry, tgt, _ = RUNS[run]
    opt, kw = run_setup(run, max_chain_skip=SKIPS[skip], host_threads=4, **fields)
    names = [n for n, _ in read_set(tgt)]
    if stream:
        return mm.map_reads_stream([engine], index_for(run), names, read_set(qry), opt=opt, k=kw["k"], chunk_bases=60_000)
    return mm.map_reads(engine, index_for(run), names, read_set(qry), opt=opt, k=kw["k"])


def own_options(name):
    o, ix = mm.map_opt_ava(name), mm.preset_ava(name)
    return json.loads(json.dumps(dict(map={k: getattr(o, k) for k in OPT_FIELDS}, index=ix)))


def ref_options(name):
    """mm_set_opt(NULL) + mm_set_opt(name) of the built reference (oracle/_ref)."""
    import ctypes as C
    import align_cases as ac
    L = ac.ref_lib()
    io, mo = ac._IdxOpt(), ac.MapOpt()
    assert L.mm_set_opt(None, C.byref(io), C.byref(mo)) == 0 and L.mm_set_opt(name.encode(), C.byref(io), C.byref(mo)) == 0
    return json.loads(json.dumps(dict(map={k: getattr(mo, k) for k in OPT_FIELDS}, index=dict(k=io.k, w=io.w, hpc=bool(io.flag & 1)))))


# ---------------------------------------------------------------- mm_est_err's walk
def anchor(qpos, rpos, span=15, rev=False, rid=0):
    return [(int(rev) << 63) | (rid << 32) | rpos, (span << 32) | qpos]


def mini(positions, span=15):
    return np.asarray([(span << 32) | p for p in positions], dtype=np.uint64)


def fwd_chain(positions, span=15, r0=1000):
    """Anchors of a forward chain whose query positions are `positions` (reference positions follow the same steps)."""
    return [anchor(p, r0 + p - positions[0], span) for p in positions]


def rev_chain(qlen, positions, span=15, r0=1000):
    """Anchors of a reverse-strand chain that covers the forward query positions `positions` (ascending): in the chain's order they descend."""
    out = []
    for i, p in enumerate(reversed(positions)):
        out.append(anchor(qlen - 1 - (p + 1 - span), r0 + (positions[-1] - p), span, rev=True))
    return out


def hit(as_, cnt, qs, rs, re, rid=0, rev=False):
    return {"as": as_, "cnt": cnt, "rid": rid, "qs": qs, "rs": rs, "re": re, "rev": rev}


def est_err_literal(rd, ref_len):
    """esterr.c:16-62 in plain Python on one read of est_err_host's input: [(n_match, n_tot)] with n_tot = -1 where the walk does not start, and sum_k."""
    mp = [int(v) for v in rd["mini_pos"]]
    n, qlen = len(mp), rd["qlen"]
    a = np.asarray(rd["anchors"], dtype=np.uint64).reshape(-1, 2)
    sum_k = sum(v >> 32 & 0xff for v in mp)
    pos = [v & 0xffffffff for v in mp]
    out = []

    def qpos(row):
        x, y = int(row[0]), int(row[1])
        p, span = y & 0xffffffff, y >> 32 & 0xff
        return qlen - 1 - (p + 1 - span) if x >> 63 else p

    def find(x):                                                # esterr.c:16-28: the binary search, whatever the order of mini_pos
        lo, hi = 0, n - 1
        while lo <= hi:
            m = (lo + hi) >> 1
            if pos[m] < x:
                lo = m + 1
            elif pos[m] > x:
                hi = m - 1
            else:
                return m
        return -1
    for h in rd["hits"]:
        if n == 0 or h["cnt"] == 0:
            out.append((0, -1))
            continue
        avg_k = np.float32(sum_k) / np.float32(n)
        at = lambda k: a[h["as"] + h["cnt"] - 1 - k] if h.get("rev") else a[h["as"] + k]
        st = en = find(qpos(at(0)))
        if st < 0:
            out.append((0, -1))
            continue
        k, n_match, j = 1, 1, st + 1
        while j < n and k < h["cnt"]:
            if qpos(at(k)) == pos[j]:
                k, en, n_match = k + 1, j, n_match + 1
            j += 1
        n_tot = en - st + 1
        n_tot += int(np.float32(h["qs"]) > avg_k and np.float32(h["rs"]) > avg_k)
        n_tot += int(np.float32(qlen - h["qs"]) > avg_k and np.float32(ref_len[h["rid"]] - h["re"]) > avg_k)
        out.append((n_match, n_tot))
    return out, sum_k


def crafted_reads():
    """(reads, ref_len, what each read is) for est_err_host / Engine.est_err: the cases of the walk."""
    ref_len = [5_000, 1_200]
    pos = list(range(20, 900, 17))                              # 52 minimizers of a 1 000-base read
    reads, what = [], []
    # forward hit with gaps between matched minimizers, and a reverse hit over the same positions
    picked = pos[3:40:3]
    reads.append(dict(qlen=1000, mini_pos=mini(pos), anchors=fwd_chain(picked) + rev_chain(1000, picked),
                      hits=[hit(0, len(picked), picked[0] - 14, 1000, 1000 + picked[-1] - picked[0] + 1),
                            hit(len(picked), len(picked), picked[0] - 14, 1000, 1000 + picked[-1] - picked[0] + 1, rev=True)]))
    what.append("forward and reverse")
    # cnt == 1 and cnt == 0
    reads.append(dict(qlen=1000, mini_pos=mini(pos), anchors=fwd_chain([pos[7]]), hits=[hit(0, 1, pos[7] - 14, 1000, 1001), hit(0, 0, 0, 0, 0)]))
    what.append("cnt 1 and cnt 0")
    # a hit touching both read ends and both reference ends: neither increment (rid 1: 1 200 long)
    reads.append(dict(qlen=1000, mini_pos=mini(pos), anchors=fwd_chain(pos[::2], r0=10), hits=[hit(0, len(pos[::2]), 5, 3, 1195, rid=1)]))
    what.append("no end increment")
    # the first anchor's position is no minimizer's: the mark
    reads.append(dict(qlen=1000, mini_pos=mini(pos), anchors=fwd_chain([pos[4] + 1, pos[6], pos[8]]), hits=[hit(0, 3, 100, 1000, 1100)]))
    what.append("first anchor absent")
    # the walk ends at j == n: the third anchor's position is absent, so j runs to the end and the rest of the chain is never met
    reads.append(dict(qlen=1000, mini_pos=mini(pos), anchors=fwd_chain([pos[2], pos[5], pos[9] + 3, pos[12], pos[20]]), hits=[hit(0, 5, 100, 1000, 1400)]))
    what.append("walk ends at j == n")
    # a read with no hits, and one without minimizers (its hit keeps div = -1)
    reads.append(dict(qlen=1000, mini_pos=mini(pos), anchors=np.zeros((0, 2), np.uint64), hits=[]))
    what.append("no hits")
    reads.append(dict(qlen=500, mini_pos=mini([]), anchors=fwd_chain([50, 80, 120]), hits=[hit(0, 3, 36, 1000, 1071)]))
    what.append("no minimizers")
    # spans differ (homopolymer compression): sum_k is no multiple of k, and a reverse chain's forward positions need not descend strictly
    spans = [15 + (i * 7) % 23 for i in range(len(pos))]
    mp = np.asarray([(s << 32) | p for s, p in zip(spans, pos)], dtype=np.uint64)
    idx = [5, 9, 10, 14, 30]
    fa = [anchor(pos[i], 2000 + pos[i], spans[i]) for i in idx]
    ra = [anchor(1000 - 1 - (pos[i] + 1 - spans[i]), 3000 - pos[i], spans[i], rev=True) for i in reversed(idx)]
    ra[1], ra[2] = ra[2], ra[1]                                 # out of order in forward position: the walk stops there
    reads.append(dict(qlen=1000, mini_pos=mp, anchors=fa + ra, hits=[hit(0, 5, pos[5] - spans[5] + 1, 2000, 2600), hit(5, 5, pos[5] - spans[5] + 1, 2400, 2900, rev=True)]))
    what.append("varying spans, a chain out of order")
    # positions that repeat: the argument for per-anchor searches does not hold, the literal walk runs
    dup_pos = pos[:20] + [pos[19]] + pos[20:]
    reads.append(dict(qlen=1000, mini_pos=mini(dup_pos), anchors=fwd_chain([pos[18], pos[19], pos[20], pos[25]]), hits=[hit(0, 4, 300, 1000, 1200)]))
    what.append("a position twice")
    return reads, ref_len, what


def synthetic_read(rng, n_mini, chain_lens, gap_hi=4, qlen=None, absent_every=0):
    """One read of n_mini minimizers and a hit per entry of chain_lens: each chain takes every 1..gap_hi-th minimizer from a random start (as far as the read
    goes); absent_every > 0: every absent_every-th chain has one position moved off its minimizer (the walk ends there)."""
    pos = (np.cumsum(rng.integers(3, 12, n_mini)) + 14).astype(np.int64)
    qlen = int(pos[-1]) + 20 if qlen is None else qlen
    span = 15
    parts, hits, n_a = [], [], 0
    for c, want in enumerate(chain_lens):
        rev = bool(rng.random() < 0.5)
        idx = int(rng.integers(0, max(1, n_mini - want))) + np.concatenate([[0], np.cumsum(rng.integers(1, gap_hi + 1, want - 1))]).astype(np.int64)
        p = pos[idx[idx < n_mini]].copy()
        if absent_every and c % absent_every == absent_every - 1:
            p[0 if c % 2 else len(p) // 2] += 1                    # (the first anchor's: the walk does not start)
        y = (qlen - 1 - (p[::-1] + 1 - span)) if rev else p
        x = 1000 + (p[-1] - p[::-1] if rev else p - p[0])
        parts.append(np.stack([x.astype(np.uint64) | np.uint64((1 << 63) if rev else 0), ((span << 32) | y).astype(np.uint64)], axis=1))
        hits.append(hit(n_a, len(p), int(p[0]) - 14, 1000, 1000 + int(p[-1] - p[0]) + 1, rev=rev))
        n_a += len(p)
    anchors = np.concatenate(parts) if parts else np.zeros((0, 2), np.uint64)
    return dict(qlen=qlen, mini_pos=mini([int(v) for v in pos]), anchors=anchors, hits=hits)


# ---------------------------------------------------------------- the walk at the shapes of the wave instantiation (hits of 64 anchors or more)
LONG_CNTS = (64, 65, 128, 129, 200)
DEFECTS = ("swap", "same", "off")


def read_layout(n_mini, seed=0):
    """(positions, spans) of a read of n_mini minimizers: positions ascend by 3..11, spans vary as in crafted_reads' "varying spans" case."""
    rng = np.random.default_rng(1000 + seed)
    pos = (np.cumsum(rng.integers(3, 12, n_mini)) + 40).astype(np.int64)
    spans = (15 + (np.arange(n_mini) * 7) % 23).astype(np.int64)
    return pos, spans


def mini_of(pos, spans):
    return (np.asarray(spans, dtype=np.uint64) << np.uint64(32)) | np.asarray(pos, dtype=np.uint64)


def chain_on(qlen, pos, spans, rev=False, r0=1000):
    """The anchors ((n, 2) uint64, in the chain's order) of a chain over the forward query positions pos (in query order) with the spans given; a reverse
    chain's own order is the query order backwards."""
    p, s = np.asarray(pos, dtype=np.int64), np.asarray(spans, dtype=np.int64)
    if rev:
        p, s = p[::-1], s[::-1]
        x = (r0 + np.arange(len(p)) * 16).astype(np.uint64) | np.uint64(1 << 63)
        y = qlen - 1 - (p + 1 - s)
    else:
        x, y = (r0 + np.arange(len(p)) * 16).astype(np.uint64), p
    assert (y >= 0).all() and (y < 2**31).all()
    return np.stack([x, ((s << 32) | y).astype(np.uint64)], axis=1)


def with_defect(pos, spans, kind, k):
    """The chain's forward positions (query order) with one defect at k >= 1, so that the walk counts k anchors: "swap" anchors k - 1 and k change places, "same"
    anchor k sits at anchor k - 1's position, "off" anchor k is one base off its minimizer."""
    p, s = np.array(pos, dtype=np.int64), np.array(spans, dtype=np.int64)
    if kind == "swap":
        p[[k - 1, k]], s[[k - 1, k]] = p[[k, k - 1]], s[[k, k - 1]]
    elif kind == "same":
        p[k], s[k] = p[k - 1], s[k - 1]
    elif kind == "off":
        p[k] += 1
    else:
        raise ValueError(kind)
    return p, s


class ReadBuilder:
    """One read of est_err_host's input, its hits added one by one."""

    def __init__(self, qlen, mini_pos):
        self.qlen, self.mini_pos, self.parts, self.hits, self.n_a = int(qlen), np.asarray(mini_pos, dtype=np.uint64), [], [], 0

    def add(self, pos, spans, rev=False, qs=200, rs=200, re=2000, rid=0):
        a = chain_on(self.qlen, pos, spans, rev, r0=1000 + 7 * len(self.hits))
        self.hits.append(hit(self.n_a, len(a), qs, rs, re, rid=rid, rev=rev))
        self.parts.append(a)
        self.n_a += len(a)
        return self

    def read(self):
        return dict(qlen=self.qlen, mini_pos=self.mini_pos, anchors=np.concatenate(self.parts) if self.parts else np.zeros((0, 2), np.uint64), hits=self.hits)


LONG_REF_LEN = [5_000, 1_200]


def crafted_long():
    """(reads, ref_len, what each read is): the walk's cases at the sizes of k_est_err<64> (and their 16-lane twins where the case has one).  Every read is small
    enough for est_err_literal; big_read() is the one that is not."""
    reads, what = [], []

    def done(b, name):
        reads.append(b.read())
        what.append(name)
    n = 460
    pos, spans = read_layout(n)
    qlen = int(pos[-1]) + 600                                                                  # (the read goes on past its last minimizer: room for anchors beyond it)
    # one defect at k in {1, 63, 64, 65, cnt - 1} of a chain of cnt anchors over every minimizer, or every first to third, from a start inside the read
    for cnt in LONG_CNTS:
        for rev in (False, True):
            b = ReadBuilder(qlen, mini_of(pos, spans))
            for gaps in (1, 3):
                idx = 7 + np.concatenate([[0], np.cumsum(1 + (np.arange(cnt - 1) * 5) % gaps)])
                assert idx[-1] < n
                b.add(pos[idx], spans[idx], rev)                                               # no defect: cnt anchors counted
                for kind in DEFECTS:
                    for k in sorted({1, 63, 64, 65, cnt - 1}):
                        if k < cnt:
                            b.add(*with_defect(pos[idx], spans[idx], kind, k), rev=rev)
            done(b, f"cnt {cnt} {'reverse' if rev else 'forward'}")
    # two failures of different kinds in different rounds of a hit: the earlier one ends the walk, valid anchors after it do not count
    b = ReadBuilder(qlen, mini_of(pos, spans))
    idx = 20 + 2 * np.arange(128)
    for rev in (False, True):
        for first, second in (("off", "swap"), ("swap", "off"), ("same", "off"), ("off", "same")):
            p, s = with_defect(pos[idx], spans[idx], second, 100)
            b.add(*with_defect(p, s, first, 70), rev=rev)
    done(b, "two defects, 70 and 100")
    # the chain goes on beyond the read's last minimizer: cnt > n - st, positions past the last one; and hits whose first anchor is the last minimizer
    b = ReadBuilder(qlen, mini_of(pos, spans))
    beyond = lambda m: int(pos[-1]) + 5 * (1 + np.arange(m))
    for tail, more in ((70, 10), (5, 3), (64, 1), (1, 4), (1, 70), (130, 80)):
        for rev in (False, True):
            b.add(np.concatenate([pos[n - tail:], beyond(more)]), np.concatenate([spans[n - tail:], np.full(more, 15)]), rev)
    done(b, "beyond the last minimizer")
    # mini_pos not strictly ascending: the literal walk, in both instantiations (hits of 5, 64 and 200 anchors from minimizer 100 on)
    for name, change in (("twice before st", ("dup", 50)), ("twice inside", ("dup", 102)), ("twice after en", ("dup", 420)), ("a descending pair", ("swap", 102)),
                         ("the first anchor's twice", ("dup", 100)), ("a descending pair before st", ("swap", 30))):
        mp = mini_of(pos, spans)
        mp = np.insert(mp, change[1], mp[change[1]]) if change[0] == "dup" else np.concatenate([mp[:change[1]], mp[change[1] + 1:change[1] + 2], mp[change[1]:change[1] + 1], mp[change[1] + 2:]])
        b = ReadBuilder(qlen, mp)
        for cnt in (5, 64, 200):
            idx = 100 + np.arange(cnt)
            for rev in (False, True):
                b.add(pos[idx], spans[idx], rev)
                b.add(*with_defect(pos[idx], spans[idx], "off", cnt - 2), rev=rev)
                b.add(pos[idx[::2]], spans[idx[::2]], rev)                                     # every second minimizer: the walk passes the changed place without asking for it
        done(b, "mini_pos: " + name)
    # coordinates near 2^31
    big_q = 2**31 - 2
    bp = (2**30 + np.arange(96) * ((2**30 - 40) // 96)).astype(np.int64)
    bs = (15 + (np.arange(96) * 5) % 11).astype(np.int64)
    assert bp[-1] <= 2**31 - 20
    b = ReadBuilder(big_q, mini_of(bp, bs))
    for cnt, start in ((8, 3), (70, 20), (96, 0)):
        for rev in (False, True):
            b.add(bp[start:start + cnt], bs[start:start + cnt], rev, qs=int(bp[start]) - 14, re=4_000)
            b.add(*with_defect(bp[start:start + cnt], bs[start:start + cnt], "off", cnt - 3), rev=rev, qs=big_q - 10)
    done(b, "coordinates near 2^31")
    # the comparisons against avg_k at equality: qs, rs, qlen - qs and ref_len - re at floor(avg_k) and floor(avg_k) + 1, one at a time, the partner well above
    for name, sp in (("avg_k exactly 16", np.full(52, 16)), ("avg_k 17.288...", np.asarray([15] * 35 + [22] * 17))):
        p = 20 + 23 * np.arange(52)
        b = ReadBuilder(2_000, mini_of(p, sp))
        lo = int(sp.sum() // 52)
        for cnt in (6, 52):                                                                    # (52 minimizers: the 16-lane form; the wave's turn is below)
            for v in (lo, lo + 1):
                for rev in (False, True):
                    b.add(p[:cnt], sp[:cnt], rev, qs=v, rs=300, re=2_000)
                    b.add(p[:cnt], sp[:cnt], rev, qs=300, rs=v, re=2_000)
                    b.add(p[:cnt], sp[:cnt], rev, qs=2_000 - v, rs=300, re=2_000)
                    b.add(p[:cnt], sp[:cnt], rev, qs=300, rs=300, re=LONG_REF_LEN[0] - v)
                    b.add(p[:cnt], sp[:cnt], rev, qs=v, rs=v, re=LONG_REF_LEN[0] - v)
        done(b, name)
        p2 = 20 + 23 * np.arange(208)
        sp2 = np.tile(sp, 4)
        b = ReadBuilder(8_000, mini_of(p2, sp2))
        for v in (lo, lo + 1):
            for rev in (False, True):
                b.add(p2[:130], sp2[:130], rev, qs=v, rs=300, re=2_000)
                b.add(p2[:130], sp2[:130], rev, qs=300, rs=v, re=2_000)
                b.add(p2[:130], sp2[:130], rev, qs=8_000 - v, rs=300, re=2_000)
                b.add(p2[:130], sp2[:130], rev, qs=300, rs=300, re=LONG_REF_LEN[0] - v)
        done(b, name + ", hits of 130")
    return reads, LONG_REF_LEN, what


BIG_N = 1_300_001


def big_read():
    """One read of 1 300 001 minimizers with spans 15 and 21 in turn, two of them 16: sum_k = 18 n - 1 = 23 400 017, odd and above 2^24, so (float)sum_k is
    23 400 016 and avg_k the float below 18 -- computed exactly it would be 18.  Three hits; the first has qs = rs = 18."""
    n = BIG_N
    spans = np.where(np.arange(n) % 2 == 0, 15, 21).astype(np.int64)
    spans[[0, 2]] = 16
    assert int(spans.sum()) == 18 * n - 1
    pos = np.cumsum(3 + (np.arange(n) * 7) % 9, dtype=np.int64) + 40
    qlen = int(pos[-1]) + 60
    assert qlen < 2**31
    b = ReadBuilder(qlen, mini_of(pos, spans))
    i0 = 1_000 + np.arange(40)
    b.add(pos[i0], spans[i0], False, qs=18, rs=18, re=2_000)
    i1 = 700_000 + 3 * np.arange(200)
    b.add(pos[i1], spans[i1], True, qs=18, rs=17, re=2_000)
    i2 = 1_200_000 + 2 * np.arange(50_000)
    b.add(*with_defect(pos[i2], spans[i2], "off", 33_333), rev=False, qs=500, rs=500, re=LONG_REF_LEN[0] - 18)
    return b.read()


def stride_batch(cu, seed=13):
    """One batch that makes each of launch_est_err's three grids stride (it caps a launch at ceil(32 cu / 4) blocks: 32 cu reads, 32 cu hits of a wave, 128 cu
    hits of 16 lanes per pass): 40 cu small reads of 5-40 minimizers and 0-8 short hits, 300 larger reads that carry more than 32 cu hits of 64-80 anchors
    among them, and a read without minimizers followed by one without hits at each end and from index 32 cu on.  Returns (reads, ref_len, counts)."""
    rng = np.random.default_rng(seed)
    n_small, n_large = 40 * cu, 300
    per_large = -(-(32 * cu) * 11 // (10 * n_large))                                # (a tenth more than needed: a chain that meets the read's end is cut short)
    no_mini = lambda: dict(qlen=500, mini_pos=mini([]), anchors=np.asarray(fwd_chain([50, 80, 120]), dtype=np.uint64), hits=[hit(0, 3, 36, 1000, 1071)])
    no_hits = lambda: dict(qlen=1000, mini_pos=mini(list(range(20, 900, 17))), anchors=np.zeros((0, 2), np.uint64), hits=[])
    body = []
    every = max(1, n_small // n_large)
    for i in range(n_small):
        n_mini = int(rng.integers(5, 41))
        body.append(synthetic_read(rng, n_mini, [int(v) for v in rng.integers(1, min(n_mini, 30) + 1, int(rng.integers(0, 9)))], gap_hi=2, absent_every=5))
        if i % every == every - 1 and i // every < n_large:
            body.append(synthetic_read(rng, 1_200, [int(v) for v in rng.integers(64, 81, per_large)], gap_hi=2, absent_every=6))
    at = 32 * cu - 2                                                              # (two reads lead the batch)
    reads = [no_mini(), no_hits()] + body[:at] + [no_mini(), no_hits()] + body[at:] + [no_mini(), no_hits()]
    cnts = [h["cnt"] for rd in reads for h in rd["hits"]]
    counts = dict(reads=len(reads), short_hits=sum(c < 64 for c in cnts), long_hits=sum(c >= 64 for c in cnts))
    return reads, [100_000], counts
