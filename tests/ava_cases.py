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
    """esterr.c:30-62 in plain Python on one read of est_err_host's input: [(n_match, n_tot)] with n_tot = -1 where the walk does not start, and sum_k."""
    mp = [int(v) for v in rd["mini_pos"]]
    n, qlen = len(mp), rd["qlen"]
    a = np.asarray(rd["anchors"], dtype=np.uint64).reshape(-1, 2)
    sum_k = sum(v >> 32 & 0xff for v in mp)
    out = []

    def qpos(row):
        x, y = int(row[0]), int(row[1])
        p, span = y & 0xffffffff, y >> 32 & 0xff
        return qlen - 1 - (p + 1 - span) if x >> 63 else p
    for h in rd["hits"]:
        if n == 0 or h["cnt"] == 0:
            out.append((0, -1))
            continue
        avg_k = np.float32(sum_k) / np.float32(n)
        at = lambda k: a[h["as"] + h["cnt"] - 1 - k] if h.get("rev") else a[h["as"] + k]
        pos = [v & 0xffffffff for v in mp]
        x0 = qpos(at(0))
        if x0 not in pos:
            out.append((0, -1))
            continue
        st = en = pos.index(x0)
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
