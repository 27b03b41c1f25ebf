"""Crafted single-chain batches for the device backend of the alignment of hits (csrc/align_kernels.hip: k_al_gather, k_al_zdrop, the second pass on resident bytes),
built on sr_cases.chain_case: one read, one chain, anchors made here.  Three families -- A: stretches that cross k_al_gather's 4 KiB slices on either side, strand and
direction; B: drops at mm_test_zdrop's thresholds, and the one dropping fill at chosen places of k_al_zdrop's length-sorted list; C: the inversion probe where its score
crosses the threshold.  What the reference's mm_align_skeleton answers on them is committed under tests/golden/align_crafted (tests/tools/gen_golden_align_crafted.py).
Test infrastructure only: imported by tests/test_align_crafted_cpu.py, tests/test_gpu_align_crafted.py and that tool."""
import copy
import json
import os
import re

import numpy as np

import align_cases as ac
import golden_io
import mm2gb_amd as mm
import sim_reads
import sr_cases

GOLD = os.path.join(golden_io.GOLD, "align_crafted")
K = 15                                   # the anchors' span (map-ont's k)
RF_REV = 1 << 10                         # mm_reg1_t's rev bit in the record's flag word
REF_LEAD = 50                            # chain_case's reference starts this many bases before the read
# the counts of mm.ALN_COUNTS that say which paths a run took (cells and their like left out)
KEEP = ("fill_one_pass", "fill_two_pass", "split", "split_refused", "inv", "inv_probe_hit", "rev_chain", "left_end", "left_short", "left_at_0", "right_end", "right_short",
        "filtered", "rounds", "reads_3_rounds", "jobs")


def al_slice():
    """AL_SLICE as csrc/align_kernels.hip states it (no call exposes it)."""
    src = open(os.path.join(os.path.dirname(os.path.abspath(mm.__file__)), "csrc", "align_kernels.hip")).read()
    return int(re.search(r"constexpr int AL_SLICE = (\d+);", src).group(1))


SLICE = 4096                             # k_al_gather's documented 4 KiB: the cases are built for it, and the tests hold al_slice() against it


# ---------------------------------------------------------------- one chain
def edits(q_n=(), q_x=(), t_n=(), t_x=(), q_del=(), t_del=(), q_inv=None, q_comp=()):
    """A job's edits by alignment column (a column holds one base of either side before anything is removed): N / another base written into the query or the target,
    the query's or the target's base of a column removed, q_inv = (column, n): the query's n bases from there replaced by their reverse complement; q_comp = ((column, other column), ...): the query's base of a column replaced by the
    complement of the target's base of another."""
    return dict(q_n=tuple(q_n), q_x=tuple(q_x), t_n=tuple(t_n), t_x=tuple(t_x), q_del=tuple(q_del), t_del=tuple(t_del), q_inv=q_inv, q_comp=tuple(q_comp))


def revcomp(s):
    """sim_reads.revcomp, which knows the four bases alone, with N kept."""
    out = sim_reads.revcomp(s)
    out[s[::-1] == ord("N")] = ord("N")
    return out


def _apply(q, t, e):
    """q, t: the two sides of a job in the job's order, equal before the edits.  Returns them edited."""
    if not e:
        return q, t
    q, t = q.copy(), t.copy()
    for c in e["q_n"]:
        q[c] = ord("N")
    for c in e["t_n"]:
        t[c] = ord("N")
    for c in e["q_x"]:
        q[c] = sr_cases._other(q[c])
    for c in e["t_x"]:
        t[c] = sr_cases._other(t[c])
    if e["q_inv"]:
        c, n = e["q_inv"]
        q[c:c + n] = revcomp(q[c:c + n])
    for c, src in e["q_comp"]:
        q[c] = revcomp(t[src:src + 1])[0]
    return np.delete(q, list(e["q_del"])), np.delete(t, list(e["t_del"]))


def chain(rng, length, fill=None, left=None, right=None, lead=30, tail=30, rev=False, at=None, fills=None):
    """sr_cases.chain_case's read and reference with anchors of span 15 made here, so that the DP jobs are known exactly: the first anchor ends on the column before the
    stretch, the last on the stretch's last column, further ones on the columns `at` (ascending, counted in the stretch before any removal) -- the left extension is then
    the `lead` bases before the stretch, read backwards, the right extension the `tail` bases behind it, and the stretch falls into one gap fill per anchor after the first.
    fill / left / right: edits() in the job's own columns (the left extension's count backwards from the stretch); fills: {fill number: edits()} in that fill's columns, in
    place of `fill`.  rev: the same case on the reverse strand -- the read reverse-complemented, bit 63 in every anchor's x, the rev bit in the record's flags, qs / qe
    mirrored.  Returns (reference, read, record, anchors) as chain_case does."""
    assert lead >= K
    t, q, reg, _ = sr_cases.chain_case(rng, length, None, lead, tail)
    t, q = np.frombuffer(t, np.uint8), np.frombuffer(q, np.uint8)
    cuts = [0] + [c + 1 for c in (at or [])] + [length]
    assert all(b - a >= K for a, b in zip(cuts, cuts[1:]))
    if fills is None:
        assert fill is None or len(cuts) == 2
        fills = {0: fill}
    lq, lt = _apply(q[:lead][::-1], t[REF_LEAD:REF_LEAD + lead][::-1], left)
    q_parts, t_parts = [lq[::-1]], [t[:REF_LEAD], lt[::-1]]
    q_end, t_end = [len(lq) - 1], [REF_LEAD + len(lt) - 1]                   # where each anchor ends
    for f, (a, b) in enumerate(zip(cuts, cuts[1:])):
        fq, ft = _apply(q[lead + a:lead + b], t[REF_LEAD + lead + a:REF_LEAD + lead + b], fills.get(f))
        q_parts.append(fq); t_parts.append(ft)
        q_end.append(q_end[-1] + len(fq)); t_end.append(t_end[-1] + len(ft))
    rq, rt = _apply(q[lead + length:], t[REF_LEAD + lead + length:REF_LEAD + lead + length + tail], right)
    q2, t2 = np.concatenate(q_parts + [rq]), np.concatenate(t_parts + [rt, t[REF_LEAD + lead + length + tail:]])
    a = np.asarray([[x, K << 32 | y] for x, y in zip(t_end, q_end)], np.uint64)
    reg = reg.copy()
    reg["cnt"], reg["score"], reg["score0"] = len(a), K * len(a), K * len(a)
    reg["qs"], reg["qe"], reg["rs"], reg["re"] = q_end[0] + 1 - K, q_end[-1] + 1, t_end[0] + 1 - K, t_end[-1] + 1
    reg["mlen"] = reg["blen"] = K * len(a)
    if rev:
        q2 = revcomp(q2)
        a[:, 0] |= np.uint64(1 << 63)
        reg["flags"] |= RF_REV
        reg["qs"], reg["qe"] = len(q2) - reg["qe"], len(q2) - reg["qs"]
    return t2.tobytes(), q2.tobytes(), reg, a


def join(cases, order=None):
    """Cases (name -> chain()'s tuple) as the alignment calls' input less the options: one reference sequence and one read per case, in the order given (names)."""
    names = list(cases) if order is None else list(order)
    regs, anchors = [], []
    for i, n in enumerate(names):
        g = cases[n][2].copy()
        g["rid"] = i
        regs.append(g)
        anchors.append(cases[n][3] + np.asarray([[i << 32, 0]], np.uint64))
    return dict(k=K, hpc=False, refs=[cases[n][0] for n in names], reads=[cases[n][1] for n in names], regs=regs, anchors=anchors), names


def batch(opt, cases, order=None):
    b, names = join(cases, order)
    b["opt"] = opt
    return b, names


def pick(b, want, idx):
    """Reads idx of a batch as a batch of their own (every read has its own reference: renumbered), with the matching expectations."""
    idx = [int(i) for i in idx]
    out = dict(opt=b["opt"], k=b["k"], hpc=b["hpc"], refs=[b["refs"][i] for i in idx], reads=[b["reads"][i] for i in idx], regs=[], anchors=[])
    w2 = []
    for new, i in enumerate(idx):
        g = b["regs"][i].copy(); g["rid"] = new
        a = b["anchors"][i].copy(); a[:, 0] = (a[:, 0] & np.uint64((1 << 63) | 0xffffffff)) | np.uint64(new << 32)
        out["regs"].append(g); out["anchors"].append(a)
        if want is not None:
            r = want[i][0].copy(); r["rid"] = new
            w2.append((r, want[i][1], want[i][2]))
    return out, w2


def as_single(b):
    """A batch under single-affine scoring: q2 = q, e2 = e (the _extz calls)."""
    c = dict(b)
    c["opt"] = copy.copy(b["opt"])
    c["opt"].q2, c["opt"].e2 = b["opt"].q, b["opt"].e
    return c


# ---------------------------------------------------------------- A: gather seams
A_OPT = dict(min_cnt=1, bw_long=500)     # a fill's band is 751: the direction bytes of the longest case stay near 12 MB
A_FILLS = (4095, 4096, 4097, 8191, 8193)


def seam_edits(n, balance=True):
    """Edits around every slice cut inside a job of n columns, each only where the job still holds its column: N in the query on the byte before the cut, another base on
    the cut's byte, the query's base two columns on removed (a one-base deletion right behind byte cut + 1), N in the target one column further -- behind the cut, which
    for a job read backwards is the side nearer the read's start.  balance: the target's base 40 columns on removed as well, so that a fill's two sides stay equal in
    length; from there both sides lie one byte earlier, and the next cut's columns are moved by as much."""
    q_n, q_x, q_del, t_n, t_del, shift = [], [], [], [], [], 0
    for cut in range(SLICE, n, SLICE):
        for col, into in ((cut - 1 + shift, q_n), (cut + shift, q_x), (cut + 3 + shift, t_n)):
            if col < n:
                into.append(col)
        if cut + 40 + shift < n:
            q_del.append(cut + 2 + shift)
            if balance:
                t_del.append(cut + 40 + shift)
                shift += 1
    return edits(q_n=q_n, q_x=q_x, q_del=q_del, t_n=t_n, t_del=t_del)


def cases_a(seed=41):
    """name -> chain: fills of 4095 .. 8193 columns with equal sides (a removed query base is balanced by a removed target base, so the stretch is built one column longer per
    cut it holds edits for), fills with one side past the cut and the other about 3000, a left and a right extension of 4500, each on both strands."""
    rng = np.random.default_rng(seed)
    out = {}
    for rev in (False, True):
        s = "_rev" if rev else ""
        for n in A_FILLS:
            e = seam_edits(n)
            extra = len(e["q_del"])
            if extra:
                e = seam_edits(n + extra)
                assert len(e["q_del"]) == extra
            out[f"fill{n}{s}"] = chain(rng, n + extra, fill=e, rev=rev)
        # 4097 against about 3000: 1097 bases of one side removed in one block well before the cut; the second slice then has one live side
        blk = list(range(1500, 1500 + 1097))
        e = seam_edits(4097, balance=False)
        out[f"q4097_t3000{s}"] = chain(rng, 4097, fill=dict(e, t_del=tuple(blk)), rev=rev)
        out[f"t4097_q3000{s}"] = chain(rng, 4097, fill=dict(e, q_del=tuple(blk), q_n=(), q_x=(), t_n=(SLICE - 1,), t_x=(SLICE,)), rev=rev)
        out[f"left4500{s}"] = chain(rng, 300, left=seam_edits(4500, balance=False), lead=4500, rev=rev)
        out[f"right4500{s}"] = chain(rng, 300, right=seam_edits(4500, balance=False), tail=4500, rev=rev)
    return out


def tiny_cases(seed=42, n=30):
    """30 reads with one fill of 17 .. 46 columns each (1 .. 15 mod 16, never 0): between the seam cases they move every arena offset by another remainder."""
    rng = np.random.default_rng(seed)
    lens = [L for L in range(17, 64) if L % 16][:n]
    return {f"tiny{L}{'_rev' if i & 1 else ''}": chain(rng, L, rev=bool(i & 1)) for i, L in enumerate(lens)}


def batches_a():
    """name -> (batch, case names): every seam case shuffled among the tiny reads.  The seam cases alone, and each alone, are taken out of it (pick)."""
    both = dict(cases_a(), **tiny_cases())
    order = [list(both)[i] for i in np.random.default_rng(43).permutation(len(both))]
    return {"A_mixed": batch(mm.align_opt("map-ont", **A_OPT), both, order)}


def seam_reads(names):
    """Where the seam cases lie in A_mixed."""
    return [i for i, n in enumerate(names) if not n.startswith("tiny")]


# ---------------------------------------------------------------- B: drop thresholds
B_OPT = dict(min_cnt=1, zdrop=80, zdrop_inv=80, q=40, e=8, q2=60, e2=7)      # a 2, b 4, sc_ambi 1 (map-ont): with gaps this dear a run of mismatches stays M
B_AT = [399]                             # stretch 800: an anchor ends on column 399, so the edits from column 100 of the second fill have anchors on either side


def _run(mism, n_n, at=100):
    """mism mismatches and n_n N-columns in a row from column `at` of a fill: 4 * mism + n_n below the maximum."""
    return edits(q_x=range(at, at + mism), q_n=range(at + mism, at + mism + n_n))


def cases_b(seed=51):
    """name -> chain.  Drops of exactly zdrop (stays) and zdrop + 1 (runs again and splits) two ways; the tie at the maximum; a deletion between the maximum and the
    deepest column, where the walk's - diff * e and the gap's own e decide."""
    rng = np.random.default_rng(seed)
    out = {}
    for rev in (False, True):
        s = "_rev" if rev else ""
        two = lambda e, **kw: chain(rng, 800, fills={1: e}, at=B_AT, rev=rev, **kw)
        out[f"mm20{s}"] = two(_run(20, 0))                   # 80: not a drop (strict >)
        out[f"mm20_n1{s}"] = two(_run(20, 1))                # 81
        out[f"mm19_n4{s}"] = two(_run(19, 4))                # 80
        out[f"mm19_n5{s}"] = two(_run(19, 5))                # 81
        # sr_cases.ungapped_cases' tie_at_max at a 2, b 4: one mismatch (-4), two matches (+4): column 112 holds the maximum of column 109 again and the maximum moves there;
        # the drop that follows is measured from column 112.  Alone it changes positions only; with the deletion of tie_gap it changes the drop's size
        tie = lambda m, n: edits(q_x=[110] + list(range(113, 113 + m)), q_n=range(113 + m, 113 + m + n))
        out[f"tie_80{s}"] = two(tie(20, 0))
        out[f"tie_81{s}"] = two(tie(20, 1))
        # a deletion of 3 query bases (40 + 3 * 8 = 64 down), 30 matches (60 up: 4 short of the maximum, which stays before the gap), then mismatches and N: the walk takes
        # 3 * e back, so the drop is 4 + 4 * mism + n - 24: 25 mismatches are 80: stays; one N more drops.  Without the - diff * e term both are 24 higher and both drop;
        # with e = 0 in the walk the gap costs 40, the 30 matches carry the maximum past it, and both are 100 and 101: both drop
        gap = lambda m, n: edits(q_del=[100, 101, 102], q_x=range(133, 133 + m), q_n=range(133 + m, 133 + m + n))
        for n in (0, 1):                 # drawn again until the gap cannot slide: the reference's base on either side of the removed three differs from the one it would swap with
            while True:
                c = two(gap(25, n))
                t = np.frombuffer(c[0], np.uint8)[REF_LEAD + 30 + 400:]
                if t[99] != t[102] and t[100] != t[103]:
                    break
            out[f"del3_{80 + n}{s}"] = c
        # the tie behind a deletion: maximum at column 99, one query base removed (48 down), 24 matches: the score is the maximum's again and the maximum moves past the gap.
        # 20 mismatches + N from there: 81, a drop; measured from column 99 it would be 81 - e
        out[f"tie_gap_80{s}"] = two(edits(q_del=[100], q_x=range(125, 145)))
        out[f"tie_gap_81{s}"] = two(edits(q_del=[100], q_x=range(125, 145), q_n=[145]))
    return out


B_DROPS = ("mm20_n1", "mm19_n5", "tie_81", "del3_81", "tie_gap_81")
B_STAYS = ("mm20", "mm19_n4", "tie_80", "del3_80", "tie_gap_80")
N_FILLS = 132                            # fills of one round in the list batches: three workgroups of k_al_zdrop
LIST_PLACES = {"first": 0, "at63": 63, "at64": 64, "last": N_FILLS - 1}        # where the dropping fill lies in the list sorted by qlen + tlen, longest first


def cases_list(place, seed=61, n_reads=6):
    """Six reads of 22 fills each, the 132 fills of 200 .. 331 columns all different in length and dealt round-robin; the fill at `place` of the descending order carries 20
    mismatches and an N (a drop of 81), no other fill an edit (place None: no fill at all).  The edits draw no random numbers: every place gives the same sequences but
    for one read."""
    rng = np.random.default_rng(seed)
    lens = list(range(200 + N_FILLS - 1, 199, -1))                        # descending: lens[p] is list position p
    out = {}
    for r in range(n_reads):
        mine = list(range(r, N_FILLS, n_reads))
        if r & 1:
            mine.reverse()
        at, col = [], -1
        for p in mine[:-1]:
            col += lens[p]
            at.append(col)
        total = sum(lens[p] for p in mine)
        fills = {f: _run(20, 1, at=60) for f, p in enumerate(mine) if p == place}
        out[f"read{r}"] = chain(rng, total, fills=fills, at=at, rev=r in (2, 3))
    return out


def batches_b():
    """The threshold cases, and the list batch with no drop; list_batch() makes the four with one."""
    o = mm.align_opt("map-ont", **B_OPT)
    return {"B": batch(o, cases_b()), "B_list": batch(o, cases_list(None))}


def list_read(place):
    """Which read of the list batch holds list position `place`."""
    return LIST_PLACES[place] % 6


def list_batch(place):
    return batch(mm.align_opt("map-ont", **B_OPT), cases_list(LIST_PLACES[place]))


def put(b, want, r, one, want1):
    """A batch and its expectations with read r replaced by the only read of `one` (the reverse of pick)."""
    out = dict(b, refs=list(b["refs"]), reads=list(b["reads"]), regs=list(b["regs"]), anchors=list(b["anchors"]))
    out["refs"][r], out["reads"][r] = one["refs"][0], one["reads"][0]
    g = one["regs"][0].copy(); g["rid"] = r
    a = one["anchors"][0].copy(); a[:, 0] = (a[:, 0] & np.uint64((1 << 63) | 0xffffffff)) | np.uint64(r << 32)
    out["regs"][r], out["anchors"][r] = g, a
    w = list(want)
    wr = want1[0][0].copy(); wr["rid"] = r
    w[r] = (wr, want1[0][1], want1[0][2])
    return out, w


# ---------------------------------------------------------------- C: the inversion probe at its threshold
C_OPT = dict(min_cnt=1, zdrop=400, zdrop_inv=40)


def inv_case(rng, n, col, rev=False):
    """A stretch of 1200 in two fills (an anchor ends on column 599) with the query's n bases from column `col` of the first fill reverse-complemented."""
    return chain(rng, 1200, fills={0: edits(q_inv=(col, n))}, at=[599], rev=rev)


C_MID, C_EDGE = 300, 1                   # the block's first column: inside the fill, and one column from the stretch's edge (the walk's `from` side is the fill's first column)
# the block length at which inv_probe_hit goes 0 -> 1 on the host form (swept over 30 .. 79): the probe needs 80, which is 40 matching bases.  Inside the fill it stays 1 from there;
# at the edge 41 misses again (the deepest column moves) and 42 onwards hit
C_FLIP = {"mid": 40, "edge": 40}
C_HITS = {"mid": (0, 1, 1), "edge": (0, 1, 0)}       # inv_probe_hit at n - 1, n, n + 1


# The probe aligns the reverse complement of the query's [q_from, q_to) to the target's [t_from, t_to) (align.c:69-84): the maximum's column is inside, the deepest is not.
# With a block of 40 in the middle only the `to` side is tight (the deepest column is the first behind the block); the pins make every one of the four positions decide a
# probe of exactly 80, 39 columns of the block and one more.  "P": the query's base behind the block is the complement of the target's base before it (and a mismatch
# where it stands, as is the next one, so the deepest column lies two behind the block): the 40th column is the target's t_from against the query's q_to - 2.  "Q": a
# seed whose target has that complement behind the block by itself, and two mismatches in the query there: the 40th column is the query's q_from against the target's
# t_to - 1.  (kind, generator seed, block length): found by a sweep over seeds with host builds whose walk reported one position one off -- t_from + 1, q_from + 1,
# t_to - 1, q_to - 1 in turn; each pin hits as it is and misses under the variants named.
PINS = (("P", 113, 39),                  # t_from + 1, q_to - 1
        ("P", 111, 40),                  # t_from + 1, q_from + 1
        ("Q", 103, 39),                  # q_from + 1
        ("Q", 106, 39))                  # t_to - 1


def pin_case(kind, seed, n, rev=False, col=C_MID):
    t = np.frombuffer(chain(np.random.default_rng(seed), 1200, at=[599])[0], np.uint8)[REF_LEAD + 30:]
    flank = revcomp(t[col - 1:col])[0] == t[col + n]
    assert flank == (kind == "Q"), "the seed's sequence does not make this kind of pin"
    e = edits(q_inv=(col, n), q_comp=[(col + n, col - 1)], q_x=[col + n + 1]) if kind == "P" else edits(q_inv=(col, n), q_x=[col + n, col + n + 1])
    return chain(np.random.default_rng(seed), 1200, fills={0: e}, at=[599], rev=rev)


def cases_c(seed=71):
    out = {}
    for kind, sd, n in PINS:
        for rev in (False, True):
            out[f"pin_{kind}_{sd}_{n}{'_rev' if rev else ''}"] = pin_case(kind, sd, n, rev)
    for where, col in (("mid", C_MID), ("edge", C_EDGE)):
        n0 = C_FLIP[where]
        for rev in (False, True):
            for n in (n0 - 1, n0, n0 + 1):
                # every case from the same generator state: the three lengths differ in the block's length alone
                out[f"inv_{where}_{n}{'_rev' if rev else ''}"] = inv_case(np.random.default_rng(seed + col), n, col, rev)
    return out


def batches_c():
    return {"C": batch(mm.align_opt("map-ont", **C_OPT), cases_c())}


def all_batches():
    """name -> (batch, case names): everything the fixture records."""
    out = {}
    out.update(batches_a()); out.update(batches_b()); out.update(batches_c())
    return out


# ---------------------------------------------------------------- what each case is built for: the host form's counts on the case alone
def counts_alone(b, i, single=False):
    one, _ = pick(b, None, [i])
    if single:
        return mm.align_regs_extz_host(as_single(one)["opt"], one["k"], one["hpc"], one["refs"], one["reads"], one["regs"], one["anchors"], threads=1)
    return ac.run_host(one, threads=1)


# ---------------------------------------------------------------- the committed fixture
STORED = ("A_mixed", "B", "B_list", "C")
LIST_NAMES = tuple("B_" + p for p in LIST_PLACES)
NAMES = STORED + LIST_NAMES


def _load(name):
    z_gold, ac.GOLD = ac.GOLD, GOLD
    try:
        return ac.load_batch(name)
    finally:
        ac.GOLD = z_gold


def _single_want(name):
    """single.npz: save_batch's layout without inputs, the answers under q2 = q, e2 = e of every recorded file's reads end to end in NAMES' order (its options are A_mixed's)."""
    m, at = meta()["batches"], 0
    for n in NAMES:
        k = 1 if n in LIST_NAMES else len(m[n]["names"])
        if n == name:
            return _load("single")[1][at:at + k]
        at += k


def load(name, single=False):
    """(batch, the reference's answers) of a recorded batch; single: under q2 = q, e2 = e (the same inputs).  The four list batches with a drop are stored as the one
    read in which they differ from B_list."""
    if name in LIST_NAMES:
        base, want = load("B_list", single)
        one, want1 = _load(name)
        return put(base, want, list_read(name[2:]), as_single(one) if single else one, _single_want(name) if single else want1)
    b, want = _load(name)
    return (as_single(b), _single_want(name)) if single else (b, want)


def meta():
    return json.load(open(os.path.join(GOLD, "meta.json")))


# ---------------------------------------------------------------- the reference's mm_align_skeleton on a crafted batch
OPT_KEYS = ("min_cnt", "bw_long", "zdrop", "zdrop_inv", "q", "e", "q2", "e2")       # what the families override


def ref_run(b):
    """The reference fed a batch's records and anchors as they are (no chaining of its own): per read (regs, aln, words).  align_cases.ref_align takes the reference's own
    pointers and frees them, so every read's records go into malloc'd memory as mm_reg1_t (80 bytes: the record's 72 and a null p) and its anchors into a malloc'd copy."""
    import ctypes as C
    ri = ac.RefIndex(b["refs"], "map-ont", **{k: getattr(b["opt"], k) for k in OPT_KEYS})
    try:
        assert all(getattr(ac.opt_from_ref(ri.mo), k) == getattr(b["opt"], k) for k, _ in mm.AlignOpt._fields_), "the options differ from the reference's"
        want = []
        for read, regs, a in zip(b["reads"], b["regs"], b["anchors"]):
            n = len(regs)
            raw = np.zeros((n, ac.REG1_BYTES), np.uint8)
            raw[:, :72] = np.ascontiguousarray(regs).view(np.uint8).reshape(n, 72)
            r_ptr = ac._libc.malloc(raw.nbytes)
            C.memmove(r_ptr, raw.ctypes.data, raw.nbytes)
            a = np.ascontiguousarray(a, np.uint64)
            a_ptr = ac._libc.malloc(a.nbytes)
            C.memmove(a_ptr, a.ctypes.data, a.nbytes)
            want.append(ac.ref_align(ri, read, r_ptr, n, a_ptr))
        return want
    finally:
        ri.close()


def host_single(b, threads=4):
    s = as_single(b)
    return mm.align_regs_extz_host(s["opt"], s["k"], s["hpc"], s["refs"], s["reads"], s["regs"], s["anchors"], threads=threads)


def gpu_single(eng, b):
    s = as_single(b)
    return eng.align_regs_extz(s["opt"], s["k"], s["hpc"], s["refs"], s["reads"], s["regs"], s["anchors"])
