"""The crafted chains of tests/align_crafted_cases.py on the host form (mm2gb_align_regs_host / _extz_host) against what the reference's mm_align_skeleton answered
when it was fed the same records and anchors (tests/golden/align_crafted), exactly; and, case by case, the counts that say the case still reaches the path it is built
for -- a slice cut of k_al_gather inside a job, a drop on either side of a threshold, the inversion probe on either side of its score.  tests/test_gpu_align_crafted.py
runs the same batches on the device."""
import numpy as np
import pytest

import align_cases as ac
import align_crafted_cases as cc
import mm2gb_amd as mm

KEEP = cc.KEEP


@pytest.fixture(scope="module")
def golden():
    return {(name, single): cc.load(name, single) for name in cc.NAMES for single in (False, True)}


def run(b, single, threads=4):
    return cc.host_single(b, threads) if single else ac.run_host(b, threads)


def nonzero(counts):
    return {k: counts[k] for k in KEEP if counts[k]}


def test_the_fixture_is_what_the_builder_makes(golden):
    """Inputs byte for byte: a change to the builder that is not recorded again fails here, not as a puzzling difference in a word."""
    made = dict(cc.all_batches(), **{"B_" + p: cc.list_batch(p) for p in cc.LIST_PLACES})
    assert set(made) == set(cc.NAMES)
    for name, (b, names) in made.items():
        g, _ = golden[name, False]
        assert names == cc.meta()["batches"][name]["names"]
        assert g["refs"] == b["refs"] and g["reads"] == b["reads"], name
        assert all(x.tobytes() == y.tobytes() for x, y in zip(g["regs"], b["regs"])) and all(x.tobytes() == np.asarray(y).tobytes() for x, y in zip(g["anchors"], b["anchors"])), name
        assert all(getattr(g["opt"], k) == getattr(b["opt"], k) for k, _ in mm.AlignOpt._fields_), name


@pytest.mark.parametrize("single", [False, True], ids=["dual", "single"])
@pytest.mark.parametrize("name", cc.NAMES)
def test_host_equals_fixture(golden, name, single):
    b, want = golden[name, single]
    got, info = run(b, single)
    ac.assert_same(got, want, name)
    stored = cc.meta()["batches"][name]["counts_single" if single else "counts"]
    assert {k: info["counts"][k] for k in KEEP} == stored, "the paths taken differ from those recorded"


def test_batch_schedule_gives_identical_bytes(golden, monkeypatch):
    """MM2GB_ALIGN_ROUNDS=batch: the device form's schedule with the host DP behind it."""
    monkeypatch.setenv("MM2GB_ALIGN_ROUNDS", "batch")
    for (name, single), (b, want) in golden.items():
        got, info = run(b, single, threads=8)
        ac.assert_same(got, want, name + ": batch schedule")
        assert info["counts"]["rounds"] == cc.meta()["batches"][name]["counts_single" if single else "counts"]["rounds"]


# ---------------------------------------------------------------- what each case is built for
def job_lengths(b, i):
    """The jobs of read i's chain as csrc/align_host.cpp plans them from two anchors without HPC: the fill between the anchors' ends (query, target), the query bases
    before the first and behind the last."""
    a, qn = b["anchors"][i], len(b["reads"][i])
    x, y = (a[:, 0] & np.uint64(0xffffffff)).astype(np.int64), (a[:, 1] & np.uint64(0xffffffff)).astype(np.int64)
    return (int(y[-1] - y[0]), int(x[-1] - x[0])), int(y[0]) + 1, qn - int(y[-1]) - 1


def slices(n):
    return -(-n // cc.SLICE)


def test_seam_cases_cross_the_cuts_they_are_built_for(golden):
    """k_al_gather writes a job AL_SLICE = 4096 bytes of either side per workgroup (its comment: 4 KiB); the constant is read from the source, no call exposes it."""
    assert cc.al_slice() == cc.SLICE == 4096
    b, _ = golden["A_mixed", False]
    names = cc.meta()["batches"]["A_mixed"]["names"]
    seen = set()
    for i, n in enumerate(names):
        (fq, ft), lead, tail = job_lengths(b, i)
        rev = bool(b["regs"][i]["flags"][0] & cc.RF_REV)
        assert rev == n.endswith("_rev")
        assert bool(int(b["anchors"][i][0, 0]) >> 63) == rev
        base = n[:-4] if n.endswith("_rev") else n
        if base.startswith("fill"):
            want = int(base[4:])
            assert (fq, ft) == (want, want), n
            assert slices(want) == {4095: 1, 4096: 1, 4097: 2, 8191: 2, 8193: 3}[want]
        elif base == "q4097_t3000":
            assert (fq, ft) == (4097, 3000) and slices(fq) == 2 and slices(ft) == 1
        elif base == "t4097_q3000":
            assert (fq, ft) == (3000, 4097) and slices(fq) == 1 and slices(ft) == 2
        elif base == "left4500":
            assert lead == 4499 and slices(lead) == 2          # (a removed query base: 4500 columns, 4499 bytes)
        elif base == "right4500":
            assert tail == 4499 and slices(tail) == 2
        else:
            assert base.startswith("tiny") and fq == ft and fq % 16 != 0 and fq < 64
        seen.add((base, rev) if not base.startswith("tiny") else ("tiny", False))
    forms = ["fill%d" % n for n in cc.A_FILLS] + ["q4097_t3000", "t4097_q3000", "left4500", "right4500"]
    assert seen == {(f, r) for f in forms for r in (False, True)} | {("tiny", False)}
    assert sum(n.startswith("tiny") for n in names) == 30 and len({job_lengths(b, i)[0][0] % 16 for i, n in enumerate(names) if n.startswith("tiny")}) == 15


def built_for(name, single=False):
    """The counts a case must show when it runs alone.  A and B are built for either scoring; C's block lengths are found under the dual-affine first pass, whose words the
    walk follows -- under q2 = q, e2 = e the words differ, and C is held to its recorded counts alone."""
    if single and name.startswith(("pin_", "inv_")):
        return {}
    rev = int(name.endswith("_rev"))
    base = name[:-4] if rev else name
    one = dict(fill_one_pass=1, fill_two_pass=0, split=0, rounds=1, rev_chain=rev, jobs=3)
    if base.startswith("fill") or base.startswith("tiny"):
        return one
    if base in ("q4097_t3000", "t4097_q3000"):                     # 1097 bases are more than the band of 751 crosses: the fill ends in a drop and the chain splits
        return dict(fill_one_pass=1, fill_two_pass=0, split=1, rounds=2, rev_chain=2 * rev)
    if base == "left4500":
        return dict(one, left_at_0=1, left_short=1)
    if base == "right4500":
        return dict(one, right_short=1)
    if base in cc.B_STAYS:
        return dict(fill_one_pass=2, fill_two_pass=0, split=0, inv_probe_hit=0, rounds=1, rev_chain=rev, jobs=4)
    if base in cc.B_DROPS:
        return dict(fill_one_pass=1, fill_two_pass=1, split=1, inv_probe_hit=0, rounds=2, rev_chain=2 * rev)
    if base.startswith("pin_"):                                     # a probe of exactly 80: a hit and the split (39 or 40 bases are too few for a record of their own)
        return dict(inv_probe_hit=1, fill_two_pass=1, split=1, inv=0, rounds=2)
    assert base.startswith("inv_")
    _, where, n = base.split("_")
    hit = cc.C_HITS[where][int(n) - cc.C_FLIP[where] + 1]
    if where == "mid":                                              # a hit splits the chain and the inverted block is aligned in a third round
        return dict(inv_probe_hit=hit, fill_two_pass=hit, split=hit, inv=hit, rounds=3 if hit else 1)
    return dict(inv_probe_hit=hit, fill_two_pass=hit, rounds=1)    # at the edge the second pass under zdrop_inv still reaches the fill's end


@pytest.mark.parametrize("name", ["A_mixed", "B", "C"])
def test_every_case_alone_reaches_its_path(golden, name):
    m = cc.meta()["batches"][name]
    for single in (False, True):
        b, want = golden[name, single]
        for i, n in enumerate(m["names"]):
            one, w = cc.pick(b, want, [i])
            got, info = run(one, single, threads=1)
            ac.assert_same(got, w, n + ": alone")
            for k, v in built_for(n, single).items():
                assert info["counts"][k] == v, f"{n} ({'single' if single else 'dual'}): {k} is {info['counts'][k]}, the case is built for {v}"
            stored = m["alone"][n][1] if single and m["alone"][n][1] is not None else m["alone"][n][0]
            assert nonzero(info["counts"]) == stored, n


def test_thresholds_lie_between_the_pairs():
    """Every pair of B differs by one N-column, a drop of zdrop and of zdrop + 1; the probe's triples are n - 1, n, n + 1 around the first hit."""
    assert len(cc.B_STAYS) == len(cc.B_DROPS) and all(s.rsplit("_", 1)[0] == d.rsplit("_", 1)[0] or (s, d) in (("mm20", "mm20_n1"), ("mm19_n4", "mm19_n5")) for s, d in zip(cc.B_STAYS, cc.B_DROPS))
    names = cc.meta()["batches"]["B"]["names"]
    assert set(names) == {n + s for n in cc.B_STAYS + cc.B_DROPS for s in ("", "_rev")}
    for where in ("mid", "edge"):
        assert cc.C_HITS[where][:2] == (0, 1)
    pins = {f"pin_{k}_{sd}_{n}{s}" for k, sd, n in cc.PINS for s in ("", "_rev")}
    assert set(cc.meta()["batches"]["C"]["names"]) == pins | {f"inv_{w}_{cc.C_FLIP[w] + d}{s}" for w in ("mid", "edge") for d in (-1, 0, 1) for s in ("", "_rev")}


def test_the_dropping_fill_lies_where_the_list_batch_says(golden):
    """k_al_zdrop's list is the round's gap fills by qlen + tlen, longest first: 132 of them, all different, and the one fill whose two sides differ is at position
    0, 63, 64 and 131 -- the first and last lane of the first workgroup, the first lane of the second, the last entry."""
    for place, want in cc.LIST_PLACES.items():
        b, _ = golden["B_" + place, False]
        fills = []
        for read, ref, a, g in zip(b["reads"], b["refs"], b["anchors"], b["regs"]):
            q, t = np.frombuffer(read, np.uint8), np.frombuffer(ref, np.uint8)
            if g["flags"][0] & cc.RF_REV:
                q = cc.revcomp(q)
            x, y = (a[:, 0] & np.uint64(0xffffffff)).astype(np.int64) + 1, (a[:, 1] & np.uint64(0xffffffff)).astype(np.int64) + 1
            for k in range(1, len(a)):
                fq, ft = q[y[k - 1]:y[k]], t[x[k - 1]:x[k]]
                fills.append((len(fq) + len(ft), len(fq) != len(ft) or bool((fq != ft).any())))
        assert len(fills) == cc.N_FILLS >= 130 and len({n for n, _ in fills}) == len(fills) and all(n >= 400 for n, _ in fills)
        fills.sort(reverse=True)
        assert [i for i, (_, edited) in enumerate(fills) if edited] == [want], place


def test_the_deletion_pair_needs_the_walks_gap_terms(golden):
    """del3_80 / del3_81 by the walk's own arithmetic (align.c:32-68) on the fill's recorded words: 80 and 81 as they are; 24 more without - diff * e; 100 and 101 with
    e = 0 throughout (the maximum then moves behind the gap) -- either mistake makes del3_80 drop, which the counts above forbid."""
    b, want = golden["B", False]
    names = cc.meta()["batches"]["B"]["names"]
    for n, z in (("del3_80", 80), ("del3_80_rev", 80)):
        i = names.index(n)
        words = want[i][2]
        assert mm.cigar_string(words) == "530M3D327M"               # 30 + 400 + 100 columns, the three removed bases, the rest: one record
        t = np.frombuffer(b["refs"][i], np.uint8)[cc.REF_LEAD + 430:cc.REF_LEAD + 830]
        q = np.frombuffer(b["reads"][i], np.uint8)
        q = (cc.revcomp(q) if n.endswith("_rev") else q)[430:827]
        fill = [100 << 4, 3 << 4 | 2, 297 << 4]

        def walk(e_gap, e_diff):
            score, top, at, worst, i_, j_ = 0, None, (0, 0), 0, 0, 0
            def see(ti, qj):
                nonlocal top, at, worst
                if top is not None and score < top:
                    worst = max(worst, top - score - abs((ti - at[0]) - (qj - at[1])) * e_diff)
                else:
                    top, at = score, (ti, qj)
            for w in fill:
                op, ln = w & 15, w >> 4
                if op == 0:
                    for l in range(ln):
                        tc, qc = t[i_ + l], q[j_ + l]
                        score += -1 if ord("N") in (tc, qc) else 2 if tc == qc else -4
                        see(i_ + l, j_ + l)
                    i_ += ln; j_ += ln
                else:
                    score -= 40 + e_gap * ln
                    i_ += ln
                    see(i_, j_)
            return worst
        assert (walk(8, 8), walk(8, 0), walk(0, 0)) == (z, z + 24, z + 20)


@pytest.mark.skipif(not ac.ref_available(), reason="the reference is not built here")
@pytest.mark.parametrize("name", cc.NAMES)
def test_fixture_equals_live_reference(golden, name):
    for single in (False, True):
        b, want = golden[name, single]
        ac.assert_same(cc.ref_run(b), want, name + ": the reference, live")
