"""The spliced alignment of hits on host threads (mm2gb_align_regs_splice_host, csrc/align_host.cpp) against the reference's mm_align_skeleton
under -x splice: the committed fixtures (tests/golden/splice), fresh random batches where oracle/_ref is built, each departure from the unspliced
path by name, the refusals, and the unspliced calls' own refusals of splice.  Every comparison is exact: the number and order of the records,
every field (trans_strand among them), every CIGAR word."""
import copy
import ctypes as C

import numpy as np
import pytest

import align_cases as ac
import mm2gb_amd as mm
import splice_cases as sc

NAMES = ["default", "hq", "for_only", "rev_only", "no_flank", "no_end_flt", "small_mat"]


@pytest.fixture(scope="module")
def golden():
    return {name: sc.load_batch(name) for name in sc.golden_names()}


@pytest.fixture(scope="module")
def host(golden):
    """The host form's answers on the fixture batches, computed once."""
    return {name: sc.run_host(golden[name][0], threads=8) for name in NAMES}


def with_opt(b, **kw):
    c = dict(b)
    c["opt"] = copy.deepcopy(b["opt"])
    for k, v in kw.items():
        setattr(c["opt"] if hasattr(c["opt"], k) else c["opt"].base, k, v)
    return c


def test_fixtures_reach_every_path():
    meta = sc.golden_meta()
    assert set(meta["batches"]) == set(NAMES) == set(sc.golden_names())
    missing = [k for k in sc.MUST_HAVE if not meta["total"].get(k)]
    assert not missing, missing
    for name, m in meta["batches"].items():          # only the batch made for it goes over max_sw_mat
        assert (m["splice_counts"]["over_sw_mat"] > 0) == (name == "small_mat"), name
    assert meta["batches"]["small_mat"]["options"]["max_sw_mat"] == 200_000 and meta["max_sw_mat"] == 100_000_000


def test_sizing_bound():
    """The 60 kb intron's read: were it one gap fill, the stretch would stay under max_sw_mat (genes() asserts the arithmetic); the read is in `default`."""
    refs, gs = sc.genes()
    assert sc.BIG_READ < 1500 and 2 * sc.BIG_READ * (2 * sc.BIG_READ + sc.BIG_INTRON) < sc.MAX_SW_MAT
    assert gs[0]["exons"][1][0] - gs[0]["exons"][0][1] == sc.BIG_INTRON
    assert refs == sc.load_genome()


@pytest.mark.parametrize("name", NAMES)
def test_host_equals_fixtures(golden, host, name):
    b, want, _ = golden[name]
    got, info = host[name]
    ac.assert_same(got, want, name)
    stored = sc.golden_meta()["batches"][name]
    assert info["splice_counts"] == stored["splice_counts"], "the paths taken differ from those recorded"
    assert info["counts"] == stored["counts"]
    assert info["counts"]["inv"] == 0 and info["counts"]["inv_probe_hit"] == 0          # mm_test_zdrop skips the inversion probe under MM_F_SPLICE
    assert all(not (r["flags"] & (1 << 24 | 1 << 11)).any() for r, _, _ in got)          # split_inv, inv


@pytest.mark.skipif(not ac.ref_available(), reason="the reference is not built here")
@pytest.mark.parametrize("name", NAMES)
def test_host_equals_live_reference(name):
    """300 fresh reads per option set on a fresh genome."""
    preset, kw = sc.OPTION_SETS[name]
    refs, reads = sc.random_batch(41 + NAMES.index(name), n_reads=300)
    b, want, _ = sc.ref_batch(refs, reads, preset, **kw)
    got, info = sc.run_host(b, threads=8)
    ac.assert_same(got, want, name)
    assert info["splice_counts"]["fill_intron"] > 100 and sum(len(w[0]) for w in want) >= 250


def test_defaults_are_the_presets(golden):
    """mm2gb_align_splice_opt_init against the values the reference's mm_set_opt left (stored with the fixtures), max_sw_mat aside: the preset's 0
    (no limit) is mm_mapopt_init's 100 000 000 here -- the stated departure."""
    for name, preset in (("default", "splice"), ("default", "cdna"), ("hq", "splice:hq")):
        o, ref = mm.align_splice_opt(preset), golden[name][2]
        assert ref["max_sw_mat"] == 0 and o.base.max_sw_mat == 100_000_000
        for k, _ in mm.AlignOpt._fields_:
            if k != "max_sw_mat":
                assert getattr(o.base, k) == ref[k], (preset, k)
        for k, _ in mm.AlignSpliceOpt._fields_[1:]:
            assert getattr(o, k) == ref[k], (preset, k)
        assert (ref["bw"], ref["bw_long"], ref["max_gap_ref"], ref["max_gap"]) == (200000, 200000, 200000, 2000)
    assert mm.preset("splice") == mm.preset("cdna") == mm.preset("splice:hq") == dict(k=15, w=5, hpc=False)
    with pytest.raises(mm.Mm2gbError, match="map-ont"):
        mm.align_splice_opt("map-ont")
    with pytest.raises(mm.Mm2gbError, match="no field"):
        mm.align_splice_opt("splice", nonsense=1)


def test_threads_give_identical_bytes(golden, host):
    one, _ = sc.run_host(golden["small_mat"][0], threads=1)
    for (r1, a1, w1), (r8, a8, w8) in zip(one, host["small_mat"][0]):
        assert r1.tobytes() == r8.tobytes() and a1.tobytes() == a8.tobytes() and w1.tobytes() == w8.tobytes()


def test_batch_schedule_gives_identical_bytes(golden, monkeypatch):
    """MM2GB_ALIGN_ROUNDS=batch: the device form's schedule (all reads in one sequence of rounds, both trials of a chain as jobs of one round, the
    second the first's twin) with the host DP behind it."""
    monkeypatch.setenv("MM2GB_ALIGN_ROUNDS", "batch")
    for name in ("small_mat", "rev_only"):
        b, want, _ = golden[name]
        got, info = sc.run_host(b, threads=8)
        ac.assert_same(got, want, name + ": batch schedule")
        assert info["splice_counts"] == sc.golden_meta()["batches"][name]["splice_counts"]


# ---------------------------------------------------------------- the departures from the unspliced path, one by one
def _names():
    return sc.default_names()


def test_two_strand_trial_keeps_the_larger_score(golden, host):
    """FOR and REV both set: per chain the record of the trial with the larger dp_score, trans_strand 1 / 2; checked against the single-trial
    batches on the reads all three batches share that have one record everywhere (no split changes the comparison)."""
    key = lambda b: {s: i for i, s in enumerate(b["reads"])}
    both, kb = host["default"][0], key(golden["default"][0])
    f, kf = host["for_only"][0], key(golden["for_only"][0])
    r, kr = host["rev_only"][0], key(golden["rev_only"][0])
    seen = set()
    for s in kf:
        gb, gf, gr = both[kb[s]], f[kf[s]], r[kr[s]]
        if not (len(gb[0]) == len(gf[0]) == len(gr[0]) == 1):
            continue
        sf, sr, ts = int(gf[1]["dp_score"][0]), int(gr[1]["dp_score"][0]), int(gb[1]["trans_strand"][0])
        assert int(gf[1]["trans_strand"][0]) == 1 and int(gr[1]["trans_strand"][0]) == 2          # the single-trial branch, align.c:1000
        assert ts == (1 if sf > sr else 2 if sf < sr else 3)
        kept = gf if sf > sr else gr if sf < sr else (gr if (len(s) + sf) & 1 else gf)                # a tie: trial (qlen + dp_score) & 1
        same = [k for k in mm.REG_DTYPE.names if k != "hash"]                                       # the hash is the read's place in its batch
        assert all(gb[0][k][0] == kept[0][k][0] for k in same) and gb[2].tobytes() == kept[2].tobytes() and int(gb[1]["dp_score"][0]) == max(sf, sr)
        seen.add((ts, (len(s) + sf) & 1 if ts == 3 else -1))
    assert seen == {(1, -1), (2, -1), (3, 0), (3, 1)}


def test_trans_strand_of_reverse_chains_is_the_trials(golden):
    """align.c:820-821 would flip trans_strand to the read's strand (^= 3) on a reverse-strand chain, but it tests a field that is set only after
    mm_align1 has returned: the reference never flips.  Decided by the recorded reference: with FOR alone every record carries 1 and with REV
    alone 2, reverse-strand chains among them (a flip would have made them 2 and 1); with both, reverse-strand chains carry 1, 2 and 3."""
    for name, ts in (("for_only", 1), ("rev_only", 2)):
        want = golden[name][1]
        got = [(bool(r["flags"][k] & (1 << 10)), int(a["trans_strand"][k])) for r, a, _ in want for k in range(len(r)) if a["cigar_off"][k] >= 0]
        assert sum(rev for rev, _ in got) >= 10 and {t for _, t in got} == {ts}, name
    want = golden["default"][1]
    assert {int(a["trans_strand"][k]) for r, a, _ in want for k in range(len(r)) if r["flags"][k] & (1 << 10) and a["cigar_off"][k] >= 0} == {1, 2, 3}


def test_end_filter(golden, host):
    """mm_fix_bad_ends_splice: with it a lone 15-mer across a long intron is left out of the alignment (the record starts / ends at the next exon);
    with MM_F_NO_END_FLT the intron is aligned.  Both as the reference has them (test_host_equals_fixtures)."""
    names = _names()
    on, off = host["default"], host["no_end_flt"]
    assert on[1]["splice_counts"]["end_flt_head"] > 0 and on[1]["splice_counts"]["end_flt_tail"] > 0 and on[1]["splice_counts"]["end_flt_probe_kept"] > 0
    assert off[1]["splice_counts"]["end_flt_head"] == off[1]["splice_counts"]["end_flt_tail"] == off[1]["splice_counts"]["end_flt_probe_kept"] == 0
    k_on = {s: i for i, s in enumerate(golden["default"][0]["reads"])}
    k_off = {s: i for i, s in enumerate(golden["no_end_flt"][0]["reads"])}
    lone = [golden["default"][0]["reads"][i] for i, n in enumerate(names) if n == "lone_end_kmer"]
    longer = 0
    for s in lone:
        a, c = on[0][k_on[s]], off[0][k_off[s]]
        span = lambda g: int(g[0]["re"][0] - g[0]["rs"][0])
        assert span(c) >= span(a)
        longer += span(c) > span(a) + 5000
    assert longer >= 4


def test_extensions_cross_introns(golden, host):
    names = _names()
    for what, first in (("left_ext_intron", True), ("right_ext_intron", False)):
        idx = [i for i, n in enumerate(names) if n == what]
        c, want = sc.sub_batch(golden["default"][0], golden["default"][1], idx)
        got, info = sc.run_host(c)
        ac.assert_same(got, want, what)
        assert info["splice_counts"][what] == len(idx) == 2
        for _, _, w in got:          # the intron is the second / the last but one word group of the record
            ops = [int(x) & 0xf for x in w]
            assert 3 in (ops[:12] if first else ops[-12:])


def test_split_tail_gets_its_own_trials(golden, host):
    got, info = host["default"]
    assert info["splice_counts"]["split"] >= 1 and info["splice_counts"]["tail_other_strand"] >= 1 and info["counts"]["rounds"] >= 2
    pairs = [(r, a) for r, a, _ in got if len(r) == 2 and (r["flags"][0] & (1 << 8)) and (r["flags"][1] & (1 << 9))]
    pairs += [(r[::-1], a[::-1]) for r, a, _ in got if len(r) == 2 and (r["flags"][1] & (1 << 8)) and (r["flags"][0] & (1 << 9))]
    assert any({int(a["trans_strand"][0]), int(a["trans_strand"][1])} == {1, 2} for _, a in pairs)


def test_seam_merges_two_introns(golden, host):
    names = _names()
    idx = [i for i, n in enumerate(names) if n == "seam"]
    c, want = sc.sub_batch(golden["default"][0], golden["default"][1], idx)
    got, info = sc.run_host(c)
    ac.assert_same(got, want, "seam")
    assert info["splice_counts"]["n_seam_merged"] >= 1
    assert any(mm.cigar_string(w) == f"{sc.SEAM_HALF}M{2000 + 100 * k}N{sc.SEAM_HALF}M" for k, (_, _, w) in enumerate(got))


def test_over_max_sw_mat_ends_the_chain(golden, host):
    """A stretch over max_sw_mat: the reset record with zdropped = 1 (mm_align_pair's rule), so the chain ends there and its tail is split off."""
    info = host["small_mat"][1]
    assert info["splice_counts"]["over_sw_mat"] > 0 and info["splice_counts"]["split"] > 0 and info["counts"]["over_sw_mat"] == info["splice_counts"]["over_sw_mat"]


# ---------------------------------------------------------------- refusals
def test_refusals(golden):
    b, _, _ = golden["for_only"]
    f = b["opt"].base.flag
    cases = [("lacks MM_F_SPLICE", with_opt(b, flag=f & ~(mm.F_SPLICE | mm.F_SPLICE_FOR | mm.F_SPLICE_REV))),
             ("MM_F_SR", with_opt(b, flag=f | mm.F_SR)), ("MM_F_QSTRAND", with_opt(b, flag=f | mm.F_QSTRAND)), ("MM_F_EQX", with_opt(b, flag=f | mm.F_EQX)),
             ("e must be above 0", with_opt(b, e=0)), ("max_sw_mat", with_opt(b, max_sw_mat=0)), ("max_sw_mat", with_opt(b, max_sw_mat=100_000_001)),
             ("0..127", with_opt(b, noncan=-1)), ("0..127", with_opt(b, junc_bonus=128)), ("0..127", with_opt(b, q2=200)), ("MM2GB_I_HPC", dict(b, hpc=True))]
    c = dict(b); c["regs"] = [x.copy() for x in b["regs"]]
    k = next(i for i, x in enumerate(c["regs"]) if len(x))
    c["regs"][k]["cnt"][0] = len(b["anchors"][k]) + 1
    cases.append(("leaves the read's anchors", c))
    c = dict(b); c["anchors"] = [x.copy() for x in b["anchors"]]
    c["anchors"][k][0, 1] |= np.uint64(1 << 48)
    cases.append(("multi-segment", c))
    for text, bad in cases:
        with pytest.raises(mm.Mm2gbError, match=text):
            sc.run_host(bad)
    with pytest.raises(mm.Mm2gbError, match="AlignSpliceOpt"):
        mm.align_regs_splice_host(b["opt"].base, b["k"], False, b["refs"], [], [], [])


def test_strand_flag_implies_splice(golden):
    """options.c:70-71: MM_F_SPLICE_FOR or _REV alone imply MM_F_SPLICE."""
    b, want, _ = golden["for_only"]
    c, w = sc.sub_batch(b, want, range(6))
    got, _ = sc.run_host(with_opt(c, flag=b["opt"].base.flag & ~mm.F_SPLICE))
    ac.assert_same(got, w, "FOR without SPLICE")


def test_refused_call_leaves_the_output_zeroed(golden):
    b, _, _ = golden["hq"]
    o = copy.deepcopy(b["opt"]); o.base.flag |= mm.F_SR
    out = mm._AlignOut()
    C.memset(C.byref(out), 0xff, C.sizeof(out))
    counts = (C.c_int64 * len(mm.SPLICE_COUNTS))(*([7] * len(mm.SPLICE_COUNTS)))
    fn = mm.lib().mm2gb_align_regs_splice_host
    fn.argtypes = None
    rc = fn(C.byref(o), C.c_int(15), C.c_int(0), C.c_int32(0), None, None, C.c_int64(0), None, None, None, None, None, None, C.c_int(1), C.byref(out), C.byref(counts))
    assert rc != 0 and bytes(out) == bytes(C.sizeof(out)) and not any(counts)


def test_edges(golden):
    b, want, _ = golden["hq"]
    got, info = mm.align_regs_splice_host(b["opt"], b["k"], False, b["refs"], [], [], [])
    assert got == [] and not any(info["splice_counts"].values())
    got, _ = mm.align_regs_splice_host(b["opt"], b["k"], False, b["refs"], b["reads"][:1], [np.zeros(0, mm.REG_DTYPE)], [np.zeros((0, 2), np.uint64)])
    assert len(got) == 1 and len(got[0][0]) == 0 and len(got[0][2]) == 0
    c, w = sc.sub_batch(b, want, [3])
    got, _ = sc.run_host(c)
    ac.assert_same(got, w, "one read")


def test_unspliced_calls_still_refuse_splice(golden):
    """The switch from the other side: the calls without _splice refuse MM_F_SPLICE by name and max_sw_mat = 0, with or without the preset's numbers."""
    b, _, _ = golden["hq"]
    args = (b["k"], False, b["refs"], b["reads"][:2], b["regs"][:2], b["anchors"][:2])
    with pytest.raises(mm.Mm2gbError, match="MM_F_SPLICE"):
        mm.align_regs_host(b["opt"].base, *args)
    with pytest.raises(mm.Mm2gbError, match="MM_F_SPLICE"):
        mm.align_regs_host(mm.align_opt("map-ont", flag=mm.F_SPLICE), *args)
    with pytest.raises(mm.Mm2gbError, match="max_sw_mat"):
        mm.align_regs_host(mm.align_opt("map-ont", max_sw_mat=0), *args)
    got, _ = mm.align_regs_host(mm.align_opt("map-ont"), *args)          # ... and still align unspliced: no N, no trans_strand
    assert all((a["trans_strand"] == 0).all() and not ((w & 0xf) == 3).any() for _, a, w in got)
