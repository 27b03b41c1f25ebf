"""Short single-end reads (minimap2 -x sr), what needs no device: the option sets, the heap order of seed collection (mm2gb_collect_seeds_heap_host, map.c:229-293) against what the
reference program printed for tests/golden/sr (tests/tools/gen_golden_sr.py) and against a plain-Python restatement on crafted matches, and the alignment of hits under MM_F_SR
(mm2gb_align_regs_sr_host) against what the reference's mm_align_skeleton returned.  Every comparison is exact.  (The mapper chains on the device: its PAFs are in tests/test_gpu_sr.py.)"""
import os

import numpy as np
import pytest

import align_cases as ac
import sr_cases as sc

mm = pytest.importorskip("mm2gb_amd")
HEAP_FLAG = mm.F_SR | mm.F_FRAG_MODE | mm.F_NO_PRINT_2ND | mm.F_HEAP_SORT


@pytest.fixture(scope="module")
def fixture_matches():
    return sc.matches([s for _, s in sc.reads()])


def test_options_equal_the_recorded_ones():
    want, got = sc.gold()["options"], sc.own_options()
    assert got["map"] == want["map"] and got["index"] == want["index"]
    assert mm.map_opt_sr().flag == HEAP_FLAG and mm.map_opt_sr().max_chain_skip == 2**31 - 1
    assert mm.preset_sr() == dict(k=21, w=11, hpc=False)
    # what mm2gb_map_opt_t has no room for: mm2gb_map_sr_t carries it
    assert want["ref_only"] == dict(max_occ=5000, max_frag_len=800, a=2, b=8, q=12, e=2, q2=24, e2=1, zdrop=100, zdrop_inv=100, end_bonus=10, min_dp_max=40)
    a = mm.map_sr()
    assert (a.max_occ, a.max_frag_len, a.align, a.what) == (5000, 800, 0, 0)
    assert {k: getattr(a.opt, k) for k in ("a", "b", "q", "e", "q2", "e2", "zdrop", "zdrop_inv", "end_bonus", "min_dp_max")} == {k: v for k, v in want["ref_only"].items() if k not in ("max_occ", "max_frag_len")}
    assert mm.map_sr(max_occ=50).max_occ == 50 and mm.map_sr(zdrop=60).opt.zdrop == 60
    o = mm.align_sr_opt()
    assert {k: getattr(o, k) for k in want["ref_only"] if hasattr(o, k)} == {k: v for k, v in want["ref_only"].items() if k not in ("max_occ", "max_frag_len")}
    assert (o.flag, o.bw, o.bw_long, o.max_gap, o.min_cnt, o.min_chain_score) == (HEAP_FLAG, 100, 100, 100, 2, 25) and bytes(o) == bytes(a.opt)
    assert mm.map_opt_sr(best_n=3).best_n == 3
    with pytest.raises(mm.Mm2gbError, match="no field"):
        mm.map_opt_sr(max_occ=5000)


def test_heap_order_equals_the_recorded_sd_lines(fixture_matches):
    rec = sc.gold()["seeds"]
    got, n_tied = mm.collect_seeds_heap_host(HEAP_FLAG, fixture_matches)
    names = [n for n, _ in sc.reads()]
    assert len(got) == len(names) == 209
    for n, a, m in zip(names, got, fixture_matches):
        assert sc.sd_rows(a) == rec[n]["sd"], n
        assert m["rep_len"] == rec[n]["rep_len"], n
    shared = [n for n, m in zip(names, fixture_matches) if sc.has_equal_cr(m)]
    assert n_tied == len(shared) and 3 <= n_tied <= len(names) // 2
    assert any(not rec[n]["sd"] for n in names) and any(len({r[0] for r in rec[n]["sd"]}) == 2 for n in names)


def test_the_heaps_tie_order_is_not_the_seed_order(fixture_matches):
    """Why a tied read goes back to the host form: sorted by (cr, seed, k) -- the device's order -- at least one fixture read differs from the recording."""
    rec, differs = sc.gold()["seeds"], 0
    for (n, _), m in zip(sc.reads(), fixture_matches):
        a = sc.heap_literal(m)
        assert sc.sd_rows(a) == rec[n]["sd"], n
        if not sc.has_equal_cr(m):
            continue
        h = np.asarray(m["hits"], np.uint64)
        owner = np.repeat(np.arange(len(m["seeds"])), np.asarray(m["seeds"])[:, 0].astype(int))
        qpos = np.asarray(m["seeds"])[:, 1].astype(np.int64)
        order = np.lexsort((np.arange(len(h)), h))
        same = (h[order] & np.uint64(1)).astype(np.int64) == (qpos[owner[order]] & 1)
        plain = [int(qpos[owner[i]] >> 1) for i in order[same]]
        differs += plain != [r[2] for r in rec[n]["sd"] if r[0] == 0]
    assert differs >= 1


@pytest.mark.parametrize("flag", [0, 0x100000, 0x200000], ids=["both", "for_only", "rev_only"])
def test_crafted_reads_equal_the_literal(flag):
    cases = sc.crafted_reads(np.random.default_rng(7))
    got, n_tied = mm.collect_seeds_heap_host(flag, list(cases.values()), threads=3)
    for (name, rd), a in zip(cases.items(), got):
        assert np.array_equal(a, sc.heap_literal(rd, flag)), name
    assert n_tied == sum(sc.has_equal_cr(rd) for rd in cases.values()) == 3
    assert len(got[0]) == 0 and len(got[1]) == (0 if flag == 0x200000 else 1)
    if flag == 0:
        assert [len(a) for a in got][4:7] == [sc.WAVE_HITS - 1, sc.WAVE_HITS, sc.WAVE_HITS + 1]


def test_name_tests_run_in_heap_order():
    """MM_F_NO_DIAG / MM_F_NO_DUAL (skip_seed is shared with the sorted form): diagonal hits dropped, MM_SEED_SELF set, a larger-named read's hits dropped."""
    five = [sc.hit(p) for p in (40, 90, 150, 2_000, 2_060)]
    rd = sc.read_of([sc.seed(5, 40), sc.seed(5, 90), sc.seed(2, 170, 1)], [five, five, [sc.hit(1_000), sc.hit(170, 1)]], 250)
    ref_len, ref_rank = [250], [1]
    for q_rank, flag in ((1, mm.F_NO_DIAG), (1, mm.F_NO_DIAG | mm.F_NO_DUAL), (2, mm.F_NO_DUAL), (0, mm.F_NO_DUAL)):
        r = dict(rd, q_rank=q_rank)
        got, _ = mm.collect_seeds_heap_host(flag, [r], ref_len=ref_len, ref_rank=ref_rank)
        want = sc.heap_literal(r, flag, ref_len, ref_rank)
        assert np.array_equal(got[0], want), (q_rank, flag)
        if flag & mm.F_NO_DIAG:
            assert len(want) == 12 - 3 and (want[:, 1] >> np.uint64(43) & np.uint64(1)).sum() > 0
        elif q_rank == 2:
            assert len(want) == 0


def test_the_new_calls_refuse_by_name():
    rd = sc.read_of([sc.seed(1, 40)], [[sc.hit(5_000)]], 100)
    with pytest.raises(mm.Mm2gbError, match="MM_F_QSTRAND is not supported"):
        mm.collect_seeds_heap_host(0x100000000, [rd])
    bad = dict(rd, seeds=np.asarray([sc.seed(2, 40)], np.uint32))
    bad["hits"] = np.asarray([sc.hit(5_000)], np.uint64)
    L = mm.lib()
    off2, off1 = np.asarray([0, 1], np.int64), np.asarray([0, 1], np.int64)
    a_off, out, ql = np.zeros(2, np.int64), np.zeros((2, 2), np.uint64), np.asarray([100], np.int32)
    L.mm2gb_collect_seeds_heap_host.argtypes = None
    import ctypes as C
    rc = L.mm2gb_collect_seeds_heap_host(C.c_int64(0), C.c_int64(1), C.c_void_p(off2.ctypes.data), C.c_void_p(bad["seeds"].ctypes.data), C.c_void_p(off1.ctypes.data),
                                         C.c_void_p(bad["hits"].ctypes.data), C.c_void_p(ql.ctypes.data), None, C.c_int32(0), None, None, C.c_int(1), C.c_void_p(a_off.ctypes.data),
                                         C.c_void_p(out.ctypes.data), None)
    assert rc == -1 and b"hit_off does not match" in L.mm2gb_last_error()
    with pytest.raises(mm.Mm2gbError, match="NO_DIAG / NO_DUAL need ref_rank"):
        mm.collect_seeds_heap_host(mm.F_NO_DUAL, [dict(rd, q_rank=1)])


def test_the_existing_calls_keep_their_refusals():
    with pytest.raises(mm.Mm2gbError, match="not supported"):
        mm.map_opt_preset("sr")
    with pytest.raises(mm.Mm2gbError):
        mm.align_opt("sr")


def test_alignment_equals_the_recorded_records_and_words():
    """mm2gb_align_regs_sr_host on the fixture's records and anchors: every record, mm_extra_t row and CIGAR word as mm_align_skeleton left them -- the reads with a
    substituted middle split their chain, most chains' stretch is shorter than the chain -- at 1 and 5 threads, and in the device form's schedule with the host DP behind it."""
    batch, want = sc.golden_aligned()
    for threads in (1, 5):
        got, info = sc.run_sr_host(batch, threads=threads)
        ac.assert_same(got, want, f"{threads} threads")
    assert info["sr_counts"] == dict(fill_ungapped=info["counts"]["fill_one_pass"], fill_rerun=info["counts"]["fill_two_pass"], stretch_short=info["sr_counts"]["stretch_short"])
    assert info["sr_counts"]["fill_rerun"] >= 2 and info["counts"]["split"] >= 2 and info["sr_counts"]["stretch_short"] >= 1 and info["counts"]["dp_max_rewritten"] == 0
    names = [n for n, _ in sc.reads()]
    assert sum(n.startswith("drop") and (r["flags"] & (1 << 8)).any() for n, (r, _, _) in zip(names, want)) >= 2
    os.environ["MM2GB_ALIGN_ROUNDS"] = "batch"
    try:
        got2, info2 = sc.run_sr_host(batch)
    finally:
        del os.environ["MM2GB_ALIGN_ROUNDS"]
    ac.assert_same(got2, want, "batch schedule")
    assert info2["sr_counts"] == info["sr_counts"]


def test_crafted_chains_on_the_host():
    """The crafted single-chain batch of tests/test_gpu_sr.py, what its cases are built to show: a drop of exactly zdrop stays ungapped, zdrop + 1 runs again."""
    cases = sc.ungapped_cases(np.random.default_rng(11))
    got, info = sc.run_sr_host(sc.ungapped_batch(cases))
    words = {n: mm.cigar_string(w) for n, (_, _, w) in zip(cases, got)}
    assert words["len1"] == "61M" and words["len1000"] == "1060M" and words["drop_100"] == "210M" and words["drop_101"] != "210M"
    assert info["sr_counts"] == dict(fill_ungapped=13, fill_rerun=4, stretch_short=0)
    score = {n: int(a["dp_score"][0]) for n, (_, a, _) in zip(cases, got)}
    assert score["n_query"] == 2 * 157 + 3 * 1 and score["n_target"] == 2 * 154 + 6 * 1            # + e2 per ambiguous column (align.c:748), not -sc_ambi


def test_the_alignment_calls_refuse_by_name():
    batch, _ = sc.golden_aligned()
    few = {k: (v[:3] if k in ("reads", "regs", "anchors") else v) for k, v in batch.items()}
    go = lambda fn, **kw: fn(kw.get("opt", few["opt"]), few["k"], kw.get("hpc", False), few["refs"], few["reads"], few["regs"], few["anchors"])
    with pytest.raises(mm.Mm2gbError, match="lacks MM_F_SR"):
        go(mm.align_regs_sr_host, opt=mm.align_sr_opt(flag=0))
    with pytest.raises(mm.Mm2gbError, match="MM2GB_I_HPC"):
        go(mm.align_regs_sr_host, hpc=True)
    for bit, name in ((0x100000000, "MM_F_QSTRAND"), (0x4000000, "MM_F_EQX"), (0x80, "MM_F_SPLICE")):
        with pytest.raises(mm.Mm2gbError, match=name):
            go(mm.align_regs_sr_host, opt=mm.align_sr_opt(flag=HEAP_FLAG | bit))
    with pytest.raises(mm.Mm2gbError, match="q == q2"):
        go(mm.align_regs_sr_host, opt=mm.align_sr_opt(q2=12, e2=2))
    # anchors that do not lie on one diagonal in ascending order: the reference asserts (align.c:745)
    t, q, reg, a = sc.chain_case(np.random.default_rng(3), 300)
    a = np.asarray([[int(a[1][0]), 20 << 32 | int(a[1][1]) & 0xffffffff], [int(a[1][0]) - 100, 20 << 32 | (int(a[1][1]) & 0xffffffff) - 100]], np.uint64)
    with pytest.raises(mm.Mm2gbError, match="differ in length|leaves its sequence"):
        mm.align_regs_sr_host(mm.align_sr_opt(min_cnt=1), 21, False, [t], [q], [reg], [a])
    # the existing calls keep refusing the bit
    for fn in (mm.align_regs_host, mm.align_regs_extz_host):
        with pytest.raises(mm.Mm2gbError, match="MM_F_SR is not supported"):
            go(fn, opt=mm.align_opt("map-ont", flag=mm.F_SR) if fn is mm.align_regs_host else mm.align_opt("map-ont", q2=4, e2=2, flag=mm.F_SR))
    with pytest.raises(mm.Mm2gbError, match="MM_F_SR is not supported"):
        go(mm.align_regs_splice_host, opt=mm.align_splice_opt(flag=0x80 | mm.F_SR))
    with pytest.raises(mm.Mm2gbError, match="no field"):
        mm.align_sr_opt(max_occ=1)
    with pytest.raises(mm.Mm2gbError, match="no field"):
        mm.map_sr(best_n=3)


def fresh_reads(seed):
    rng = np.random.default_rng(seed)
    g = np.frombuffer(sc.gold()["genome"].encode(), np.uint8)
    reads = []
    for r in range(300):
        n = int(rng.integers(100, 251))
        st = sc.TANDEM[0] + int(rng.integers(0, 1_300)) if r % 3 == 0 else int(rng.integers(0, len(g) - n))
        s = sc.sim_reads.mutate(rng, g[st:st + n], float(rng.uniform(0.005, 0.02)))
        if r % 10 == 4:                  # a stretch of substituted bases: fills that drop
            s = s.copy(); m = len(s) // 2; s[m - 15:m + 15] = sc._other(np.where(s[m - 15:m + 15] == ord("N"), ord("A"), s[m - 15:m + 15]))
        reads.append((f"fresh{r}", (sc.sim_reads.revcomp(s) if rng.random() < 0.5 else s).tobytes()))
    return reads


@pytest.mark.skipif(not ac.ref_available(), reason="the reference library is built only where its checkout exists")
def test_fresh_reads_through_mm_align_skeleton():
    """300 fresh reads of 100-250 bases, a third from the tandem array, a tenth with 30 substituted bases in the middle: every read's records, rows and words equal
    mm_align_skeleton's; none is left out."""
    reads = fresh_reads(2026)
    batch, want = sc.sr_ref_batch(sc.gold()["genome"].encode(), [s for _, s in reads])
    got, info = sc.run_sr_host(batch)
    ac.assert_same(got, want, "fresh reads")
    assert len(want) == 300 and sum(len(w[0]) > 0 for w in want) >= 250 and info["sr_counts"]["fill_rerun"] >= 5 and info["sr_counts"]["fill_ungapped"] >= 250


@pytest.mark.skipif(not os.path.exists(sc.REF_EXE), reason="the reference program is built only where its checkout exists")
def test_fresh_reads_against_the_reference_program():
    """300 fresh reads of 100-250 bases, a third of them from the tandem array: every read's anchors equal the program's SD lines."""
    rng = np.random.default_rng(2024)
    g = np.frombuffer(sc.gold()["genome"].encode(), np.uint8)
    reads = []
    for r in range(300):
        n = int(rng.integers(100, 251))
        st = sc.TANDEM[0] + int(rng.integers(0, 1_300)) if r % 3 == 0 else int(rng.integers(0, len(g) - n))
        s = sc.sim_reads.mutate(rng, g[st:st + n], float(rng.uniform(0.005, 0.02)))
        reads.append((f"fresh{r}", (sc.sim_reads.revcomp(s) if rng.random() < 0.5 else s).tobytes()))
    rec = sc.record_seeds(sc.gold()["genome"].encode(), reads)
    m = sc.matches([s for _, s in reads])
    got, n_tied = mm.collect_seeds_heap_host(HEAP_FLAG, m)
    assert n_tied >= 50
    for (n, _), a, x in zip(reads, got, m):
        assert sc.sd_rows(a) == rec[n]["sd"] and x["rep_len"] == rec[n]["rep_len"], n
