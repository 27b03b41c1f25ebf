"""Read-against-read overlap without a GPU: the option sets of ava-ont / ava-pb against the recorded ones and mm_set_opt, the names that stay refused,
the calls with base-level alignment refusing the overlap bits by name, what the recorded runs must contain, and mm_est_err's walk on host threads
(mm2gb_est_err_host) against esterr.c written out in Python.  The mapper itself needs a device: its PAFs are compared in tests/test_gpu_ava.py."""
import types

import numpy as np
import pytest

import align_cases as ac
import ava_cases as av
import mm2gb_amd as mm

needs_ref = pytest.mark.skipif(not ac.ref_available(), reason="the reference build (oracle/_ref) is not here")


@pytest.mark.parametrize("name", ["ava-ont", "ava-pb"])
def test_options_equal_the_recorded_ones(name):
    assert av.own_options(name) == av.gold()["options"][name]


@needs_ref
@pytest.mark.parametrize("name", ["ava-ont", "ava-pb"])
def test_options_equal_mm_set_opt(name):
    assert av.own_options(name) == av.ref_options(name)


def test_option_values_and_exported_bits():
    assert (mm.F_NO_DIAG, mm.F_NO_DUAL, mm.F_NO_LJOIN, mm.F_ALL_CHAINS) == (0x001, 0x002, 0x400, 0x800000)
    base = mm.map_opt()
    for name in ("ava-ont", "ava-pb"):
        o = mm.map_opt_ava(name)
        assert o.flag == av.X_BITS and (o.min_chain_score, o.pri_ratio, o.occ_dist) == (100, 0.0, 0)
        assert o.max_chain_skip == base.max_chain_skip == av.INF and o.seeding_on_device == 0          # this project's default: exhaustive
    assert (mm.map_opt_ava("ava-ont").bw, mm.map_opt_ava("ava-ont").bw_long) == (2000, 2000)
    assert (mm.map_opt_ava("ava-pb").bw, mm.map_opt_ava("ava-pb").bw_long) == (base.bw, base.bw)
    assert mm.map_opt_ava("ava-ont", max_chain_skip=25, seeding_on_device=mm.SEEDING_RESIDENT).max_chain_skip == 25 and mm.SEEDING_RESIDENT == 2
    assert mm.preset_ava("ava-ont") == dict(k=15, w=5, hpc=False) and mm.preset_ava("ava-pb") == dict(k=19, w=5, hpc=True)
    with pytest.raises(mm.Mm2gbError, match="no field"):
        mm.map_opt_ava("ava-ont", bandwidth=3)


def test_the_old_names_stay_refused_and_the_new_calls_take_only_their_own():
    for name in ("ava-ont", "ava-pb"):
        with pytest.raises(mm.Mm2gbError, match="not supported"):
            mm.map_opt_preset(name)
        with pytest.raises(mm.Mm2gbError, match="not supported"):
            mm.preset(name)
    for name in ("map-ont", "ava", "asm5", ""):
        with pytest.raises(mm.Mm2gbError, match="ava-ont, ava-pb"):
            mm.map_opt_ava(name)
        with pytest.raises(mm.Mm2gbError, match="ava-ont, ava-pb"):
            mm.preset_ava(name)


@pytest.mark.parametrize("bit, name", [(mm.F_ALL_CHAINS, "MM_F_ALL_CHAINS"), (mm.F_NO_DIAG, "MM_F_NO_DIAG"), (mm.F_NO_DUAL, "MM_F_NO_DUAL")])
def test_calls_with_alignment_refuse_the_overlap_bits_by_name(bit, name):
    """The options are looked at before anything else: nothing runs, not even the look for an engine (the handle here is null)."""
    no_engine = types.SimpleNamespace(_h=None)
    refs = [b"ACGT" * 300]
    reads = [("q", b"ACGT" * 100)]
    with mm.SeedIndex(refs, k=15, w=10, threads=1) as ix:
        with pytest.raises(mm.Mm2gbError, match=f"mm2gb_map_reads_aln: {name} is not supported with base-level alignment"):
            mm.map_reads(no_engine, ix, ["t"], reads, opt=mm.map_opt(flag=bit | mm.F_NO_LJOIN), align=mm.map_align(refs))
        with pytest.raises(mm.Mm2gbError, match=f"mm2gb_map_reads_splice: {name} is not supported with base-level alignment"):
            mm.map_reads(no_engine, ix, ["t"], reads, opt=mm.map_opt_splice(flag=bit), align=mm.map_splice(refs))
        # MM_F_NO_LJOIN alone is no reason to refuse: the call gets as far as looking for its engine
        with pytest.raises(mm.Mm2gbError, match="null argument"):
            mm.map_reads(no_engine, ix, ["t"], reads, opt=mm.map_opt(flag=mm.F_NO_LJOIN), align=mm.map_align(refs))
        with pytest.raises(mm.Mm2gbError, match="null argument"):
            mm.map_reads(no_engine, ix, ["t"], reads, opt=mm.map_opt_ava("ava-ont"))


def test_the_fixture_holds_what_the_tests_rely_on():
    for skip in av.SKIPS:
        a = [ln.split("\t") for ln in av.golden_paf("a.ava-ont", skip).splitlines()]
        assert len(a) >= 100 and any(f[0] == f[5] for f in a) and sum(f[4] == "-" for f in a) >= 10
        assert {n for n, _ in av.read_set("a")} - {f[0] for f in a}                               # a read without a line
        assert all(f[11] == "0" and "tp:A:S" in f and not any(t.startswith("s2:") for t in f) for f in a)
    assert any(av.golden_paf(run, "s25") != av.golden_paf(run, "inf") for run in av.RUNS)         # the finite skip shows in the bytes


def test_name_traps_in_fixture():
    """Set c: what strcmp order, name equality and the length test decide shows in the recorded lines."""
    names_t = [n for n, _ in av.read_set("ct")]
    assert names_t.count("dup") == 2 and any(max(n.encode()) >= 0x80 for n in names_t)
    for kind in ("ava-ont", "X"):
        c = [ln.split("\t") for ln in av.golden_paf(f"c.{kind}", "inf").splitlines()]
        pairs = {(f[0], f[5]) for f in c}
        assert all(q.encode() <= t.encode() for q, t in pairs)                                     # every pair once, the smaller name as query
        assert ("r1", "r10") in pairs and ("read10", "read9") not in pairs                          # a prefix is smaller; "read10" < "read9"
        assert any(q != "ré" and t == "ré" for q, t in pairs)                                      # bytes compare as unsigned: ASCII < 0xc3
        assert any(f[0] == f[5] == "dup" and f[1] != f[6] and f[2] == f[7] for f in c)             # on the diagonal, kept because the lengths differ
        same = [f for f in c if f[0] == f[5] == "same"]
        assert all(f[1] == f[6] for f in same)                                                     # two different reads, one name, one length


# ---------------------------------------------------------------- mm_est_err's walk on host threads
def check_against_literal(got, reads, ref_len):
    for r, rd in enumerate(reads):
        want, sum_k = av.est_err_literal(rd, ref_len)
        assert got[r]["sum_k"] == sum_k, r
        assert [tuple(v) for v in zip(got[r]["n_match"].tolist(), got[r]["n_tot"].tolist())] == want, r
        for (n_match, n_tot), div in zip(want, got[r]["div"]):
            if n_tot < 0:
                assert div == np.float32(-1.0)
            else:
                avg_k = np.float32(sum_k) / np.float32(len(rd["mini_pos"]))
                assert div == (np.float32(0.0) if n_match >= n_tot else np.float32(1.0 - (n_match / n_tot) ** (1.0 / float(avg_k))))


def test_est_err_host_crafted():
    reads, ref_len, what = av.crafted_reads()
    got = mm.est_err_host(reads, ref_len, threads=3)
    check_against_literal(got, reads, ref_len)
    by = dict(zip(what, got))
    fr = by["forward and reverse"]
    assert fr["n_match"][0] == fr["n_match"][1] == 13 and fr["n_tot"][0] == fr["n_tot"][1] == 37 + 2 and 0 < fr["div"][0] == fr["div"][1] < 1
    assert by["cnt 1 and cnt 0"]["n_match"].tolist() == [1, 0] and by["cnt 1 and cnt 0"]["n_tot"].tolist() == [3, -1]
    assert by["no end increment"]["n_tot"][0] == len(reads[2]["mini_pos"]) - 1 and by["no end increment"]["n_match"][0] == 26
    assert by["first anchor absent"]["n_tot"][0] == -1 and by["first anchor absent"]["div"][0] == -1
    assert by["walk ends at j == n"]["n_match"][0] == 2 and by["walk ends at j == n"]["n_tot"][0] == 4 + 2
    assert len(by["no hits"]["div"]) == 0 and by["no hits"]["sum_k"] == 15 * 52
    assert by["no minimizers"]["n_tot"][0] == -1 and by["no minimizers"]["sum_k"] == 0
    assert by["varying spans, a chain out of order"]["n_match"].tolist() == [5, 3]             # (in query order 5, 9, 14, 10, 30: the walk passes 10 before it asks for it)


def test_est_err_host_synthetic():
    rng = np.random.default_rng(3)
    reads = [av.synthetic_read(rng, int(rng.integers(1, 400)), [int(v) for v in rng.integers(1, 60, int(rng.integers(0, 12)))], absent_every=5) for _ in range(40)]
    check_against_literal(mm.est_err_host(reads, [100_000], threads=4), reads, [100_000])


def test_est_err_host_refuses_records_outside_their_read():
    reads, ref_len, _ = av.crafted_reads()
    bad = [dict(reads[0], hits=[av.hit(20, 13, 0, 0, 10)])]
    with pytest.raises(mm.Mm2gbError, match="outside its read"):
        mm.est_err_host(bad, ref_len)
    with pytest.raises(mm.Mm2gbError, match=">= n_ref"):
        mm.est_err_host([dict(reads[0], hits=[av.hit(0, 13, 0, 0, 10, rid=2)])], ref_len)


# ---------------------------------------------------------------- the walk at the sizes of the wave instantiation
def test_est_err_host_crafted_long():
    reads, ref_len, what = av.crafted_long()
    got = mm.est_err_host(reads, ref_len, threads=3)
    check_against_literal(got, reads, ref_len)
    by = dict(zip(what, zip(reads, got)))
    assert len(by) == len(what)
    # a defect at k: k anchors counted, whatever the kind, the strand and the chain's spacing
    for cnt in av.LONG_CNTS:
        ks = sorted(k for k in {1, 63, 64, 65, cnt - 1} if k < cnt)
        for strand in ("forward", "reverse"):
            rd, g = by[f"cnt {cnt} {strand}"]
            assert all(h["cnt"] == cnt for h in rd["hits"]) and g["n_match"].tolist() == ([cnt] + ks * len(av.DEFECTS)) * 2
    assert by["two defects, 70 and 100"][1]["n_match"].tolist() == [70] * 8                      # the earlier defect ends the walk
    rd, g = by["beyond the last minimizer"]
    n = len(rd["mini_pos"])
    assert g["n_match"].tolist() == [70, 70, 5, 5, 64, 64, 1, 1, 1, 1, 130, 130] and all(h["cnt"] > m for h, m in zip(rd["hits"], g["n_match"]))
    assert [h["cnt"] for h in rd["hits"][8:10]] == [71, 71] and g["n_tot"][8] == 1 + 2                 # the first anchor is the last minimizer, cnt > 1
    assert max(h["cnt"] for h in rd["hits"]) == 210 > n - (n - 130)
    # mini_pos not strictly ascending: where the changed place lies outside [st, en] the counts are those of the read without it
    clean = by["mini_pos: twice before st"][1]["n_match"].tolist()
    assert clean == [5, 3, 3, 5, 3, 3, 64, 62, 32, 64, 62, 32, 200, 198, 100, 200, 198, 100]
    for name in ("twice after en", "a descending pair before st", "twice inside", "the first anchor's twice"):
        assert by["mini_pos: " + name][1]["n_match"].tolist() == clean, name
    assert by["mini_pos: twice inside"][1]["n_tot"].tolist() != by["mini_pos: twice before st"][1]["n_tot"].tolist()       # (one more place between st and en)
    assert by["mini_pos: a descending pair"][1]["n_match"].tolist() == [3, 3, 3, 3, 3, 3, 3, 3, 32, 3, 3, 32, 3, 3, 100, 3, 3, 100]
    # near 2^31
    rd, g = by["coordinates near 2^31"]
    assert rd["qlen"] == 2**31 - 2 and int(rd["mini_pos"][-1] & 0xffffffff) > 2**31 - 2**24 and g["n_match"].tolist() == [8, 5, 8, 5, 70, 67, 70, 67, 96, 93, 96, 93]
    # at equality nothing is added: 16 > 16.0 is false, 17 > 16.0 true; 17 > 17.288 false, 18 true
    for name, lo in (("avg_k exactly 16", 16), ("avg_k 17.288...", 17)):
        for suffix, per, base in (("", 5, None), (", hits of 130", 4, 130)):
            rd, g = by[name + suffix]
            tot = g["n_tot"].tolist()
            for j, h in enumerate(rd["hits"]):
                walked = h["cnt"] if base is None else base
                v_at = (j // (2 * per)) % 2                                                         # the hits come as (cnt,) v, strand, quantity
                which = j % per
                if which < 2:                                                                       # qs or rs at v, the other end of the hit far from its ends
                    assert tot[j] == walked + v_at + 1, (name, suffix, j)
                elif which < 4:
                    assert tot[j] == walked + 1 + v_at, (name, suffix, j)
                else:                                                                               # qs, rs and ref_len - re at v: both tests turn on v alone
                    assert tot[j] == walked + 2 * v_at, (name, suffix, j)


def test_est_err_host_sum_k_above_2_to_24():
    """1 300 001 minimizers: sum_k is odd and above 2^24, so its float is not its value, and avg_k falls just below 18 where the exact quotient rounds to 18."""
    rd = av.big_read()
    n = len(rd["mini_pos"])
    got = mm.est_err_host([rd], av.LONG_REF_LEN, threads=2)[0]
    sum_k = int((rd["mini_pos"] >> np.uint64(32) & np.uint64(0xff)).sum())
    assert got["sum_k"] == sum_k == 18 * n - 1 and sum_k > 2**24 and sum_k % 2 == 1
    avg_k = np.float32(sum_k) / np.float32(n)                                                       # esterr.c:39: (float)sum_k / n
    assert float(np.float32(sum_k)) == sum_k - 1 and avg_k < np.float32(18.0) == np.float32(sum_k / n)
    h = rd["hits"][0]
    by_hand = (40 - 1) + 1 + int(np.float32(h["qs"]) > avg_k and np.float32(h["rs"]) > avg_k) + int(np.float32(rd["qlen"] - h["qs"]) > avg_k and np.float32(av.LONG_REF_LEN[0] - h["re"]) > avg_k)
    assert (h["qs"], h["rs"]) == (18, 18) and by_hand == 42 and got["n_tot"][0] == by_hand and got["n_match"][0] == 40
    assert got["n_match"].tolist() == [40, 200, 33_333]
    assert got["n_tot"].tolist() == [42, 3 * 199 + 1 + 1, 2 * 33_332 + 1 + 2]                        # (rs = 17 is not above avg_k; ref_len - re = 18 is)


def test_stride_batch_at_a_small_cu_count():
    """The batch tests/test_gpu_ava.py builds for the device's CU count, at 4 CUs: its counts, its special reads, and the host form against the literal walk."""
    reads, ref_len, c = av.stride_batch(4)
    assert c["reads"] == len(reads) > 32 * 4 and c["short_hits"] > 128 * 4 and c["long_hits"] > 32 * 4
    for at in (0, 32 * 4, len(reads) - 2):
        assert len(reads[at]["mini_pos"]) == 0 and len(reads[at]["hits"]) == 1 and len(reads[at + 1]["hits"]) == 0 and len(reads[at + 1]["mini_pos"]) > 0
    check_against_literal(mm.est_err_host(reads, ref_len, threads=4), reads, ref_len)
