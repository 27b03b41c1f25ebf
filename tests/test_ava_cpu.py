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
