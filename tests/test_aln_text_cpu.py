"""The text of the alignment tags on host threads (mm2gb_aln_text_host, csrc/aln_text_host.cpp): cg:Z, cs:Z short and long, MD:Z against what the
reference's mm_gen_cs_or_MD printed for the records of tests/golden/align (tests/golden/paf_aln/text_*.npz), against the reference itself on
fresh records where oracle/_ref is built, hand-made records with their text written out, and the refusals.  Every comparison is of bytes."""
import numpy as np
import pytest

import align_cases as ac
import aln_text_cases as tc
import mm2gb_amd as mm

CG, CS, LONG, MD = mm.TEXT_CG, mm.TEXT_CS, mm.TEXT_CS_LONG, mm.TEXT_MD


def host(recs, what, threads=2):
    return tc.split(*mm.aln_text_host(what, *tc.batch(recs), threads=threads))


@pytest.mark.parametrize("name", tc.BATCHES)
def test_host_equals_recorded_reference(name):
    args, texts = tc.golden_args(name), tc.load_texts(name)
    assert len(texts["cs"]) == len(args[2]) > 0
    for what in tc.WHATS:
        tc.assert_texts(tc.split(*mm.aln_text_host(what, *args)), tc.want_for(args, texts, what), f"{name}, what = {what}")


@pytest.mark.skipif(not ac.ref_available(), reason="the reference is not built here")
def test_host_equals_live_reference():
    """200 records of a fresh batch, aligned by the reference, their text by the reference."""
    refs, reads = ac.random_batch(41, "map-ont", n_reads=220)
    b, want = ac.ref_batch(refs, reads, "map-ont")
    regs, read_of, aln, cigar = mm.flatten_aligned(want)
    pick = np.sort(np.random.default_rng(1).permutation(len(regs))[:200])
    assert len(pick) == 200
    args = (b["refs"], b["reads"], regs[pick], read_of[pick], aln[pick], cigar)
    texts = tc.ref_texts(*args)
    assert (regs[pick]["flags"] >> 10 & 1).any() and not (regs[pick]["flags"] >> 10 & 1).all()
    for what in (CS, CS | LONG, MD, CG | CS):
        tc.assert_texts(tc.split(*mm.aln_text_host(what, *args, threads=8)), tc.want_for(args, texts, what), f"live, what = {what}")


def test_builder_agrees_with_written_out_text():
    """The cases below and the device tests lean on aln_text_cases.build: one record with every kind of segment, its text written out by hand."""
    r = tc.build([("=", 3), ("X", 1), ("=", 2), ("I", 2), ("=", 4), ("D", 3), ("=", 1)], seed=3)
    t, q = r["ref"], r["read"]
    assert r["cg"] == b"6M2I4M3D1M" and len(t) == 14 and len(q) == 13
    assert r["cs"] == b":3*" + t[3:4].lower() + q[3:4].lower() + b":2+" + q[6:8].lower() + b":4-" + t[10:13].lower() + b":1"
    assert r["md"] == b"3" + t[3:4] + b"6^" + t[10:13] + b"1"
    assert r["cs_long"] == b"=" + t[0:3] + b"*" + t[3:4].lower() + q[3:4].lower() + b"=" + t[4:6] + b"+" + q[6:8].lower() + b"=" + t[6:10] + b"-" + t[10:13].lower() + b"=" + t[13:14]
    for what in tc.WHATS:
        assert host([r], what) == tc.expected([r], what)


def test_written_out_by_hand():
    """A record given as plain text, no builder: target ACGTNACGTACGA, query ACCTNAGTAAAACG as 6M1D3M2I3M."""
    reg = np.zeros(1, mm.REG_DTYPE)
    reg["re"], reg["qe"] = 13, 14
    ref, read = b"ACGTNACGTACGA", b"ACCTNAGTAAAACG"
    #   ACGTNA C GTA -- CGA
    #   ACCTNA - GTA AA ACG      columns: 6M 1D 3M 2I 3M
    w = np.array([6 << 4, 1 << 4 | 2, 3 << 4, 2 << 4 | 1, 3 << 4], np.uint32)
    aln = np.zeros(1, mm.ALN_DTYPE); aln["n_cigar"] = 5
    args = ([ref], [read], reg, np.zeros(1, np.int32), aln, w)
    text = lambda what: mm.aln_text_host(what, *args)[1]
    assert text(CG) == b"\tcg:Z:6M1D3M2I3M"
    assert text(CS) == b"\tcs:Z::2*gc:3-c:3+aa*ca*gc*ag"
    assert text(CS | LONG) == b"\tcs:Z:=AC*gc=TNA-c=GTA+aa*ca*gc*ag"
    assert text(MD) == b"\tMD:Z:2G3^C3C0G0A"
    assert text(CG | CS | MD) == b"\tcg:Z:6M1D3M2I3M\tMD:Z:2G3^C3C0G0A"
    assert text(0) == b""


def test_one_word_of_identical_bases():
    for n in (1, 7, 250):
        r = tc.build([("=", n)], seed=n)
        assert host([r], CS) == [b"\tcs:Z::%d" % n] and host([r], MD) == [b"\tMD:Z:%d" % n] and host([r], CG) == [b"\tcg:Z:%dM" % n]
        assert host([r], CS | LONG) == [b"\tcs:Z:=" + r["ref"]]


def test_mismatch_in_first_and_last_column():
    r = tc.build([("X", 1), ("=", 5), ("X", 1)], seed=2)
    t, q = r["ref"], r["read"]
    assert host([r], CS) == [b"\tcs:Z:*" + (t[0:1] + q[0:1]).lower() + b":5*" + (t[6:7] + q[6:7]).lower()]
    assert host([r], MD) == [b"\tMD:Z:0" + t[0:1] + b"5" + t[6:7]]            # nothing after the last mismatch: the count is zero


@pytest.mark.parametrize("n", [9, 10, 99, 100, 1000])
def test_run_lengths_where_the_digits_change(n):
    r = tc.build([("=", n), ("X", 1), ("=", n), ("D", 2), ("=", n)], seed=n)
    for what in (CS, MD, CS | LONG, CG):
        assert host([r], what) == tc.expected([r], what)
    assert host([r], CS)[0].count(b":%d" % n) == 3 and host([r], MD)[0].endswith(b"%d" % n)


def test_n_against_n_and_n_against_a():
    reg = np.zeros(1, mm.REG_DTYPE)
    reg["re"], reg["qe"] = 6, 6
    aln = np.zeros(1, mm.ALN_DTYPE); aln["n_cigar"] = 1
    args = ([b"ANNCGT"], [b"ANACXT"], reg, np.zeros(1, np.int32), aln, np.array([6 << 4], np.uint32))         # X is no base: it reads as N
    assert mm.aln_text_host(CS, *args)[1] == b"\tcs:Z::2*na:1*gn:1"
    assert mm.aln_text_host(CS | LONG, *args)[1] == b"\tcs:Z:=AN*na=C*gn=T"
    assert mm.aln_text_host(MD, *args)[1] == b"\tMD:Z:2N1G1"


def test_deletion_directly_after_a_mismatch():
    r = tc.build([("=", 4), ("X", 1), ("D", 2), ("=", 3)], seed=5)
    t = r["ref"]
    assert host([r], MD) == [b"\tMD:Z:4" + t[4:5] + b"0^" + t[5:7] + b"3"]
    assert host([r], CS)[0].endswith(b"-" + t[5:7].lower() + b":3")
    r = tc.build([("D", 2), ("D", 1), ("=", 3)], seed=6)                          # two D words in a row, and a deletion first
    assert host([r], MD) == [b"\tMD:Z:0^" + r["ref"][0:2] + b"0^" + r["ref"][2:3] + b"3"] and r["cg"] == b"2D1D3M"


def test_insertion_between_two_match_runs():
    r = tc.build([("=", 5), ("I", 3), ("=", 6)], seed=7)
    assert host([r], MD) == [b"\tMD:Z:11"]                                       # the count runs on across the insertion
    assert host([r], CS) == [b"\tcs:Z::5+" + r["read"][5:8].lower() + b":6"]   # the run does not
    r = tc.build([("=", 5), ("W", 0), ("=", 6)], seed=8)                          # two M words in a row: a run ends with its word
    assert r["cg"] == b"5M6M" and host([r], CS) == [b"\tcs:Z::5:6"] and host([r], MD) == [b"\tMD:Z:11"]
    assert host([r], CS | LONG) == [b"\tcs:Z:=" + r["ref"][:5] + b"=" + r["ref"][5:]]


def test_reverse_strand_record():
    segs = [("=", 6), ("X", 2), ("I", 2), ("=", 5), ("D", 3), ("=", 4)]
    fwd, rev = tc.build(segs, seed=9, lead=(3, 5), tail=(2, 7)), tc.build(segs, seed=9, rev=True, lead=(3, 5), tail=(2, 7))
    assert rev["read"] == tc.revcomp(fwd["read"]) and int(rev["reg"]["qs"][0]) == 7 and int(fwd["reg"]["qs"][0]) == 5
    for what in tc.WHATS:
        assert host([rev], what) == tc.expected([fwd], what) == host([fwd], what)
    n = tc.build([("=", 3)], seed=1, rev=True)                                    # N on the reverse strand stays N
    n["ref"], n["read"] = b"ANG", b"CNT"
    assert host([n], CS | LONG) == [b"\tcs:Z:=ANG"]


def test_record_without_cigar_and_empty_calls():
    a, b, c = tc.build([("=", 4)], seed=1), tc.build([("=", 9)], seed=2), tc.build([("X", 1)], seed=3)
    b["no_cigar"] = True
    off, text = mm.aln_text_host(CG | CS, *tc.batch([a, b, c]))
    want = tc.expected([a, b, c], CG | CS)
    assert want[1] == b"" and list(off) == [0, len(want[0]), len(want[0]), len(want[0]) + len(want[2])] and tc.split(off, text) == want
    b2 = dict(b); b2["reg"] = b["reg"].copy(); b2["reg"]["re"] = 10**6                  # a record without a CIGAR is not looked at
    assert tc.split(*mm.aln_text_host(CS, *tc.batch([b2, a]))) == [b"", b"\tcs:Z::4"]
    off, text = mm.aln_text_host(CG | MD, [], [], np.zeros(0, mm.REG_DTYPE), [], np.zeros(0, mm.ALN_DTYPE), [])
    assert list(off) == [0] and text == b""
    z = tc.build([], seed=1)                                                      # a CIGAR of no words: the tags' names alone
    assert host([z], CG | CS) == [b"\tcg:Z:\tcs:Z:"]


def test_threads_give_identical_bytes():
    args = tc.golden_args("ont")
    for what in (CG | CS, MD):
        assert mm.aln_text_host(what, *args, threads=1)[1] == mm.aln_text_host(what, *args, threads=8)[1]


def refusals():
    """(what the error names, the call that is refused): one sound record, and a second one with a single change"""
    ok = tc.build([("=", 5), ("I", 2), ("=", 5), ("D", 1), ("=", 3)], seed=4, lead=(2, 2), tail=(2, 2))
    def change(word=None, read_of=None, **kw):
        refs, reads, regs, read_of_reg, aln, cigar = tc.batch([tc.build([("=", 3)]), ok])
        for k, v in kw.items():
            regs[k][1] = v
        if word:
            cigar[int(aln["cigar_off"][1]) + word[0]] = word[1]
        if read_of is not None:
            read_of_reg[1] = read_of
        return refs, reads, regs, read_of_reg, aln, cigar
    out = [("CIGAR operation " + name, change(word=(1, 2 << 4 | op))) for name, op in (("N", 3), ("=", 7), ("X", 8), ("S", 4))]
    out.append(("length 0", change(word=(1, 1))))
    out.append(("do not sum", change(word=(0, 6 << 4))))                          # one column more on both sides
    out.append(("do not sum", change(qe=int(ok["reg"]["qe"][0]) + 1)))              # the query alone
    out.append(("do not sum", change(re=int(ok["reg"]["re"][0]) - 1)))              # the target alone
    out.append(("outside its sequences", change(re=len(ok["ref"]) + 1)))
    out.append(("outside its sequences", change(qe=len(ok["read"]) + 1)))
    out.append(("outside its sequences", change(rs=-1)))
    out.append(("outside its sequences", change(qs=9, qe=8)))
    out.append(("outside its sequences", change(rid=2)))
    out.append(("outside its sequences", change(rid=-1)))
    out.append(("outside its sequences", change(read_of=2)))
    return out


def test_refusals():
    for text, args in refusals():
        with pytest.raises(mm.Mm2gbError, match=text):
            mm.aln_text_host(CS, *args)
    with pytest.raises(mm.Mm2gbError, match="MM2GB_TEXT"):
        mm.aln_text_host(0x10, *tc.batch([tc.build([("=", 3)])]))
    with pytest.raises(mm.Mm2gbError, match="CIGAR operation N"):                        # checked whatever is asked for
        mm.aln_text_host(0, *refusals()[0][1])
