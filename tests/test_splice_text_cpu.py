"""The tag text of spliced records on host threads (mm2gb_aln_text_splice_host, csrc/aln_text_host.cpp): cg:Z with N, cs:Z with "~", MD:Z across
introns -- byte for byte against the strings the reference's mm_gen_cs_or_MD printed for the reference's own records (tests/golden/splice/text_*),
against the live reference where oracle/_ref is built, and on records built by hand.  The unspliced text calls keep refusing N."""
import numpy as np
import pytest

import align_cases as ac
import aln_text_cases as at
import mm2gb_amd as mm
import splice_cases as sc

def test_build_text_is_the_reference():
    """The helper's expected strings against mm_gen_cs_or_MD itself, where the reference is built."""
    if not ac.ref_available():
        pytest.skip("the reference is not built here")
    recs = sc.text_recs()
    args = at.batch(recs)
    texts = at.ref_texts(*args)
    for m in ("cs", "cs_long", "md"):
        assert texts[m] == [r[m] for r in recs], m


@pytest.mark.parametrize("what", at.WHATS)
def test_hand_built_records(what):
    recs = sc.text_recs()
    off, text = mm.aln_text_splice_host(what, *at.batch(recs))
    at.assert_texts(at.split(off, text), at.expected(recs, what), f"what {what}")


def test_spelled_out():
    r = sc.build_text([("=", 3), ("N", 12), ("=", 2)], seed=1)
    t = r["ref"]
    assert r["cg"] == b"3M12N2M" and r["md"] == b"5"
    assert r["cs"] == b":3~" + t[3:5].lower() + b"12" + t[13:15].lower() + b":2"
    assert r["cs_long"] == b"=" + t[:3] + b"~" + t[3:5].lower() + b"12" + t[13:15].lower() + b"=" + t[15:17]
    off, text = mm.aln_text_splice_host(mm.TEXT_CG | mm.TEXT_CS, *at.batch([r]))
    assert text == b"\tcg:Z:3M12N2M\tcs:Z:" + r["cs"]


@pytest.mark.parametrize("name", sc.TEXT_BATCHES)
def test_fixture_records(name):
    args, texts = sc.golden_text_args(name), sc.load_texts(name)
    assert sum(x.count(b"~") for x in texts["cs"]) == sc.golden_meta()["batches"][name]["text_introns"] > 50
    for what in at.WHATS:
        off, text = mm.aln_text_splice_host(what, *args, threads=8)
        at.assert_texts(at.split(off, text), at.want_for(args, texts, what), f"{name}: what {what}")
    one = mm.aln_text_splice_host(mm.TEXT_CG | mm.TEXT_CS, *args, threads=1)
    eight = mm.aln_text_splice_host(mm.TEXT_CG | mm.TEXT_CS, *args, threads=8)
    assert one[1] == eight[1] and one[0].tobytes() == eight[0].tobytes()


@pytest.mark.skipif(not ac.ref_available(), reason="the reference is not built here")
def test_live_reference():
    """The records of a fresh spliced batch, aligned by this project's host form, through mm_gen_cs_or_MD."""
    refs, reads = sc.random_batch(61, n_reads=60)
    b, _, _ = sc.ref_batch(refs, reads)
    got, _ = sc.run_host(b, threads=8)
    args = (b["refs"], b["reads"]) + mm.flatten_aligned(got)
    texts = at.ref_texts(*args)
    for what in (mm.TEXT_CS, mm.TEXT_CS | mm.TEXT_CS_LONG, mm.TEXT_MD):
        off, text = mm.aln_text_splice_host(what, *args)
        at.assert_texts(at.split(off, text), at.want_for(args, texts, what), f"what {what}")


def test_refusals():
    for n in (0, 1):          # an N word of length 0 or 1 (format.c:180 asserts len >= 2)
        r = sc.build_text([("=", 5), ("N", 4), ("=", 5)])
        r["words"] = r["words"].copy(); r["words"][1] = n << 4 | 3
        r["reg"] = r["reg"].copy(); r["reg"]["re"] -= 4 - n
        with pytest.raises(mm.Mm2gbError, match="length 0" if n == 0 else "shorter than 2"):
            mm.aln_text_splice_host(mm.TEXT_CS, *at.batch([r]))
    r = sc.build_text([("=", 5), ("N", 4), ("=", 5)])
    for op, letter in ((4, "S"), (7, "=")):
        bad = dict(r, words=r["words"].copy()); bad["words"][0] = 5 << 4 | op
        with pytest.raises(mm.Mm2gbError, match=f"CIGAR operation {letter}"):
            mm.aln_text_splice_host(mm.TEXT_CS, *at.batch([bad]))
    with pytest.raises(mm.Mm2gbError, match="MM2GB_TEXT"):
        mm.aln_text_splice_host(0x10, *at.batch([r]))
    r = sc.build_text([("=", 5), ("N", 4), ("=", 5)], tail=(3, 0))
    bad = dict(r, reg=r["reg"].copy()); bad["reg"]["re"] += 1
    with pytest.raises(mm.Mm2gbError, match="do not sum"):
        mm.aln_text_splice_host(mm.TEXT_CS, *at.batch([bad]))


def test_unspliced_text_calls_still_refuse_n():
    r = sc.build_text([("=", 5), ("N", 4), ("=", 5)])
    with pytest.raises(mm.Mm2gbError, match="CIGAR operation N"):
        mm.aln_text_host(mm.TEXT_CG, *at.batch([r]))
    with pytest.raises(mm.Mm2gbError, match="MM2GB_TEXT"):
        mm.aln_text_host(0x10, *at.batch([sc.build_text([("=", 5)])]))
    plain = sc.build_text(sc.TEXT_CASES["no_intron"])          # ... and both give the same bytes where there is no N
    assert mm.aln_text_host(mm.TEXT_CG | mm.TEXT_MD, *at.batch([plain]))[1] == mm.aln_text_splice_host(mm.TEXT_CG | mm.TEXT_MD, *at.batch([plain]))[1]
