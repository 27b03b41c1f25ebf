"""The = / X rewrite on host threads (mm2gb_cigar_eqx_host; minimap2 --eqx, mm_update_cigar_eqx): against the words the reference left under
MM_F_EQX for the batches of tests/golden/align (tests/golden/sam/eqx_*.npz), against the live reference where it is built, on hand-made records
with the expected words written out, and the refusals by name."""
import numpy as np
import pytest

import align_cases as ac
import eqx_cases as ec
import mm2gb_amd as mm
from eqx_cases import D, EQ, I, M, N, X, w

needs_ref = pytest.mark.skipif(not ac.ref_available(), reason="the reference build (oracle/_ref) is not here")


@pytest.mark.parametrize("name", ec.BATCHES)
def test_recorded_words(name):
    args = ec.golden_args(name)
    want = ec.load_words(name)
    assert len(want) == len(args[2]) and any(x is not None and len(x) for x in want)
    for threads in (1, 4):
        ec.assert_words(mm.cigar_eqx_host(*args, threads=threads), want, f"{name}, {threads} threads")
    aln, cigar = args[4].copy(), args[5].copy()
    mm.cigar_eqx_host(*args)
    assert np.array_equal(aln, args[4]) and np.array_equal(cigar, args[5]), "the input is untouched"


def test_the_vectors_hold_what_the_tests_rely_on():
    ops = np.concatenate([x for name in ec.BATCHES for x in ec.load_words(name) if x is not None]) & 0xf
    assert set(np.unique(ops)) == {I, D, EQ, X}
    assert any((ec.golden_args(name)[2]["flags"] >> 10 & 1).any() for name in ec.BATCHES), "no reverse-strand record"


@needs_ref
@pytest.mark.parametrize("preset", ["map-ont", "map-pb"])
def test_fresh_reads_against_the_reference(preset):
    refs, reads = ac.random_batch(41, preset, n_reads=300)
    b, want = ac.ref_batch(refs, reads, preset)
    regs, read_of, aln, cigar = mm.flatten_aligned(want)
    eregs, _, ealn, ecigar = ec.ref_words(refs, reads, preset, anchors=b["anchors"])
    assert np.array_equal(regs, eregs) and len(regs) > 250
    ec.assert_words(mm.cigar_eqx_host(refs, reads, regs, read_of, aln, cigar, threads=8), ec.split(ealn, ecigar), preset)


@needs_ref
def test_fresh_spliced_reads_against_the_reference():
    """-x splice: N words from the reference's own splice path, copied between the = / X runs."""
    import splice_cases
    refs, reads = splice_cases.random_batch(41, n_reads=300)
    b, want, _ = splice_cases.ref_batch(refs, reads)
    regs, read_of, aln, cigar = mm.flatten_aligned(want)
    _, ewant, _ = splice_cases.ref_batch(refs, reads, anchors=b["anchors"], flag_set=mm.F_EQX)
    eregs, _, ealn, ecigar = mm.flatten_aligned(ewant)
    assert np.array_equal(regs, eregs) and len(regs) > 250 and (ecigar & 0xf == N).sum() > 100
    ec.assert_words(mm.cigar_eqx_host(refs, reads, regs, read_of, aln, cigar, threads=8), ec.split(ealn, ecigar), "splice")


def test_recorded_spliced_words():
    args = ec.golden_splice_args()
    want = ec.load_words("splice_default")
    assert (np.concatenate([x for x in want if x is not None]) & 0xf == N).any()
    ec.assert_words(mm.cigar_eqx_host(*args), want, "splice_default")


HAND = {          # name -> (segments, the words written out)
    "one_column_m": ([("=", 1)], [w(1, EQ)]),
    "one_column_x": ([("X", 1)], [w(1, X)]),
    "all_mismatch": ([("X", 37)], [w(37, X)]),
    "n_against_n": ([("=", 5), ("n", 3), ("=", 4)], [w(12, EQ)]),
    "n_against_n_alone": ([("n", 2)], [w(2, EQ)]),
    "flip_at_the_last_column": ([("=", 20), ("X", 1)], [w(20, EQ), w(1, X)]),
    "flip_at_the_first_column": ([("X", 1), ("=", 20)], [w(1, X), w(20, EQ)]),
    "m_i_m_matches_either_side": ([("=", 6), ("I", 2), ("=", 7)], [w(6, EQ), w(2, I), w(7, EQ)]),
    "m_d_m": ([("=", 6), ("X", 2), ("D", 3), ("X", 1), ("=", 7)], [w(6, EQ), w(2, X), w(3, D), w(1, X), w(7, EQ)]),
    "two_m_words_not_merged": ([("=", 6), ("W", 0), ("=", 7)], [w(6, EQ), w(7, EQ)]),
    "an_n_word": ([("=", 9), ("N", 120), ("=", 4), ("X", 1)], [w(9, EQ), w(120, N), w(4, EQ), w(1, X)]),
}


@pytest.mark.parametrize("rev", [False, True])
@pytest.mark.parametrize("name", list(HAND))
def test_hand_made_records(name, rev):
    segs, want = HAND[name]
    r = ec.build(segs, seed=5, rev=rev, lead=(7, 3), tail=(2, 11))
    assert list(r["want"]) == want, "the builder's own expectation"
    ec.assert_words(mm.cigar_eqx_host(*ec.batch([r])), [np.array(want, np.uint32)], f"{name}, rev {rev}")


def test_a_batch_with_a_record_without_a_cigar_and_an_empty_batch():
    recs = [ec.build(HAND["m_d_m"][0], seed=1), dict(ec.build([("=", 4)], seed=2), no_cigar=True), ec.build(HAND["an_n_word"][0], seed=3, rev=True)]
    aln, words = mm.cigar_eqx_host(*ec.batch(recs))
    ec.assert_words((aln, words), [recs[0]["want"], None, recs[2]["want"]], "mixed batch")
    assert aln["cigar_off"][1] == -1
    aln, words = mm.cigar_eqx_host(*ec.batch([]))
    assert len(aln) == 0 and len(words) == 0


def test_refusals_by_name():
    r = ec.build([("=", 10), ("I", 2), ("=", 5)], seed=9)
    def go(words=None, **reg):
        x = dict(r, words=np.array(r["words"] if words is None else words, np.uint32), reg=r["reg"].copy())
        for k, v in reg.items():
            x["reg"][k] = v
        return mm.cigar_eqx_host(*ec.batch([x]))
    with pytest.raises(mm.Mm2gbError, match="rewritten already"):
        go([w(10, EQ), w(2, I), w(5, M)])
    with pytest.raises(mm.Mm2gbError, match="CIGAR operation X"):
        go([w(10, X), w(2, I), w(5, M)])
    with pytest.raises(mm.Mm2gbError, match="CIGAR operation S is not supported"):
        go([w(10, M), w(2, 4), w(5, M)])
    with pytest.raises(mm.Mm2gbError, match="length 0"):
        go([w(10, M), w(0, I), w(2, I), w(5, M)])
    with pytest.raises(mm.Mm2gbError, match="do not sum"):
        go([w(10, M), w(2, I), w(4, M)])
    with pytest.raises(mm.Mm2gbError, match="outside its sequences"):
        go(re=10_000)
    with pytest.raises(mm.Mm2gbError, match="one entry per record"):
        args = ec.batch([r])
        mm.cigar_eqx_host(args[0], args[1], args[2], args[3][:0], args[4], args[5])
    ec.assert_words(go(), [r["want"]], "a good call after the refusals")


def test_the_text_calls_keep_refusing_eqx_words_and_the_alignment_calls_the_flag():
    r = ec.build([("=", 10), ("X", 2)], seed=4)
    aln, words = mm.cigar_eqx_host(*ec.batch([r]))
    args = ec.batch([r])
    with pytest.raises(mm.Mm2gbError, match="CIGAR operation = is not supported"):
        mm.aln_text_host(mm.TEXT_CS, args[0], args[1], args[2], args[3], aln, words)
    b, _ = ac.load_batch("small_mat")
    b["opt"].flag |= mm.F_EQX
    with pytest.raises(mm.Mm2gbError, match="MM_F_EQX"):
        ac.run_host(b)
