"""The text of the alignment tags on the device (mm2gb_aln_text_gpu, csrc/aln_text_kernels.hip) against the host form, byte for byte: the
records of tests/golden/align for every `what`, and records built to put runs, words and records on the seams of the device form -- the cut
between two slices, between two rounds of a workgroup and between two waves -- with the text they must give known from how they were built."""
import numpy as np
import pytest

import aln_text_cases as tc
import mm2gb_amd as mm

pytestmark = pytest.mark.gpu
CG, CS, LONG, MD = mm.TEXT_CG, mm.TEXT_CS, mm.TEXT_CS_LONG, mm.TEXT_MD
SOME = (CS, CS | LONG, MD, CG | CS)


@pytest.fixture(scope="module")
def eng():
    with mm.Engine(device=0) as e:
        yield e


@pytest.fixture(scope="module")
def seams(eng):
    info = eng.aln_text_info()
    assert info["slice"] >= 2 * info["wg"] and info["wg"] % 64 == 0
    return info["slice"], info["wg"]


def check(eng, recs, what_list=SOME, name=""):
    """device == host == the text the records were built with"""
    args = tc.batch(recs)
    for what in what_list:
        got = tc.split(*eng.aln_text(what, *args))
        tc.assert_texts(got, tc.split(*mm.aln_text_host(what, *args, threads=8)), f"{name}: device against host, what = {what}")
        tc.assert_texts(got, tc.expected(recs, what), f"{name}: device against the built text, what = {what}")


@pytest.mark.parametrize("name", tc.BATCHES)
def test_device_equals_host_and_recorded_reference(eng, name):
    args, texts = tc.golden_args(name), tc.load_texts(name)
    for what in tc.WHATS:
        off, text = eng.aln_text(what, *args)
        h_off, h_text = mm.aln_text_host(what, *args, threads=8)
        assert np.array_equal(off, h_off), f"{name}, what = {what}: offsets"
        tc.assert_texts(tc.split(off, text), tc.split(h_off, h_text), f"{name}: device against host, what = {what}")
        tc.assert_texts(tc.split(off, text), tc.want_for(args, texts, what), f"{name}: device against the reference, what = {what}")


def test_run_ends_at_before_and_after_a_seam(eng, seams):
    """A match run whose closing event is the first column after a cut, the last before it, the second after it: at the slice's seam, a round's
    and a wave's; then the same with the run's START moved instead."""
    S, G = seams
    recs = []
    for seam in (S, 2 * S, G, 3 * G, 64, S - 64):
        for d in (-1, 0, 1):
            recs.append(tc.build([("=", seam + d), ("X", 1), ("=", 37)], seed=len(recs)))
            recs.append(tc.build([("=", 11), ("X", 1), ("=", seam + d - 12), ("D", 2), ("=", 5)], seed=len(recs)))
            recs.append(tc.build([("=", seam + d), ("I", 3), ("=", 9)], seed=len(recs), rev=True, lead=(1, 2), tail=(3, 4)))
            recs.append(tc.build([("X", seam + d), ("=", S + 3)], seed=len(recs)))                       # the run STARTS at the seam and ends with the record
    check(eng, recs, name="run ends at a seam")


def test_run_crosses_slices_without_an_event(eng, seams):
    S, _ = seams
    recs = [tc.build([("=", 5), ("X", 1), ("=", S // 2 + n * S + S // 2), ("X", 1), ("=", 10)], seed=n) for n in (1, 2, 5)]
    recs += [tc.build([("=", 3 * S)], seed=7), tc.build([("=", 3 * S + 1)], seed=8, rev=True), tc.build([("=", 2 * S), ("I", 4), ("=", 2 * S), ("D", 1), ("=", 2 * S)], seed=9)]
    check(eng, recs, name="run across slices")


def test_power_of_ten_run_straddles_a_cut(eng, seams):
    S, _ = seams
    recs = []
    for k in range(1, 6):
        for n in (10**k - 1, 10**k):
            recs.append(tc.build([("=", S - 5), ("X", 1), ("=", n), ("X", 1), ("=", 3)], seed=len(recs)))
            recs.append(tc.build([("=", S - 5), ("D", 1), ("=", n)], seed=len(recs)))                 # closed by the record's end
    check(eng, recs, name="10^k")


def test_words_longer_than_a_slice_and_cuts_inside_words(eng, seams):
    S, _ = seams
    recs = [tc.build([("=", 100), ("I", S + 300), ("=", 100), ("D", 2 * S + 700), ("=", 100)], seed=1),
            tc.build([("I", S), ("D", S), ("=", 1)], seed=2, rev=True),
            tc.build([("=", S - 2), ("I", 5), ("=", 10)], seed=3),                                  # the cut inside an I word
            tc.build([("=", S - 2), ("D", 5), ("=", 10)], seed=4),
            tc.build([("=", S - 1), ("W", 0), ("=", 1), ("W", 0), ("=", S)], seed=5),                # a word of one column in front of the cut
            tc.build([("=", S), ("W", 0), ("=", S)], seed=6)]                                       # the cut between two M words
    check(eng, recs, what_list=SOME + (CG | MD,), name="long words")


def test_more_words_than_a_slice(eng, seams):
    """cg:Z is cut by words: a record of 2.5 slices of words, and one of exactly a slice."""
    S, _ = seams
    many = [s for _ in range(5 * S // 4) for s in (("=", 1), ("I", 1))]
    check(eng, [tc.build(many, seed=1), tc.build(many[:S], seed=2), tc.build(many[:S + 1], seed=3)], what_list=(CG, CG | MD, CG | CS | LONG), name="many words")


def test_records_of_one_column_and_none(eng):
    recs = [tc.build([(k, 1)], seed=i) for i, k in enumerate("=XID")] + [tc.build([], seed=9)]
    recs.insert(2, dict(tc.build([("=", 5)], seed=4), no_cigar=True))
    check(eng, recs, what_list=tc.WHATS, name="one column")
    off, text = eng.aln_text(CG | CS, [], [], np.zeros(0, mm.REG_DTYPE), [], np.zeros(0, mm.ALN_DTYPE), [])
    assert list(off) == [0] and text == b""


def test_3000_one_word_records(eng):
    rng = np.random.default_rng(5)
    recs = [tc.build([("=", int(rng.integers(1, 40)))], seed=i, rev=bool(i & 1)) for i in range(3000)]
    check(eng, recs, what_list=(CG | CS, MD), name="3000 records")


def test_one_long_record_beside_500_tiny_ones(eng, seams):
    S, _ = seams
    rng = np.random.default_rng(6)
    tiny = [tc.build(tc.random_segs(rng, int(rng.integers(1, 60)), match=8), seed=i, rev=bool(i % 3 == 0)) for i in range(500)]
    big = tc.build(tc.random_segs(rng, 40 * S - 100), seed=1000, rev=True, lead=(7, 9), tail=(5, 3))
    assert 39 * S < sum(int(w) >> 4 for w in big["words"]) <= 41 * S
    check(eng, tiny[:250] + [big] + tiny[250:], name="long beside tiny")


def test_arena_reuse(eng, seams):
    """A small call, a larger one, the small one again: identical bytes."""
    S, _ = seams
    rng = np.random.default_rng(7)
    small = tc.batch([tc.build(tc.random_segs(rng, 300), seed=1)])
    large = tc.batch([tc.build(tc.random_segs(rng, 5 * S), seed=i) for i in range(2, 12)])
    first = eng.aln_text(CG | CS, *small)
    assert eng.aln_text(CG | CS, *large)[1] == mm.aln_text_host(CG | CS, *large)[1]
    again = eng.aln_text(CG | CS, *small)
    assert first[1] == again[1] == mm.aln_text_host(CG | CS, *small)[1] and np.array_equal(first[0], again[0])


def test_refusals(eng):
    ok = tc.batch([tc.build([("=", 5), ("I", 2), ("=", 5)], seed=4)])
    for text, word in (("CIGAR operation N", 2 << 4 | 3), ("CIGAR operation =", 2 << 4 | 7), ("CIGAR operation X", 2 << 4 | 8), ("length 0", 1), ("do not sum", 3 << 4 | 1)):
        bad = ok[:5] + (ok[5].copy(),)
        bad[5][1] = word
        with pytest.raises(mm.Mm2gbError, match=text):
            eng.aln_text(CS, *bad)
    bad = ok[:2] + (ok[2].copy(),) + ok[3:]
    bad[2]["re"] += 1
    with pytest.raises(mm.Mm2gbError, match="outside its sequences"):
        eng.aln_text(CS, *bad)
    with pytest.raises(mm.Mm2gbError, match="MM2GB_TEXT"):
        eng.aln_text(0x20, *ok)
    assert eng.aln_text(CS, *ok)[1] == mm.aln_text_host(CS, *ok)[1]                            # a refused call leaves the engine usable
