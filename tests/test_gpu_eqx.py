"""The = / X rewrite on the device (mm2gb_cigar_eqx_gpu, csrc/eqx_kernels.hip) against the host form and the recorded words, word for word: the
batches of tests/golden/align, and crafted records at the shapes where the kernels can go wrong -- the cuts every 2048 columns and the rounds
of 256: a run across two cuts, a flip on either side of a cut and of a round, words that begin at a cut, gaps that straddle one, every column
a start, N words around a cut, each on both strands."""
import numpy as np
import pytest

import eqx_cases as ec
import mm2gb_amd as mm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    with mm.Engine() as e:
        yield e


def test_the_seams_are_where_the_cases_put_them(eng):
    info = eng.cigar_eqx_info()
    assert (info["slice"], info["wg"]) == (ec.SLICE, ec.WG)


@pytest.mark.parametrize("name", ec.BATCHES)
def test_recorded_batches(eng, name):
    args = ec.golden_args(name)
    want = ec.load_words(name)
    got = eng.cigar_eqx(*args)
    ec.assert_words(got, want, f"{name}: device against the recorded words")
    host = mm.cigar_eqx_host(*args)
    assert np.array_equal(got[0], host[0]) and np.array_equal(got[1], host[1]), "device and host form differ"


@pytest.mark.parametrize("rev", [False, True])
@pytest.mark.parametrize("name", list(ec.crafted()))
def test_crafted_records(eng, name, rev):
    r = ec.build(ec.crafted()[name], seed=11, rev=rev, lead=(5, 9), tail=(3, 4))
    args = ec.batch([r])
    ec.assert_words(mm.cigar_eqx_host(*args), [r["want"]], f"{name}, rev {rev}: host form")
    ec.assert_words(eng.cigar_eqx(*args), [r["want"]], f"{name}, rev {rev}: device form")


def test_a_mixed_batch_and_an_empty_one(eng):
    recs = [ec.build(segs, seed=20 + i, rev=i % 2 == 1) for i, segs in enumerate(ec.crafted().values())]
    recs.insert(3, ec.build([("X", 1)], seed=2))                                      # a one-column record
    recs.insert(5, dict(ec.build([("=", 4)], seed=3), no_cigar=True))                 # a record without a CIGAR
    recs.append(ec.build([("=", 1)], seed=4, rev=True))
    want = [None if r.get("no_cigar") else r["want"] for r in recs]
    ec.assert_words(eng.cigar_eqx(*ec.batch(recs)), want, "mixed batch")
    aln, words = eng.cigar_eqx(*ec.batch([]))
    assert len(aln) == 0 and len(words) == 0
    ec.assert_words(eng.cigar_eqx(*ec.batch(recs[::-1])), want[::-1], "the batch backwards, after the empty one")


def test_a_refused_call_leaves_the_engine_usable(eng):
    r = ec.build([("=", 3000), ("X", 2), ("=", 10)], seed=6)
    bad = dict(r, words=np.array([ec.w(3000, ec.EQ), ec.w(12, ec.M)], np.uint32))
    with pytest.raises(mm.Mm2gbError, match="rewritten already"):
        eng.cigar_eqx(*ec.batch([bad]))
    with pytest.raises(mm.Mm2gbError, match="do not sum"):
        eng.cigar_eqx(*ec.batch([dict(r, words=np.array([ec.w(3000, ec.M)], np.uint32))]))
    ec.assert_words(eng.cigar_eqx(*ec.batch([r])), [r["want"]], "a good call after the refusals")


def test_the_text_call_and_the_rewrite_take_turns(eng):
    """Both run on one plan's buffers: a text call between two rewrites changes neither."""
    import aln_text_cases as at
    args = ec.golden_args("ont")
    want = ec.load_words("ont")
    ec.assert_words(eng.cigar_eqx(*args), want, "before the text call")
    text = eng.aln_text(mm.TEXT_CG | mm.TEXT_CS, *args)
    host = mm.aln_text_host(mm.TEXT_CG | mm.TEXT_CS, *args)
    assert text[1] == host[1] and np.array_equal(text[0], host[0])
    ec.assert_words(eng.cigar_eqx(*args), want, "after the text call")
    assert at.BATCHES == ec.BATCHES


def test_recorded_spliced_batch(eng):
    """N words from the reference's own splice path (tests/golden/splice, `default`)."""
    args = ec.golden_splice_args()
    ec.assert_words(eng.cigar_eqx(*args), ec.load_words("splice_default"), "splice default: device against the recorded words")
