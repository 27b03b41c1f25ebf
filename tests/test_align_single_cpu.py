"""The alignment of hits at q == q2 && e == e2 (mm2gb_align_regs_extz_host; mm_align_pair then runs ksw_extz2_sse) against the reference's
mm_align_skeleton: the committed fixtures (tests/golden/paf_single/align_*.npz) everywhere, fresh reads against the compiled reference where
oracle/_ref is built.  Every comparison is exact: records, alignment fields and CIGAR words."""
import copy

import numpy as np
import pytest

import align_cases as ac
import ksw_single_cases as ks
import mm2gb_amd as mm


@pytest.fixture(scope="module")
def golden():
    return {name: ks.load_align(name) for name in ks.ALIGN_BATCHES}


@pytest.mark.parametrize("name", list(ks.ALIGN_BATCHES))
def test_host_equals_fixtures(golden, name):
    b, want = golden[name]
    q, e = ks.ALIGN_BATCHES[name]
    assert (b["opt"].q, b["opt"].e, b["opt"].q2, b["opt"].e2) == (q, e, q, e)
    got, info = ks.run_align_host(b, threads=4)
    ac.assert_same(got, want, name)
    assert info["counts"]["jobs"] > 0
    one, _ = ks.run_align_host(b, threads=1)
    ac.assert_same(one, want, name + ", 1 thread")


def test_batch_schedule_gives_identical_bytes(golden, monkeypatch):
    """MM2GB_ALIGN_ROUNDS=batch: the device form's schedule with the host DP behind it."""
    monkeypatch.setenv("MM2GB_ALIGN_ROUNDS", "batch")
    for name, (b, want) in golden.items():
        ac.assert_same(ks.run_align_host(b, threads=8)[0], want, name + " (batch schedule)")


@pytest.mark.skipif(not ac.ref_available(), reason="the reference build (oracle/_ref) is not here")
@pytest.mark.parametrize("preset,q,e", [("map-ont", 4, 2), ("map-pb", 6, 2)])
def test_host_equals_live_reference(preset, q, e):
    """300 fresh reads per preset, a tenth of them with unrelated sequence or an inverted block in the middle."""
    refs, reads = ac.random_batch(41 if preset == "map-ont" else 42, preset, n_reads=300)
    b, want = ac.ref_batch(refs, reads, preset, q=q, e=e, q2=q, e2=e)
    got, info = ks.run_align_host(b, threads=8)
    ac.assert_same(got, want, preset)


def test_align_opt_builds_the_option_set(golden):
    o, w = mm.align_opt("map-ont", q2=4, e2=2), golden["ont"][0]["opt"]
    assert all(getattr(o, k) == getattr(w, k) for k, _ in mm.AlignOpt._fields_ if k != "max_sw_mat")


def test_refusals(golden):
    b, _ = golden["ont"]

    def with_opt(**kw):
        c = dict(b)
        c["opt"] = copy.copy(b["opt"])
        for k, v in kw.items():
            setattr(c["opt"], k, v)
        return c
    # q != q2 || e != e2 belongs to the pair without _extz, and the error names it
    for kw in (dict(q2=24), dict(e2=1), dict(q2=24, e2=1)):
        with pytest.raises(mm.Mm2gbError, match=r"mm2gb_align_regs_extz_host: q != q2 \|\| e != e2 selects ksw_extd2_sse: that is mm2gb_align_regs_host / mm2gb_align_regs_gpu"):
            ks.run_align_host(with_opt(**kw))
    # ... and that pair still refuses this option set, in the words it always had
    with pytest.raises(mm.Mm2gbError, match="mm2gb_align_regs_host: q == q2 && e == e2 selects ksw_extz2_sse, which is not supported"):
        ac.run_host(b)
    for name, bit in (("MM_F_SPLICE", mm.F_SPLICE), ("MM_F_SR", mm.F_SR), ("MM_F_QSTRAND", mm.F_QSTRAND), ("MM_F_EQX", mm.F_EQX)):
        with pytest.raises(mm.Mm2gbError, match="mm2gb_align_regs_extz_host: " + name + " is not supported"):
            ks.run_align_host(with_opt(flag=b["opt"].flag | bit))
    for v in (0, 100_000_001):
        with pytest.raises(mm.Mm2gbError, match="max_sw_mat"):
            ks.run_align_host(with_opt(max_sw_mat=v))
    with pytest.raises(mm.Mm2gbError, match="gap penalties out of range"):          # 2(q + e) > 127
        ks.run_align_host(with_opt(q=61, q2=61, e=3, e2=3))
    for text, bad in ac.refusals(b)[-3:]:                                            # anchors outside their records, multi-segment reads
        with pytest.raises(mm.Mm2gbError, match=text):
            ks.run_align_host(bad)
    c = dict(b); c["anchors"] = [x.copy() for x in b["anchors"]]
    k = next(i for i, x in enumerate(c["regs"]) if len(x))
    c["anchors"][k][int(c["regs"][k]["as_"][0]), 0] |= np.uint64(0x7fffffff)         # a reference position far beyond its sequence
    with pytest.raises(mm.Mm2gbError, match="an anchor lies outside its sequences"):
        ks.run_align_host(c)
