"""The spliced alignment of hits with the DP and its sequences on the device (mm2gb_align_regs_splice_gpu, csrc/align_kernels.hip) against the
host form and the committed fixtures (tests/golden/splice): every record, field and CIGAR word, and the paths met.  Reads fixtures only."""
import copy

import numpy as np
import pytest

import align_cases as ac
import mm2gb_amd as mm
import splice_cases as sc

pytestmark = pytest.mark.gpu
NAMES = ["default", "hq", "for_only", "rev_only", "no_flank", "no_end_flt", "small_mat"]


@pytest.fixture(scope="module")
def eng():
    with mm.Engine(device=0) as e:
        yield e


@pytest.fixture(scope="module")
def golden():
    return {name: sc.load_batch(name) for name in NAMES}


def names_of_default():
    return sc.default_names()


def without_big(golden, name="default"):
    """`default` without the 60 kb intron's read, whose two fills take seconds on their own (test_big_intron_alone has it)."""
    b, want, _ = golden[name]
    keep = [i for i, n in enumerate(names_of_default()) if n != "big_intron"]
    return sc.sub_batch(b, want, keep)


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_host_and_fixtures(eng, golden, name):
    b, want = without_big(golden) if name == "default" else golden[name][:2]
    got, info = sc.run_gpu(eng, b)
    ac.assert_same(got, want, name + ": device against the fixtures")
    host, hinfo = sc.run_host(b, threads=8)
    ac.assert_same(got, host, name + ": device against host")
    assert info["splice_counts"] == hinfo["splice_counts"] and info["counts"] == hinfo["counts"]
    if name != "default":
        assert info["splice_counts"] == sc.golden_meta()["batches"][name]["splice_counts"]


def test_big_intron_alone(eng, golden):
    """The read across the 60 kb intron: its fill's state image (13 bytes a target position) is beyond what the DP keeps in LDS, so the job runs in
    the global-image class; both trials of it."""
    b, want, _ = golden["default"]
    i = names_of_default().index("big_intron")
    c, w = sc.sub_batch(b, want, [i])
    before = eng.ksw_class_jobs()
    got, info = sc.run_gpu(eng, c)
    after = eng.ksw_class_jobs()
    ac.assert_same(got, w, "60 kb intron")
    assert any(int(x) & 0xf == 3 and int(x) >> 4 >= sc.BIG_INTRON - 10 for x in got[0][2])
    assert 13 * sc.BIG_INTRON > eng.ksw_info()["lds_max"] > 0
    assert after[1] - before[1] >= 2, "the fill across the intron, once per trial, was not launched in the global-image class"
    assert info["splice_counts"]["fill_intron"] >= 1 and info["splice_counts"]["single_trial"] == 0


def test_batches_in_one_call_shuffled(eng, golden):
    """The batches that share their options, concatenated, read order shuffled: the same answers per read."""
    b, want = sc.concat([without_big(golden), without_big(golden)])
    order = np.random.default_rng(3).permutation(len(b["reads"]))
    c, w = sc.sub_batch(b, want, order)
    got, _ = sc.run_gpu(eng, c)
    ac.assert_same(got, w, "default twice, shuffled")


def test_one_read_and_none(eng, golden):
    b, want, _ = golden["hq"]
    c, w = sc.sub_batch(b, want, [5])
    got, _ = sc.run_gpu(eng, c)
    ac.assert_same(got, w, "one read")
    got, info = eng.align_regs_splice(b["opt"], b["k"], False, b["refs"], [], [], [])
    assert got == [] and not any(info["splice_counts"].values())


def test_spliced_and_unspliced_calls_take_turns(eng, golden):
    """Arena reuse with the splice-aware and the dual-affine form of the DP alternating on one engine: identical bytes each time."""
    sp, sw = sc.sub_batch(*golden["no_flank"][:2], range(12))
    ub, uw = ac.load_batch("inv_pair")
    for turn in range(2):
        got, _ = sc.run_gpu(eng, sp)
        ac.assert_same(got, sw, f"spliced, turn {turn}")
        got, _ = ac.run_gpu(eng, ub)
        ac.assert_same(got, uw, f"unspliced, turn {turn}")


def test_refusals_leave_the_engine_usable(eng, golden):
    b, want, _ = golden["for_only"]
    c, w = sc.sub_batch(b, want, range(4))

    def bad(**kw):
        d = dict(c); d["opt"] = copy.deepcopy(c["opt"])
        for k, v in kw.items():
            setattr(d["opt"] if hasattr(d["opt"], k) else d["opt"].base, k, v)
        return d
    f = c["opt"].base.flag
    for text, x in (("lacks MM_F_SPLICE", bad(flag=f & ~(mm.F_SPLICE | mm.F_SPLICE_FOR))), ("MM_F_SR", bad(flag=f | mm.F_SR)), ("MM_F_EQX", bad(flag=f | mm.F_EQX)),
                    ("MM_F_QSTRAND", bad(flag=f | mm.F_QSTRAND)), ("e must be above 0", bad(e=0)), ("max_sw_mat", bad(max_sw_mat=0)), ("MM2GB_I_HPC", dict(c, hpc=True))):
        with pytest.raises(mm.Mm2gbError, match=text):
            sc.run_gpu(eng, x)
    with pytest.raises(mm.Mm2gbError, match="MM_F_SPLICE"):          # the unspliced device call keeps refusing splice
        eng.align_regs(c["opt"].base, c["k"], False, c["refs"], c["reads"], c["regs"], c["anchors"])
    got, _ = sc.run_gpu(eng, c)
    ac.assert_same(got, w, "after the refusals")


# ---------------------------------------------------------------- the tag text of spliced records on the device (mm2gb_aln_text_splice_gpu)
import aln_text_cases as at  # noqa: E402


@pytest.mark.parametrize("name", sc.TEXT_BATCHES)
def test_text_device_equals_host_and_fixtures(eng, name):
    args, texts = sc.golden_text_args(name), sc.load_texts(name)
    for what in at.WHATS:
        off, text = eng.aln_text_splice(what, *args)
        h_off, h_text = mm.aln_text_splice_host(what, *args, threads=8)
        assert text == h_text and off.tobytes() == h_off.tobytes(), f"{name}: what {what}: device against host"
        at.assert_texts(at.split(off, text), at.want_for(args, texts, what), f"{name}: what {what}")


def test_text_introns_at_the_slice_cuts(eng):
    """A record of more than four slices with an N column just before a cut, as the first column behind a cut and as the second behind one, a
    run of matches open across a cut without N and across an intron (MD keeps it open), on both strands; and short records with N at either end
    of a run.  An intron of 100 000 bases is one column."""
    S = eng.aln_text_info()["slice"]
    long_segs = [("=", S - 1), ("N", 700), ("=", S - 1), ("X", 1), ("N", 5000), ("=", S), ("N", 33), ("=", 2 * S), ("X", 1), ("=", 10), ("N", 100_000), ("=", 3)]
    recs = [sc.build_text(long_segs, seed=5, rev=rev, lead=(2, 3), tail=(1, 4)) for rev in (False, True)]
    recs += [sc.build_text([("=", S), ("N", 2), ("=", S)], seed=6), sc.build_text([("=", S - 2), ("I", 2), ("N", 9), ("D", 1), ("=", S)], seed=7, rev=True)]
    recs += sc.text_recs()
    args = at.batch(recs)
    n_cols = sum(int(w) >> 4 if int(w) & 0xf != 3 else 1 for w in recs[0]["words"])
    assert n_cols > 4 * S and n_cols < 5 * S + 100
    for what in at.WHATS:
        off, text = eng.aln_text_splice(what, *args)
        at.assert_texts(at.split(off, text), at.expected(recs, what), f"what {what}")
        h_off, h_text = mm.aln_text_splice_host(what, *args)
        assert text == h_text and off.tobytes() == h_off.tobytes()


def test_text_refusals_leave_the_engine_usable(eng):
    r = sc.build_text([("=", 5), ("N", 4), ("=", 5)])
    bad = dict(r, words=r["words"].copy(), reg=r["reg"].copy()); bad["words"][1] = 1 << 4 | 3; bad["reg"]["re"] -= 3
    with pytest.raises(mm.Mm2gbError, match="shorter than 2"):
        eng.aln_text_splice(mm.TEXT_CS, *at.batch([bad]))
    with pytest.raises(mm.Mm2gbError, match="CIGAR operation N"):          # the unspliced device call keeps refusing N
        eng.aln_text(mm.TEXT_CS, *at.batch([r]))
    with pytest.raises(mm.Mm2gbError, match="MM2GB_TEXT"):
        eng.aln_text_splice(0x10, *at.batch([r]))
    off, text = eng.aln_text_splice(mm.TEXT_CG | mm.TEXT_CS, *at.batch([r]))
    assert text == b"\tcg:Z:5M4N5M\tcs:Z:" + r["cs"]
    plain = sc.build_text([("=", 20), ("X", 1), ("I", 2), ("=", 20)])      # no N: the plain instantiation behind the spliced entry
    assert eng.aln_text_splice(mm.TEXT_MD, *at.batch([plain]))[1] == eng.aln_text(mm.TEXT_MD, *at.batch([plain]))[1] == b"\tMD:Z:" + plain["md"]


# ---------------------------------------------------------------- the mapper under -x splice (mm2gb_map_reads_splice, mm2gb_map_reads_stream_splice)
@pytest.fixture(scope="module")
def paf_case():
    refs, reads, pafs = sc.load_pafs()
    with mm.SeedIndex([s for _, s in refs], **mm.preset("splice")) as ix:
        yield refs, reads, pafs, ix


def same_paf(got, want, what):
    if got != want:
        g, w = got.splitlines(), want.splitlines()
        bad = [k for k in range(min(len(g), len(w))) if g[k] != w[k]]
        first = bad[0] if bad else min(len(g), len(w))
        at = next((i for i, (x, y) in enumerate(zip(g[first], w[first])) if x != y), None) if bad else None
        raise AssertionError(f"{what}: {len(bad)} of {len(w)} PAF lines differ (got {len(g)}); first: line {first}, byte {at}: "
                             f"{g[first][max((at or 0) - 60, 0):(at or 0) + 60] if bad else None!r} vs {w[first][max((at or 0) - 60, 0):(at or 0) + 60] if bad else None!r}")


def test_recorded_pafs_hold_what_the_tests_rely_on():
    _, reads, pafs = sc.load_pafs()
    lines = pafs["cs"].splitlines()
    assert "\tts:A:+" in pafs["cs"] and "\tts:A:-" in pafs["cs"] and any("\tts:A:" not in ln for ln in lines)
    assert {ln.split("\t")[0] for ln in lines} == {n for n, _ in reads}, "a read left out"
    assert "~" in pafs["cs"] and "\tMD:Z:" in pafs["md"] and "\tcs:Z:=" in pafs["cs_long"] and all("\tcg:Z:" in ln for ln in pafs["c"].splitlines())
    assert len(reads) == sc.golden_meta()["paf"]["reads"] >= 100


@pytest.mark.parametrize("variant", list(sc.PAF_VARIANTS))
def test_paf_identical_to_the_reference(eng, paf_case, variant):
    """The four recorded PAFs of minimap2 -x splice --cap-sw-mem=100000000, with the alignment call and the text call each on the device and on host threads."""
    refs, reads, pafs, ix = paf_case
    for align_on_device in (1, -1):
        for text_on_device in (1, -1):
            al = mm.map_splice([s for _, s in refs], align_on_device=align_on_device, text_on_device=text_on_device, **sc.PAF_KW[variant])
            paf, st = mm.map_reads(eng, ix, [n for n, _ in refs], reads, opt=mm.map_opt_splice(), k=15, align=al)
            same_paf(paf, pafs[variant], f"{variant}, alignment {align_on_device}, text {text_on_device}")
            assert st["n_reads"] == len(reads) and st["n_rechained"] == 0 and all(key in st for key in ("s_align", "s_post_align", "s_text"))


@pytest.mark.parametrize("seeds_on_device, seeding_on_device", [(-1, 0), (1, 0), (1, 1)])
def test_paf_with_seeds_and_seeding_on_either_side(eng, paf_case, seeds_on_device, seeding_on_device):
    refs, reads, pafs, ix = paf_case
    opt = mm.map_opt_splice(seeds_on_device=seeds_on_device, seeding_on_device=seeding_on_device)
    paf, _ = mm.map_reads(eng, ix, [n for n, _ in refs], reads, opt=opt, k=15, align=mm.map_splice([s for _, s in refs], cs="short"))
    same_paf(paf, pafs["cs"], f"seeds {seeds_on_device}, seeding {seeding_on_device}")


def test_a_stream_of_chunks(eng, paf_case):
    refs, reads, pafs, ix = paf_case
    with mm.Engine(device=0) as e2:
        for text_on_device in (1, -1):
            al = mm.map_splice([s for _, s in refs], cs="long", text_on_device=text_on_device)
            paf, st = mm.map_reads_stream([eng, e2], ix, [n for n, _ in refs], reads, opt=mm.map_opt_splice(host_threads=8), k=15, chunk_bases=12_000, align=al)
            same_paf(paf, pafs["cs_long"], f"stream, text {text_on_device}")
            assert st["n_reads"] == len(reads) and st["s_align"] > 0
        assert mm.map_reads_stream([eng, e2], ix, [n for n, _ in refs], [], opt=mm.map_opt_splice(), align=al)[0] == ""


def test_mapper_refusals(eng, paf_case):
    refs, reads, pafs, ix = paf_case
    names = [n for n, _ in refs]
    with pytest.raises(mm.Mm2gbError, match="MM_F_SPLICE"):          # the unspliced mapper call keeps refusing a splice flag
        mm.map_reads(eng, ix, names, reads[:3], k=15, align=mm.map_align([s for _, s in refs], flag=mm.F_SPLICE))
    with pytest.raises(mm.Mm2gbError, match="lacks MM_F_SPLICE"):
        mm.map_reads(eng, ix, names, reads[:3], opt=mm.map_opt_splice(), k=15, align=mm.map_splice([s for _, s in refs], flag=0))
    al = mm.map_splice([s for _, s in refs]); al.what = 0x40
    with pytest.raises(mm.Mm2gbError, match="MM2GB_TEXT"):
        mm.map_reads(eng, ix, names, reads[:3], opt=mm.map_opt_splice(), k=15, align=al)
    with pytest.raises(mm.Mm2gbError, match="another number of reference sequences"):
        mm.map_reads(eng, ix, names, reads[:3], opt=mm.map_opt_splice(), k=15, align=mm.map_splice([]))
    o = mm.map_opt_splice()
    assert (o.bw, o.bw_long, o.max_gap_ref, o.max_gap) == (200000, 200000, 200000, 2000) and o.min_cnt == mm.map_opt().min_cnt
    paf, _ = mm.map_reads(eng, ix, names, reads[:3], opt=o, k=15, align=mm.map_splice([s for _, s in refs]))
    same_paf(paf, "".join(ln + "\n" for ln in pafs["c"].splitlines() if ln.split("\t")[0] in {n for n, _ in reads[:3]}), "after the refusals")
