"""The HiFi and assembly presets on the device: the DP kernel at the presets' scores, the alignment call with their options, the RMQ kernels on a
contig's raw anchors (the first chainer of MM_F_RMQ: bw = 1000, max_gap = 10000), and the mapper against the PAF the reference's CPU program printed
(tests/golden/asm, recorded by tests/tools/gen_golden_asm.py) byte for byte."""
import numpy as np
import pytest

import align_cases as ac
import asm_cases as am
import ksw_cases as kc

pytestmark = pytest.mark.gpu

import mm2gb_amd as mm  # noqa: E402


@pytest.fixture(scope="module")
def engine():
    with mm.Engine() as e:
        yield e


def test_dp_kernel_at_the_presets_scores(engine):
    """3 000 jobs per preset tuple from LENS_GPU against the host form, then the recorded answers of the reference."""
    rng = np.random.default_rng(13)
    for k, p in enumerate(am.ksw_params()):
        jobs, q, t = kc.make_batch(rng, p.m, 3000, kc.LENS_GPU, p_empty=0.02)
        kc.assert_same(engine.ksw_extd2_batch(p, jobs, q, t), mm.ksw_extd2_host_batch(p, jobs, q, t, threads=16), f"tuple of {am.PRESETS[k]}", jobs)
    for k, (p, jobs, q, t, want) in enumerate(am.golden_ksw()):
        kc.assert_same(engine.ksw_extd2_batch(p, jobs, q, t), want, f"fixture set {am.PRESETS[k]}", jobs)


@pytest.mark.parametrize("preset", am.PRESETS)
def test_align_regs_with_the_presets_options(engine, preset):
    b, want = am.load_align(preset)
    b["opt"] = mm.align_opt(preset)
    got = ac.run_gpu(engine, b)[0]
    ac.assert_same(got, ac.run_host(b, threads=8)[0], preset + ": device against host")
    ac.assert_same(got, want, preset + ": device against the recorded vectors")


def test_align_regs_squeezes_a_contigs_anchors(engine):
    """The plain contig with every anchor the chaining kept, those no record holds included: mm_squeeze_a inside the call moves them."""
    b, want = am.load_align("unsqueezed_asm10")
    assert sum(len(a) for a in b["anchors"]) > 4 * sum(int(r["cnt"].sum()) for r in b["regs"])
    b["opt"] = mm.align_opt("asm10")
    ac.assert_same(ac.run_gpu(engine, b)[0], want, "unsqueezed: device against the recorded vectors")


@pytest.fixture(scope="module")
def raw_anchors():
    refs, contigs = am.load_sim()
    return am.own_anchors([s for _, s in refs], [s for _, s in contigs["d3"]] + [s for _, s in contigs["d8"]], "asm10")


@pytest.mark.parametrize("skip", list(am.SKIPS))
def test_rmq_kernels_on_raw_anchors(engine, raw_anchors, skip):
    """Engine.rmq_chain (reads without a deciding tie) and Engine.rmq_chain_exact (every read) against rmq_chain_host."""
    prm = am.to_lib(am.rmq_param_first(am.SKIPS[skip]))
    allr, off = np.concatenate(raw_anchors), am.offsets_of(raw_anchors)
    host, _ = mm.rmq_chain_host(allr, off, prm, threads=8)
    got, tied, _ = engine.rmq_chain(allr, off, prm)
    for r in range(len(raw_anchors)):
        if not tied[r]:
            assert np.array_equal(got[r][0], host[r][0]) and np.array_equal(got[r][1], host[r][1]), (skip, r)
    exact, where, _ = engine.rmq_chain_exact(allr, off, prm, threads=8)
    am.same_chains(exact, host, f"rmq_chain_exact, skip {skip}")
    assert all(len(h[0]) > 0 for h in host)


def run_mapper(engine, pair, preset, skip, variant, index_engine=None, stream=None, align_on_device=0, text_on_device=0, **opt_kw):
    refs, reads = am.pair_inputs(pair)
    al = mm.map_align([s for _, s in refs], preset=preset, cs="short" if variant == "cs" else None, align_on_device=align_on_device, text_on_device=text_on_device)
    opt = mm.map_opt_preset(preset, max_chain_skip=am.SKIPS[skip], **opt_kw)
    with mm.SeedIndex([s for _, s in refs], engine=index_engine, **mm.preset(preset)) as ix:
        if stream:
            return mm.map_reads_stream(stream, ix, [n for n, _ in refs], reads, opt=opt, k=19, chunk_bases=stream_chunk(reads), align=al)
        return mm.map_reads(engine, ix, [n for n, _ in refs], reads, opt=opt, k=19, align=al)


def stream_chunk(reads):
    return sum(len(s) for _, s in reads) // 2


@pytest.mark.parametrize("pair,preset,skip,variant", am.paf_cases(), ids=[am.paf_key(*c) for c in am.paf_cases()])
def test_paf_identical_to_the_reference(engine, pair, preset, skip, variant):
    """Every recorded set.  The two sim_d8.asm5 cases take about 30 s each, all of it in the alignment call (asm5's b = 19 and zdrop 200 at 8 %: a drop
    and a further round every few hundred bases); every other case takes up to a few seconds."""
    want = am.golden_paf(pair, preset, skip, variant)
    paf, st = run_mapper(engine, pair, preset, skip, variant)
    am.same_paf(paf, want, am.paf_key(pair, preset, skip, variant))
    assert (want == "") == ((pair, preset) == ("sim_" + am.EMPTY[0], am.EMPTY[1]) or (pair, preset) == ("mt", "asm5"))
    assert st["n_reads"] == len(am.pair_inputs(pair)[1])


FORMS = {"rechain_device": dict(rechain_on_device=1), "rechain_host": dict(rechain_on_device=-1), "align_host": dict(align_on_device=-1), "text_device": dict(text_on_device=1),
         "seeding_device": dict(seeding_on_device=1), "index_device": dict(index_engine=True), "stream": dict(stream=True)}


FORM_SET = "sim_d05"          # asm10's PAF of this set differs between the two skips


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("skip", list(am.SKIPS))
def test_every_form_gives_the_same_bytes(engine, form, skip):
    """The asm10 contigs at 0.5 % (an inversion record, a bridged deletion, re-chained contigs, and bytes that depend on max-chain-skip) through each
    other form of the stages.  At skip 25 the device's RMQ form is the one-anchor-per-step kernel and every tie goes to the host form."""
    kw = dict(FORMS[form])
    want = am.golden_paf(FORM_SET, "asm10", skip, "cs")
    assert "tp:A:I" in want and want != am.golden_paf(FORM_SET, "asm10", "s25" if skip == "inf" else "inf", "cs")
    if kw.pop("index_engine", None):
        kw["index_engine"] = engine
    if kw.pop("stream", None):
        with mm.Engine() as e2:
            paf, st = run_mapper(engine, FORM_SET, "asm10", skip, "cs", stream=[engine, e2], host_threads=8)
    else:
        paf, st = run_mapper(engine, FORM_SET, "asm10", skip, "cs", **kw)
    am.same_paf(paf, want, f"{form}, skip {skip}")
    assert st["n_reads"] == 4


def test_reads_without_anchors_come_through(engine):
    """One read of random bases (no anchor), one contig, one read of 25 bases -- and a batch in which no read has an anchor."""
    refs, contigs = am.load_sim()
    rng = np.random.default_rng(3)
    junk = ("junk", bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 3000)]))
    ctg = contigs["d3"][3]
    batch = [junk, ctg, ("tiny", ctg[1][:25])]
    al = mm.map_align([s for _, s in refs], preset="asm10")
    with mm.SeedIndex([s for _, s in refs], **mm.preset("asm10")) as ix:
        names = [n for n, _ in refs]
        for rechain_on_device in (0, 1, -1):
            opt = mm.map_opt_preset("asm10", rechain_on_device=rechain_on_device)
            alone, _ = mm.map_reads(engine, ix, names, [ctg], opt=opt, k=19, align=al)
            paf, st = mm.map_reads(engine, ix, names, batch, opt=opt, k=19, align=al)
            assert paf == alone and alone.startswith(ctg[0] + "\t") and st["n_reads"] == 3 and st["n_mapped"] == 1
            none, st = mm.map_reads(engine, ix, names, [junk, ("junk2", junk[1][::-1])], opt=opt, k=19, align=al)
            assert none == "" and st["n_anchors"] == 0 and st["n_chains"] == 0
            few, st = mm.map_reads(engine, ix, names, [junk, batch[2]], opt=opt, k=19, align=al)          # at most an anchor or two, no chain
            assert few == "" and st["n_chains"] == 0
            plain, _ = mm.map_reads(engine, ix, names, batch, opt=opt, k=19)          # without an alignment: the same stages 1-5
            assert len(plain.splitlines()) >= 1 and all(ln.startswith(ctg[0] + "\t") for ln in plain.splitlines())


def test_refusals(engine):
    refs, reads = am.pair_inputs("inv")
    names, seqs = [n for n, _ in refs], [s for _, s in refs]
    with mm.SeedIndex(seqs, **mm.preset("splice")) as ix:
        with pytest.raises(mm.Mm2gbError, match="MM_F_RMQ"):
            mm.map_reads(engine, ix, names, reads, opt=mm.map_opt_splice(flag=mm.F_RMQ), k=15, align=mm.map_splice(seqs))
        with pytest.raises(mm.Mm2gbError, match="MM_F_RMQ"):
            mm.map_reads_stream([engine], ix, names, reads, opt=mm.map_opt_splice(flag=mm.F_RMQ), k=15, align=mm.map_splice(seqs))
        with pytest.raises(mm.Mm2gbError, match="only MM_F_FOR_ONLY and MM_F_REV_ONLY are supported"):
            mm.map_reads(engine, ix, names, reads, opt=mm.map_opt(flag=mm.F_RMQ | 0x1))
