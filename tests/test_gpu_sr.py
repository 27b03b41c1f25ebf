"""Short single-end reads on the device.  The mapper (mm2gb_map_reads_sr / _stream_sr) against the reference program's PAFs of tests/golden/sr, byte for byte, without
and with base-level alignment, seeded on the host and on the device.  The alignment of hits under MM_F_SR (mm2gb_align_regs_sr_gpu: k_al_ungapped for every fill's first
pass) against the host form, which tests/test_sr_cpu.py pins to the reference's mm_align_skeleton, on the fixture and on crafted single-chain batches.  The heap order of seed
collection on the device (csrc/seed_heap_kernels.hip, mm2gb_collect_seeds_heap_gpu) against the host form, the recording and the plain-Python restatement on crafted matches:
reads of 0 and 1 hit, three seeds on one five-hit list, reads just under, at and just over the one-wave bound, a long read with a tie.  Every comparison is exact."""
import os

import numpy as np
import pytest

import align_cases as ac
import sr_cases as sc

pytestmark = pytest.mark.gpu

mm = pytest.importorskip("mm2gb_amd")
HEAP_FLAG = mm.F_SR | mm.F_FRAG_MODE | mm.F_NO_PRINT_2ND | mm.F_HEAP_SORT


@pytest.fixture(scope="module")
def engine():
    with mm.Engine() as e:
        yield e


@pytest.fixture(scope="module")
def fixture_matches():
    return sc.matches([s for _, s in sc.reads()])


def same(got, want, names):
    assert len(got) == len(want) == len(names)
    for n, a, b in zip(names, got, want):
        assert a.shape == b.shape and np.array_equal(a, b), n


def test_fixture_equals_host_form_and_recording(engine, fixture_matches):
    names = [n for n, _ in sc.reads()]
    want, host_tied = mm.collect_seeds_heap_host(HEAP_FLAG, fixture_matches)
    got, n_tied = engine.collect_seeds_heap(HEAP_FLAG, fixture_matches)
    same(got, want, names)
    assert n_tied == host_tied and 0 < n_tied < len(names)
    rec = sc.gold()["seeds"]
    for n, a in zip(names, got):
        assert sc.sd_rows(a) == rec[n]["sd"], n


@pytest.mark.parametrize("flag", [0, 0x100000, 0x200000], ids=["both", "for_only", "rev_only"])
def test_crafted_reads(engine, flag):
    cases = sc.crafted_reads(np.random.default_rng(7))
    reads = list(cases.values())
    want, host_tied = mm.collect_seeds_heap_host(flag, reads)
    got, n_tied = engine.collect_seeds_heap(flag, reads)
    same(got, want, list(cases))
    same(got, [sc.heap_literal(rd, flag) for rd in reads], list(cases))
    assert n_tied == host_tied == 3 and 0 < n_tied < len(reads)
    if flag == 0:
        assert [len(a) for a in got][:2] == [0, 1] and [len(a) for a in got][4:7] == [sc.WAVE_HITS - 1, sc.WAVE_HITS, sc.WAVE_HITS + 1]
        # the long reads' order with nothing done again: the sort alone gives the heap's order where no cr repeats
        alone, t = engine.collect_seeds_heap(flag, [cases["wave_plus_1"], cases["no_seed"], cases["odd_65"]])
        assert t == 0
        same(alone, [want[6], want[0], want[8]], ["wave_plus_1", "no_seed", "odd_65"])


def test_one_read_batches_and_empty_batches(engine):
    cases = sc.crafted_reads(np.random.default_rng(11))
    for name, rd in cases.items():
        got, _ = engine.collect_seeds_heap(0, [rd])
        same(got, [sc.heap_literal(rd)], [name])
    got, n_tied = engine.collect_seeds_heap(0, [cases["no_seed"], cases["no_seed"]])
    assert n_tied == 0 and [len(a) for a in got] == [0, 0]


def test_name_tests(engine):
    five = [sc.hit(p) for p in (40, 90, 150, 2_000, 2_060)]
    rd = sc.read_of([sc.seed(5, 40), sc.seed(5, 90), sc.seed(2, 170, 1)], [five, five, [sc.hit(1_000), sc.hit(170, 1)]], 250)
    other = sc.read_of([sc.seed(2, 30)], [[sc.hit(700), sc.hit(900)]], 120)
    ref_len, ref_rank = [250], [1]
    for q_rank, flag in ((1, mm.F_NO_DIAG), (1, mm.F_NO_DIAG | mm.F_NO_DUAL), (2, mm.F_NO_DUAL), (0, mm.F_NO_DUAL)):
        reads = [dict(rd, q_rank=q_rank), dict(other, q_rank=0)]
        got, _ = engine.collect_seeds_heap(flag, reads, ref_len=ref_len, ref_rank=ref_rank)
        same(got, [sc.heap_literal(r, flag, ref_len, ref_rank) for r in reads], [f"rank{q_rank}", "other"])


def test_refusals(engine, fixture_matches):
    with pytest.raises(mm.Mm2gbError, match="MM_F_QSTRAND is not supported"):
        engine.collect_seeds_heap(0x100000000, fixture_matches[:2])
    # the existing calls still refuse the preset's bits
    names, seqs = ["ref"], sc.reads()[:3]
    with pytest.raises(mm.Mm2gbError, match="of mm_mapopt_t::flag only"):
        mm.map_reads(engine, sc.index(), names, seqs, opt=mm.map_opt_sr(), k=21)
    with pytest.raises(mm.Mm2gbError, match="not supported"):
        mm.map_opt_preset("sr")


# ---------------------------------------------------------------- alignment of hits under MM_F_SR (mm2gb_align_regs_sr_gpu, k_al_ungapped)
def test_ungapped_fills_on_crafted_chains(engine):
    """One chain per read on one diagonal, caller-made anchors: stretches of 1, 63, 64, 65, 128, 129, 255, 300 and 1000 columns (where the kernel's 64-column steps begin
    and end), a drop across a step's boundary, the walk's tie at the maximum, every column a mismatch, N in the query, the target and both, a drop of exactly zdrop (the
    ungapped word stands) and of zdrop + 1 (the fill runs again as a DP): records, rows, words and counts equal the host form's."""
    cases = sc.ungapped_cases(np.random.default_rng(11))
    b = sc.ungapped_batch(cases)
    want, winfo = sc.run_sr_host(b)
    got, info = sc.run_sr_gpu(engine, b)
    ac.assert_same(got, want, "crafted chains")
    assert info["sr_counts"] == winfo["sr_counts"] == dict(fill_ungapped=13, fill_rerun=4, stretch_short=0)
    for k in ("fill_one_pass", "fill_two_pass", "split", "split_refused", "jobs", "cells", "left_end", "right_end", "seam_merged"):
        assert info["counts"][k] == winfo["counts"][k], k
    # every case alone: a round of one fill, and the two extensions beside it
    for i, n in enumerate(cases):
        one = dict(b, refs=[b["refs"][i]], reads=[b["reads"][i]], regs=[cases[n][2]], anchors=[cases[n][3]])
        g1, _ = sc.run_sr_gpu(engine, one)
        w1, _ = sc.run_sr_host(one)
        ac.assert_same(g1, w1, n)


def test_alignment_of_the_fixture_equals_the_recording(engine):
    batch, want = sc.golden_aligned()
    _, winfo = sc.run_sr_host(batch)
    got, info = sc.run_sr_gpu(engine, batch)
    ac.assert_same(got, want, "fixture")
    assert info["sr_counts"] == winfo["sr_counts"] and info["sr_counts"]["fill_rerun"] >= 2 and info["sr_counts"]["stretch_short"] >= 1 and info["counts"]["split"] == winfo["counts"]["split"] >= 2


def test_alignment_refusals(engine):
    batch, _ = sc.golden_aligned()
    few = {k: (v[:3] if k in ("reads", "regs", "anchors") else v) for k, v in batch.items()}
    go = lambda fn, opt, hpc=False: fn(opt, few["k"], hpc, few["refs"], few["reads"], few["regs"], few["anchors"])
    with pytest.raises(mm.Mm2gbError, match="lacks MM_F_SR"):
        go(engine.align_regs_sr, mm.align_sr_opt(flag=0))
    with pytest.raises(mm.Mm2gbError, match="MM2GB_I_HPC"):
        go(engine.align_regs_sr, mm.align_sr_opt(), True)
    # the existing calls still refuse MM_F_SR by name
    with pytest.raises(mm.Mm2gbError, match="MM_F_SR is not supported"):
        go(engine.align_regs, mm.align_opt("map-ont", flag=mm.F_SR))
    with pytest.raises(mm.Mm2gbError, match="MM_F_SR is not supported"):
        go(engine.align_regs_extz, mm.align_opt("map-ont", q2=4, e2=2, flag=mm.F_SR))
    with pytest.raises(mm.Mm2gbError, match="MM_F_SR is not supported"):
        go(engine.align_regs_splice, mm.align_splice_opt(flag=0x80 | mm.F_SR))


# ---------------------------------------------------------------- the mapper (mm2gb_map_reads_sr)
RESCUED = None


def check_run(run, text, st):
    assert text == sc.golden_paf(run)
    assert st["n_reads"] == 209 and st["n_mapped"] == len({ln.split("\t")[0] for ln in text.splitlines()})
    assert st["n_rechained"] == 0 and st["n_rmq_tied"] == 0
    if run in ("sr",) + sc.ALIGNED:
        assert st["n_tied_reads"] == 9 and st["n_rescued"] == 0 and "tp:A:S" not in text and st["n_chain_calls"] >= 5
    if run == "sr":
        assert "dv:f" not in text and st["sr_counts"] == dict(fill_ungapped=0, fill_rerun=0, stretch_short=0)
    if run in sc.ALIGNED:
        assert st["sr_counts"]["fill_rerun"] >= 2 and st["sr_counts"]["fill_ungapped"] >= 200 and st["sr_counts"]["stretch_short"] >= 1
    if run == "sr.2nd":
        assert "tp:A:S" in text
    if run == "sr.sorted":
        assert st["n_tied_reads"] == 0
    rescued = {ln.split("\t")[0] for ln in sc.golden_paf("sr.f4_50").splitlines()} - {ln.split("\t")[0] for ln in sc.golden_paf("sr.f4_4").splitlines()}
    if run == "sr.f4_50":
        assert len(rescued) >= 2 and st["n_rescued"] >= len(rescued)
    if run == "sr.f4_4":
        assert st["n_rescued"] == 0


@pytest.mark.parametrize("seeding_on_device", [0, 1], ids=["seed_host", "seed_device"])
@pytest.mark.parametrize("run", [r for r in sc.RUNS if r not in sc.ALIGNED])
def test_paf_identical_to_the_reference(engine, run, seeding_on_device):
    """Byte for byte what minimap2 -t 1 <run's arguments> printed: five read lengths (several max_dist_x groups and the max_gap floor), the tandem array's reads (the
    heap's tie order decides their chains' anchors), the rescue at -f 4,50, secondaries printed and suppressed, anchors sorted instead (--heap-sort=no); seeded on host
    threads and on the device, where the heap-order collection reads the resident matches."""
    text, st = sc.map_run(engine, run, seeding_on_device=seeding_on_device)
    check_run(run, text, st)


@pytest.mark.parametrize("align_on_device", [1, -1], ids=["align_device", "align_host"])
@pytest.mark.parametrize("seeding_on_device", [0, 1], ids=["seed_host", "seed_device"])
@pytest.mark.parametrize("run", list(sc.ALIGNED))
def test_aligned_paf_identical_to_the_reference(engine, run, seeding_on_device, align_on_device):
    """minimap2 -x sr -c, -c --cs and --cs=long --MD -c: the reads with a substituted middle split into two lines, no secondary line is printed."""
    text, st = sc.map_run(engine, run, seeding_on_device=seeding_on_device, align_on_device=align_on_device, text_on_device=align_on_device)
    check_run(run, text, st)


def test_host_side_settings_and_anchors_uploaded(engine):
    """seeds_on_device: the heap-order collection from the host's matches on host threads (-1) and through mm2gb_collect_seeds_heap_gpu (1); seeding_on_device = 2 is 1."""
    for kw in (dict(seeds_on_device=-1), dict(seeds_on_device=1), dict(seeding_on_device=2)):
        for run in ("sr.c", "sr.f4_50"):
            text, st = sc.map_run(engine, run, **kw)
            check_run(run, text, st)


@pytest.mark.parametrize("run", ["sr", "sr.csmd", "sr.f4_50"])
def test_stream_form(engine, run):
    """mm2gb_map_reads_stream_sr in chunks of about 5000 bases: the same bytes, the counts summed over the chunks."""
    text, st = sc.map_run(engine, run, stream=True)
    whole, wst = sc.map_run(engine, run)
    assert text == whole == sc.golden_paf(run)
    assert st["n_reads"] == 209 and st["n_tied_reads"] == wst["n_tied_reads"] and st["sr_counts"] == wst["sr_counts"] and st["n_chain_calls"] > wst["n_chain_calls"]


def test_one_length_batch_and_empty_batch(engine):
    """Reads of one length make one chaining call over the batch as it lies (no gather): the same lines as in the mixed batch."""
    want = [ln for ln in sc.golden_paf("sr").splitlines() if ln.split("\t")[1] == "150"]
    reads = [(n, s) for n, s in sc.reads() if len(s) == 150]
    text, _ = mm.map_reads(engine, sc.index(), ["ref"], reads, opt=mm.map_opt_sr(host_threads=2), k=21, align=mm.map_sr())
    assert len(want) >= 15
    assert text.splitlines() == want
    text, st = mm.map_reads(engine, sc.index(), ["ref"], [], opt=mm.map_opt_sr(), k=21, align=mm.map_sr())
    assert text == "" and st["n_reads"] == 0


def test_mapper_refusals(engine):
    reads = sc.reads()[:4]
    go = lambda opt, sr, ix=None: mm.map_reads(engine, ix or sc.index(), ["ref"], reads, opt=opt, k=21, align=sr)
    with pytest.raises(mm.Mm2gbError, match="needs refs"):
        mm.map_sr(align=True)
    with pytest.raises(mm.Mm2gbError, match="align is 0"):
        go(mm.map_opt_sr(), mm.map_sr(cs="short"))
    with pytest.raises(mm.Mm2gbError, match="MM_F_EQX"):
        go(mm.map_opt_sr(), mm.map_sr([sc.gold()["genome"].encode()], align=True, flag=mm.map_opt_sr().flag | 0x4000000))
    with pytest.raises(mm.Mm2gbError, match="MM_F_RMQ"):
        go(mm.map_opt_sr(flag=mm.map_opt_sr().flag | mm.F_RMQ), mm.map_sr())
    with pytest.raises(mm.Mm2gbError, match="MM_F_QSTRAND"):
        go(mm.map_opt_sr(flag=mm.map_opt_sr().flag | 0x100000000), mm.map_sr())
    with pytest.raises(mm.Mm2gbError, match="MM_F_NO_DIAG"):
        go(mm.map_opt_sr(flag=mm.map_opt_sr().flag | mm.F_NO_DIAG), mm.map_sr())
    with pytest.raises(mm.Mm2gbError, match="do not carry MM_F_SR"):
        go(mm.map_opt(), mm.map_sr())
    hpc = mm.SeedIndex([sc.gold()["genome"].encode()], k=21, w=11, hpc=True)
    with pytest.raises(mm.Mm2gbError, match="homopolymer-compressed index"):
        go(mm.map_opt_sr(), mm.map_sr(), hpc)
    with pytest.raises(mm.Mm2gbError, match="of mm_mapopt_t::flag only"):
        mm.map_reads_stream([engine], sc.index(), ["ref"], reads, opt=mm.map_opt_sr(), k=21)


@pytest.mark.skipif(not os.path.exists(sc.REF_EXE), reason="the reference program is built only where its checkout exists")
def test_fresh_reads_against_the_reference_program(engine):
    """300 fresh reads of 100-250 bases (about 150 distinct lengths: as many chaining calls over gathered anchors), a third of them from the tandem array and a sixth
    from the repeat family, at -f 4,50 so that the rescue runs: every read's lines equal the program's, none left out."""
    rng = np.random.default_rng(2025)
    g = np.frombuffer(sc.gold()["genome"].encode(), np.uint8)
    reads = []
    for r in range(300):
        n = int(rng.integers(100, 251))
        st = sc.TANDEM[0] + int(rng.integers(0, 1_300)) if r % 3 == 0 else 14_000 + int(rng.integers(0, 12)) * 3_500 + int(rng.integers(0, 150)) if r % 6 == 1 else int(rng.integers(0, len(g) - n))
        s = sc.sim_reads.mutate(rng, g[st:st + n], float(rng.uniform(0.005, 0.02)))
        reads.append((f"fresh{r}", (sc.sim_reads.revcomp(s) if rng.random() < 0.5 else s).tobytes()))
    want = sc.record_paf(sc.gold()["genome"].encode(), reads, ["-x", "sr", "-f", "4,50"])
    got, st = mm.map_reads(engine, sc.index(), ["ref"], reads, opt=mm.map_opt_sr(mid_occ=4, host_threads=4), k=21, align=mm.map_sr(max_occ=50))
    assert got == want
    assert st["n_rescued"] > 0 and st["n_tied_reads"] > 0 and len(want.splitlines()) >= 250
    # ... and with base-level alignment, seeded on the device
    want = sc.record_paf(sc.gold()["genome"].encode(), reads, ["-x", "sr", "--cs=long", "--MD", "-c"])
    got, st = mm.map_reads(engine, sc.index(), ["ref"], reads, opt=mm.map_opt_sr(host_threads=4, seeding_on_device=1), k=21,
                           align=mm.map_sr([sc.gold()["genome"].encode()], align=True, cs="long", md=True))
    assert got == want and st["sr_counts"]["fill_ungapped"] >= 250
