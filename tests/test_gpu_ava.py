"""Read-against-read overlap on the device: the mapper's PAF byte for byte against the runs recorded from the reference program (tests/golden/ava) in its
staged forms and on the resident path, the stream form, the fall-back where the options have a re-chaining stage, and k_est_err against mm2gb_est_err_host."""
import numpy as np
import pytest

import ava_cases as av
import mm2gb_amd as mm
from asm_cases import same_paf

pytestmark = pytest.mark.gpu

FORMS = {"host_seeding": dict(seeds_on_device=-1), "seeds_on_device": dict(seeds_on_device=1), "seeding_on_device": dict(seeding_on_device=1),
         "resident": dict(seeding_on_device=mm.SEEDING_RESIDENT)}


@pytest.fixture(scope="module")
def engine():
    with mm.Engine(device=0) as e:
        yield e


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("run", list(av.RUNS))
def test_paf_equals_the_reference(engine, run, form):
    got, st = av.map_run(engine, run, "inf", **FORMS[form])
    same_paf(got, av.golden_paf(run, "inf"), f"{run} {form}")
    assert st["n_rechained"] == 0 and st["n_chains"] >= len(got.splitlines()) > 0 and st["n_anchors"] > 0


@pytest.mark.parametrize("form", ["host_seeding", "resident"])
@pytest.mark.parametrize("run", list(av.RUNS))
def test_paf_with_a_finite_skip_limit(engine, run, form):
    got, _ = av.map_run(engine, run, "s25", **FORMS[form])
    same_paf(got, av.golden_paf(run, "s25"), f"{run} {form} at max-chain-skip 25")


@pytest.mark.parametrize("form", ["host_seeding", "resident"])
def test_stream_form(engine, form):
    got, st = av.map_run(engine, "a.ava-ont", "inf", stream=True, **FORMS[form])         # several chunks: the ranks are the call's, not a chunk's
    same_paf(got, av.golden_paf("a.ava-ont", "inf"), f"stream {form}")
    assert st["n_reads"] == len(av.read_set("a"))


def test_resident_says_which_path_ran(engine, capfd, monkeypatch):
    monkeypatch.setenv("MM2GB_DEBUG_PHASES", "1")
    av.map_run(engine, "a.ava-ont", "inf", **FORMS["resident"])
    assert "map path: resident" in capfd.readouterr().err
    av.map_run(engine, "a.ava-ont", "inf", **FORMS["seeding_on_device"])
    assert "map path: staged" in capfd.readouterr().err


def test_resident_falls_back_where_there_is_re_chaining(engine, capfd, monkeypatch):
    """map-ont defaults (bw_long > bw, no MM_F_NO_LJOIN): asking for the resident path has no effect and the lines are those of the staged path."""
    reads, names = av.read_set("a"), [n for n, _ in av.read_set("a")]
    with mm.SeedIndex([s for _, s in reads], k=15, w=10, threads=4) as ix:
        want, st0 = mm.map_reads(engine, ix, names, reads, opt=mm.map_opt(host_threads=4, seeding_on_device=1))
        monkeypatch.setenv("MM2GB_DEBUG_PHASES", "1")
        got, st1 = mm.map_reads(engine, ix, names, reads, opt=mm.map_opt(host_threads=4, seeding_on_device=mm.SEEDING_RESIDENT))
    assert "map path: staged (resident asked for: the options do not allow it)" in capfd.readouterr().err
    assert got == want and len(want.splitlines()) > 40 and "tp:A:P" in want
    assert (st0["n_chains"], st0["n_rechained"]) == (st1["n_chains"], st1["n_rechained"])


def test_calls_with_alignment_refuse_the_bits(engine):
    reads = av.read_set("a")[:3]
    refs = [s for _, s in reads]
    with mm.SeedIndex(refs, k=15, w=10, threads=2) as ix:
        with pytest.raises(mm.Mm2gbError, match="mm2gb_map_reads_aln: MM_F_ALL_CHAINS is not supported"):
            mm.map_reads(engine, ix, [n for n, _ in reads], reads, opt=mm.map_opt(flag=av.X_BITS), align=mm.map_align(refs))
        with pytest.raises(mm.Mm2gbError, match="mm2gb_map_reads_aln: MM_F_NO_DUAL is not supported"):
            mm.map_reads_stream([engine], ix, [n for n, _ in reads], reads, opt=mm.map_opt(flag=mm.F_NO_DUAL), align=mm.map_align(refs))
        got, _ = mm.map_reads(engine, ix, [n for n, _ in reads], reads, opt=mm.map_opt(flag=mm.F_NO_LJOIN, host_threads=2), align=mm.map_align(refs))
        assert "cg:Z:" in got


# ---------------------------------------------------------------- k_est_err
def same_est(engine, reads, ref_len):
    want = mm.est_err_host(reads, ref_len, threads=8)
    got = engine.est_err(reads, ref_len)
    for r, (g, w) in enumerate(zip(got, want)):
        assert g["sum_k"] == w["sum_k"], r
        assert np.array_equal(g["n_match"], w["n_match"]) and np.array_equal(g["n_tot"], w["n_tot"]), (r, g, w)
        assert g["div"].tobytes() == w["div"].tobytes(), r
    return want


def test_est_err_crafted(engine):
    reads, ref_len, _ = av.crafted_reads()
    same_est(engine, reads, ref_len)


def test_est_err_lane_wave_and_block_seams(engine):
    rng = np.random.default_rng(7)
    lens = [1, 63, 64, 65, 4097]
    for absent in (0, 2):
        rd = av.synthetic_read(rng, 6000, lens, gap_hi=1, absent_every=absent)
        want = same_est(engine, [rd], [100_000])
        if not absent:
            assert want[0]["n_match"].tolist() == lens


def test_est_err_many_reads(engine):
    rng = np.random.default_rng(11)
    reads = [av.synthetic_read(rng, int(rng.integers(1, 3000)), [int(v) for v in rng.integers(1, 150, int(rng.integers(0, 201)))], gap_hi=5, absent_every=7) for _ in range(300)]
    want = same_est(engine, reads, [100_000])
    assert sum(len(w["div"]) for w in want) > 20_000 and any((w["n_tot"] < 0).any() for w in want)


def test_est_err_crafted_long(engine):
    """The walk's cases at the sizes of k_est_err<64>: a defect of each kind at k = 1, 63, 64, 65 and cnt - 1 of hits of 64 to 200 anchors, two defects in different
    rounds, chains that go on beyond the read's last minimizer, reads whose mini_pos is not strictly ascending (the literal walk in both instantiations),
    coordinates near 2^31 and the comparisons against avg_k at equality."""
    reads, ref_len, what = av.crafted_long()
    want = same_est(engine, reads, ref_len)
    by = dict(zip(what, want))
    assert by["two defects, 70 and 100"]["n_match"].tolist() == [70] * 8 and by["cnt 200 reverse"]["n_match"].tolist()[:5] == [200, 1, 63, 64, 65]
    one_at_a_time = [same_est(engine, [rd], ref_len)[0] for rd in reads]                            # a read alone: its place in the batch plays no part
    assert all(np.array_equal(a["n_tot"], b["n_tot"]) and np.array_equal(a["n_match"], b["n_match"]) for a, b in zip(one_at_a_time, want))


def test_est_err_sum_k_above_2_to_24(engine):
    want = same_est(engine, [av.big_read()], av.LONG_REF_LEN)
    assert want[0]["sum_k"] == 18 * av.BIG_N - 1 and want[0]["n_tot"].tolist() == [42, 599, 66_667] and want[0]["n_match"].tolist() == [40, 200, 33_333]


def test_est_err_every_grid_strides(engine):
    """launch_est_err caps each launch at ceil(32 CU / 4) blocks: a batch with more than 32 CU reads, more than 32 CU hits of a wave and more than 128 CU hits of
    16 lanes makes each of the three kernels take a second step through its grid, with a read without minimizers and one without hits at the seams."""
    cu = engine.cu_count()
    assert cu >= 1
    reads, ref_len, c = av.stride_batch(cu)
    print(f"CUs {cu}: {c['reads']} reads (one pass: {32 * cu}), {c['long_hits']} hits of 64 anchors or more (one pass: {32 * cu}), {c['short_hits']} shorter hits (one pass: {128 * cu})")
    assert c["reads"] == len(reads) > 32 * cu and c["long_hits"] > 32 * cu and c["short_hits"] > 128 * cu
    for at in (0, 32 * cu, len(reads) - 2):
        assert len(reads[at]["mini_pos"]) == 0 and len(reads[at]["hits"]) == 1 and len(reads[at + 1]["hits"]) == 0
    want = same_est(engine, reads, ref_len)
    assert want[32 * cu]["n_tot"].tolist() == [-1] and any((w["n_tot"] < 0).any() for w in want[32 * cu + 2:]) and any((w["n_match"] >= 64).any() for w in want[32 * cu + 2:])
