"""The mapper's resident path (seeding_on_device = 2) where records are dropped: map-ont / map-pb --no-long-join and map-ont -r 500,500 on the chimeric set and on
sim160, byte for byte against the runs recorded from the reference program (tests/golden/resident) in the four forms of tests/test_gpu_ava.py; the per-batch
fall-backs of the resident path, its early return for a batch without a chain, several engines, and staged and resident calls alternating on one engine's arenas.
Where the reference did not record the expected text it is the staged form's (seeding_on_device = 1) for the same call."""
import re

import pytest

import mm2gb_amd as mm
import resident_cases as rc
from asm_cases import same_paf
from test_gpu_ava import FORMS

pytestmark = pytest.mark.gpu

RESIDENT, STAGED = FORMS["resident"], FORMS["seeding_on_device"]
RUN = "chim.map-ont"
LINE = re.compile(r"\[mm2gb\] map path: (resident|staged)( \([^)]*\))?; (\d+) anchors, (\d+) chains; copied to the device (\d+) B, back (\d+) B")
NO_ROOM, NOT_ALLOWED = "exceed one chaining micro-batch", "the options do not allow it"


@pytest.fixture(scope="module")
def engine():
    with mm.Engine(device=0) as e:
        yield e


@pytest.fixture(scope="module")
def engines3(engine):
    with mm.Engine(device=0) as e2, mm.Engine(device=0) as e3:
        yield [engine, e2, e3]


def path_lines(capfd):
    """The MM2GB_DEBUG_PHASES lines of the calls since the last look: one per batch."""
    return [dict(path=m[1], why=m[2] or "", anchors=int(m[3]), chains=int(m[4]), up=int(m[5]), back=int(m[6])) for m in LINE.finditer(capfd.readouterr().err)]


def traced(capfd, monkeypatch, call):
    """call() with the path line on: (its result, the lines)."""
    monkeypatch.setenv("MM2GB_DEBUG_PHASES", "1")
    capfd.readouterr()
    res = call()
    lines = path_lines(capfd)
    monkeypatch.delenv("MM2GB_DEBUG_PHASES")
    return res, lines


def names_of(reads):
    return [n for n, _ in reads]


# ---------------------------------------------------------------- the recorded runs
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("skip", list(rc.SKIPS))
@pytest.mark.parametrize("run", rc.RUNS)
def test_paf_equals_the_reference(engine, capfd, monkeypatch, run, skip, form):
    if form != "resident":
        got, st = rc.map_run(engine, run, skip, **FORMS[form])
        same_paf(got, rc.golden_paf(run, skip), f"{run} {skip} {form}")
        assert st["n_rechained"] == 0
        return
    (got, st), res = traced(capfd, monkeypatch, lambda: rc.map_run(engine, run, skip, **RESIDENT))
    same_paf(got, rc.golden_paf(run, skip), f"{run} {skip} resident")
    _, stg = traced(capfd, monkeypatch, lambda: rc.map_run(engine, run, skip, **STAGED))
    assert [ln["path"] for ln in res] == ["resident"] and [ln["path"] for ln in stg] == ["staged"] and res[0]["why"] == stg[0]["why"] == ""
    assert st["n_rechained"] == 0
    assert st["n_chains"] > len(got.splitlines()) > 0                               # mm_select_sub dropped something
    assert (res[0]["anchors"], res[0]["chains"]) == (stg[0]["anchors"], stg[0]["chains"]) == (st["n_anchors"], st["n_chains"])
    assert res[0]["back"] < stg[0]["back"] and res[0]["back"] < 16 * st["n_anchors"]  # no anchor array came down


# ---------------------------------------------------------------- the per-batch fall-backs and the early return
def test_falls_back_where_the_batch_exceeds_one_micro_batch(engine, capfd, monkeypatch):
    want, st = rc.map_run(engine, RUN, **STAGED)
    monkeypatch.setenv("MM2GB_CHAIN_SLICE_ANCHORS", str(st["n_anchors"] // 3))                       # 1.5 x the value: half the batch's hits
    (got, _), lines = traced(capfd, monkeypatch, lambda: rc.map_run(engine, RUN, **RESIDENT))
    assert [ln["path"] for ln in lines] == ["staged"] and NO_ROOM in lines[0]["why"]
    assert got == want == rc.golden_paf(RUN, "inf")


def test_resident_at_the_size_limit_and_staged_one_anchor_beyond(engine, capfd, monkeypatch):
    """resident_max_anchors is v + v / 2 for MM2GB_CHAIN_SLICE_ANCHORS = v: the smallest v that holds the batch's hits keeps it resident, one less does not."""
    want, st = rc.map_run(engine, RUN, **STAGED)
    n = st["n_anchors"]                                                                              # (without the strand and rank bits every hit is an anchor)
    v = next(v for v in range(n * 2 // 3 - 2, n) if v + v // 2 >= n)
    assert v + v // 2 >= n > (v - 1) + (v - 1) // 2
    for value, path in ((v, "resident"), (v - 1, "staged")):
        monkeypatch.setenv("MM2GB_CHAIN_SLICE_ANCHORS", str(value))
        (got, _), lines = traced(capfd, monkeypatch, lambda: rc.map_run(engine, RUN, **RESIDENT))
        assert [ln["path"] for ln in lines] == [path] and (NO_ROOM in lines[0]["why"]) == (path == "staged"), (value, n, lines)
        assert got == want


def test_a_batch_without_a_hit(engine, capfd, monkeypatch):
    reads = rc.no_hit_reads(RUN, 3) + rc.ODD + [("tiny_" + n, s) for n, s in rc.no_hit_reads(RUN, 2, length=400, seed=rc.NO_HIT_SEED + 1)]
    (got, st), lines = traced(capfd, monkeypatch, lambda: rc.map_run(engine, RUN, reads=reads, **RESIDENT))
    assert got == "" and (st["n_reads"], st["n_mapped"], st["n_anchors"], st["n_chains"]) == (len(reads), 0, 0, 0)
    assert [ln["path"] for ln in lines] == ["staged"] and "or it has none" in lines[0]["why"]
    assert rc.map_run(engine, RUN, reads=reads, **STAGED)[0] == ""


def test_a_batch_with_anchors_and_no_chain(engine, capfd, monkeypatch):
    """hit_records_resident returns before its kernels where the batch has no chain: no line, and the next batch on the engine is served as ever."""
    reads = rc.piece_reads()
    (got, st), lines = traced(capfd, monkeypatch, lambda: rc.map_run(engine, RUN, reads=reads, **RESIDENT))
    assert [ln["path"] for ln in lines] == ["resident"]
    assert st["n_anchors"] > 0 and st["n_chains"] == 0 and got == "" and st["n_mapped"] == 0
    stg, st1 = rc.map_run(engine, RUN, reads=reads, **STAGED)
    assert stg == "" and (st1["n_anchors"], st1["n_chains"]) == (st["n_anchors"], 0)
    same_paf(rc.map_run(engine, RUN, **RESIDENT)[0], rc.golden_paf(RUN, "inf"), "the whole set after a batch without a chain")


def test_a_mixed_batch(engine, capfd, monkeypatch):
    """Reads without a minimizer, without a hit and without a chain first, last and between mapping reads: lines for exactly the mapping reads."""
    chim = rc.reads_of("chim")
    nowhere = rc.ODD + rc.no_hit_reads(RUN, 2) + rc.piece_reads(n=3)
    reads = nowhere[:2] + chim[:3] + nowhere[2:5] + chim[3:4] + nowhere[5:7] + chim[4:9] + nowhere[7:]
    assert len(reads) == len(nowhere) + 9 and reads[0][0] == "empty" and reads[-1][0].startswith("piece")
    (got, st), lines = traced(capfd, monkeypatch, lambda: rc.map_run(engine, RUN, reads=reads, **RESIDENT))
    want, _ = rc.map_run(engine, RUN, reads=reads, **STAGED)
    assert [ln["path"] for ln in lines] == ["resident"]
    assert got == want == rc.lines_of(rc.golden_paf(RUN, "inf"), names_of(chim[:9]))
    assert {ln.split("\t")[0] for ln in got.splitlines()} == set(names_of(chim[:9])) and st["n_mapped"] == 9 and st["n_reads"] == len(reads)


def test_one_read_one_chain(engine, capfd, monkeypatch):
    """The smallest batch that maps: 400 exact bases of the genome's unique part."""
    genome = rc.refs_of("chim")[0][1]
    reads = [("one", genome[85_000:85_400])]
    (got, st), lines = traced(capfd, monkeypatch, lambda: rc.map_run(engine, RUN, reads=reads, **RESIDENT))
    want, _ = rc.map_run(engine, RUN, reads=reads, **STAGED)
    assert [ln["path"] for ln in lines] == ["resident"] and st["n_chains"] == 1 and st["n_anchors"] >= 3
    assert got == want and len(got.splitlines()) == 1
    f = got.split("\t")
    assert f[:9] == ["one", "400", f[2], f[3], "+", "chim_ref", "120000", str(85_000 + int(f[2])), str(85_000 + int(f[3]))] and "tp:A:P" in f


# ---------------------------------------------------------------- one engine's arenas, several engines
def test_staged_and_resident_calls_alternate_on_one_engine(engine):
    """The two paths share the engine's post_out, reg_out, sd_* and ee_* arenas: a large resident batch, a small staged one, the small one resident, the large one
    again, and the small one after the host scratch was given back -- the same text for the same input every time."""
    few = rc.reads_of("chim")[20:24]
    all_want, few_want = rc.golden_paf(RUN, "inf"), rc.lines_of(rc.golden_paf(RUN, "inf"), names_of(few))
    assert len(few_want.splitlines()) >= 4
    same_paf(rc.map_run(engine, RUN, **RESIDENT)[0], all_want, "resident, all")
    same_paf(rc.map_run(engine, RUN, reads=few, **STAGED)[0], few_want, "staged, 4 reads")
    same_paf(rc.map_run(engine, RUN, reads=few, **RESIDENT)[0], few_want, "resident, 4 reads")
    same_paf(rc.map_run(engine, RUN, **RESIDENT)[0], all_want, "resident, all again")
    engine.release_host_scratch()
    same_paf(rc.map_run(engine, RUN, reads=few, **RESIDENT)[0], few_want, "resident, 4 reads after release_host_scratch")


@pytest.mark.parametrize("run", ["chim.map-ont", "chim.map-pb"])
def test_reads_sharded_over_three_engines(engines3, capfd, monkeypatch, run):
    reads, refs = rc.reads_of("chim"), rc.refs_of("chim")
    opt, k = rc.options(run, host_threads=6, **RESIDENT)
    (got, st), lines = traced(capfd, monkeypatch, lambda: mm.map_reads_multi(engines3, rc.index_for(run), names_of(refs), reads, opt=opt, k=k))
    same_paf(got, rc.golden_paf(run, "inf"), f"{run}: three engines")
    assert [ln["path"] for ln in lines] == ["resident"] * 3 and sum(ln["chains"] for ln in lines) == st["n_chains"] and st["n_reads"] == len(reads)


def test_a_stream_of_chunks_where_one_has_no_hit(engines3, capfd, monkeypatch):
    """Three engines take chunks of about 60 kb; the random reads in the middle fill at least one chunk of their own, which falls back (no hit: nothing to keep on
    the device) while the others stay resident."""
    chim, chunk = rc.reads_of("chim"), 60_000
    nowhere = rc.no_hit_reads(RUN, 45)                                               # 135 kb: whatever the cut before them, a whole chunk of them follows
    reads = chim[:30] + nowhere + chim[30:]
    chunks = rc.stream_chunks([len(s) for _, s in reads], chunk)
    lonely = [c for c in chunks if all(reads[r][0].startswith("random") for r in range(*c))]
    assert 7 <= len(chunks) <= 12 and len(lonely) >= 1
    opt, k = rc.options(RUN, host_threads=6, **RESIDENT)
    call = lambda: mm.map_reads_stream(engines3, rc.index_for(RUN), names_of(rc.refs_of("chim")), reads, opt=opt, k=k, chunk_bases=chunk)
    (got, st), lines = traced(capfd, monkeypatch, call)
    same_paf(got, rc.golden_paf(RUN, "inf"), "stream, three engines")
    assert st["n_reads"] == len(reads) and len(lines) == len(chunks)
    staged = [ln for ln in lines if ln["path"] == "staged"]
    assert len(staged) == len(lonely) and all("or it has none" in ln["why"] and ln["anchors"] == 0 for ln in staged)
    assert all(ln["why"] == "" and ln["anchors"] > 0 for ln in lines if ln["path"] == "resident")


def test_a_finite_skip_limit_runs_the_walk_on_the_resident_path(capfd, monkeypatch):
    """max_chain_skip = 25 with records dropped: the chaining kernel is the skip-limited walk (k_skip_fill), whose counters change with the call."""
    monkeypatch.setenv("MM2GB_SKIP_STATS", "1")
    few = rc.reads_of("chim")[:4]
    with mm.Engine(device=0) as e:
        got, _ = rc.map_run(e, RUN, "inf", **RESIDENT)                               # exhaustive: the walk has not run, there are no counters
        same_paf(got, rc.golden_paf(RUN, "inf"), "inf")
        with pytest.raises(mm.Mm2gbError, match="no counters"):
            e.skip_stats()
        (got, st), lines = traced(capfd, monkeypatch, lambda: rc.map_run(e, RUN, "s25", reads=few, **RESIDENT))
        assert [ln["path"] for ln in lines] == ["resident"] and got == rc.lines_of(rc.golden_paf(RUN, "s25"), names_of(few))
        first = e.skip_stats()
        assert e.last_score_form() == 1 and first["targets"] > 0 and first["rounds"] > 0
        (got, st), lines = traced(capfd, monkeypatch, lambda: rc.map_run(e, RUN, "s25", **RESIDENT))
        same_paf(got, rc.golden_paf(RUN, "s25"), "s25")
        second = e.skip_stats()
        assert [ln["path"] for ln in lines] == ["resident"] and st["n_chains"] > len(got.splitlines())
        assert second != first and second["targets"] > first["targets"]
