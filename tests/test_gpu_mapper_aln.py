"""The mapper with base-level alignment (mm2gb_map_reads_aln, mm2gb_map_reads_stream_aln; minimap2 -c, --cs, --MD) against the PAF the
reference's CPU program printed for the same sequences (tests/golden/paf_aln/pafs_*.npz, recorded by tests/tools/gen_golden_paf_aln.py): byte for
byte, with the alignment call and the text call each on the device and on host threads."""
import hashlib
import json
import os

import numpy as np
import pytest

import golden_io
import sim_reads
from test_seeding_cpu import DATA, read_fasta

pytestmark = pytest.mark.gpu

import mm2gb_amd as mm  # noqa: E402
GOLD = os.path.join(golden_io.GOLD, "paf_aln")
VARIANTS = {"c": dict(), "cs": dict(cs="short"), "long_md": dict(cs="long", md=True)}
CASES = ["mt", "inv", "q2", "sim_map-ont", "sim_map-pb"]
PAIRS = {"mt": ("MT-human.fa", "MT-orang.fa"), "inv": ("t-inv.fa", "q-inv.fa"), "q2": ("t2.fa", "q2.fa")}


@pytest.fixture(scope="module")
def engine():
    with mm.Engine() as e:
        yield e


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """case -> (references, reads, preset)"""
    out = {c: (read_fasta(os.path.join(DATA, t)), read_fasta(os.path.join(DATA, q)), "map-ont") for c, (t, q) in PAIRS.items()}
    meta = json.load(open(os.path.join(GOLD, "sim.json")))
    d = tmp_path_factory.mktemp("sim")
    ref, reads = str(d / "ref.fa"), str(d / "reads.fa")
    sim_reads.simulate(ref, reads, **meta["sim"])
    assert hashlib.md5(open(ref, "rb").read()).hexdigest() == meta["ref_md5"], "simulator drifted: regenerate the golden"
    assert hashlib.md5(open(reads, "rb").read()).hexdigest() == meta["reads_md5"]
    for preset in ("map-ont", "map-pb"):
        out["sim_" + preset] = (read_fasta(ref), read_fasta(reads), preset)
    return out


def golden(case, variant):
    return np.load(os.path.join(GOLD, f"pafs_{case}.npz"))[variant].tobytes().decode()


def index_of(refs, preset):
    return mm.SeedIndex([s for _, s in refs], **(mm.preset("map-pb") if preset == "map-pb" else {}))


def same_paf(got, want, what):
    if got != want:
        g, w = got.splitlines(), want.splitlines()
        bad = [k for k in range(min(len(g), len(w))) if g[k] != w[k]]
        first = bad[0] if bad else min(len(g), len(w))
        at = next((i for i, (x, y) in enumerate(zip(g[first], w[first])) if x != y), None) if bad else None
        raise AssertionError(f"{what}: {len(bad)} of {len(w)} PAF lines differ (got {len(g)}); first: line {first}, byte {at}: "
                             f"{g[first][max((at or 0) - 60, 0):(at or 0) + 60] if bad else None!r} vs {w[first][max((at or 0) - 60, 0):(at or 0) + 60] if bad else None!r}")


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("case", CASES)
def test_paf_identical_to_the_reference(engine, inputs, case, variant):
    refs, reads, preset = inputs[case]
    want = golden(case, variant)
    k = 19 if preset == "map-pb" else 15
    with index_of(refs, preset) as ix:
        for align_on_device in (1, -1):
            for text_on_device in (1, -1):
                al = mm.map_align([s for _, s in refs], preset=preset, align_on_device=align_on_device, text_on_device=text_on_device, **VARIANTS[variant])
                paf, st = mm.map_reads(engine, ix, [n for n, _ in refs], reads, k=k, align=al)
                same_paf(paf, want, f"{case} {variant}, alignment {align_on_device}, text {text_on_device}")
                assert st["n_rmq_tied"] == 0 and st["n_reads"] == len(reads)
                assert all(key in st for key in ("s_align", "s_post_align", "s_text"))
    if case == "inv":
        assert "tp:A:I" in want or "tp:A:i" in want
    if case.startswith("sim"):
        assert "tp:A:S" in want and "\tzd:i:" in want and "\t-\t" in want


def test_default_sides_and_no_text(engine, inputs):
    """align_on_device / text_on_device left at 0; what = 0 gives the -c line without cg:Z."""
    refs, reads, preset = inputs["sim_map-ont"]
    want = golden("sim_map-ont", "cs")
    with index_of(refs, preset) as ix:
        paf, _ = mm.map_reads(engine, ix, [n for n, _ in refs], reads, align=mm.map_align([s for _, s in refs], cs="short"))
        same_paf(paf, want, "defaults")
        bare, _ = mm.map_reads(engine, ix, [n for n, _ in refs], reads, align=mm.map_align([s for _, s in refs], cigar=False))
        same_paf(bare, "".join(ln.split("\tcg:Z:")[0] + "\n" for ln in want.splitlines()), "what = 0")


def test_a_stream_of_chunks_with_alignment(engine, inputs):
    refs, reads, preset = inputs["sim_map-ont"]
    want = golden("sim_map-ont", "long_md")
    with index_of(refs, preset) as ix, mm.Engine() as e2:
        for text_on_device in (1, -1):
            al = mm.map_align([s for _, s in refs], cs="long", md=True, text_on_device=text_on_device)
            paf, st = mm.map_reads_stream([engine, e2], ix, [n for n, _ in refs], reads, opt=mm.map_opt(host_threads=8), chunk_bases=12_000, align=al)
            same_paf(paf, want, f"stream, text {text_on_device}")
            assert st["n_reads"] == len(reads) and st["n_rmq_tied"] == 0 and st["s_align"] > 0
        assert mm.map_reads_stream([engine, e2], ix, [n for n, _ in refs], [], align=al)[0] == ""


def test_without_align_nothing_moves(engine, tmp_path):
    """align=None is the path of before: the golden of tests/test_gpu_mapper.py."""
    meta = json.load(open(os.path.join(golden_io.GOLD, "sim160.json")))
    ref, reads = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fa")
    sim_reads.simulate(ref, reads, seed=meta["seed"], n_reads=meta["n_reads"], len_lo=meta["len_lo"], len_hi=meta["len_hi"], tandem=meta["tandem"])
    refs, rd = read_fasta(ref), read_fasta(reads)
    with mm.SeedIndex([s for _, s in refs]) as ix:
        paf, st = mm.map_reads(engine, ix, [n for n, _ in refs], rd, align=None)
    same_paf(paf, open(os.path.join(golden_io.GOLD, "sim160_inf.paf")).read(), "align=None")
    assert "s_align" not in st


def test_refusals(engine, inputs):
    refs, reads, preset = inputs["mt"]
    with index_of(refs, preset) as ix:
        with pytest.raises(mm.Mm2gbError, match="MM_F_SPLICE"):                                   # the alignment call's own text
            mm.map_reads(engine, ix, [n for n, _ in refs], reads, align=mm.map_align([s for _, s in refs], flag=mm.F_SPLICE))
        with pytest.raises(mm.Mm2gbError, match="another number of reference sequences"):
            mm.map_reads(engine, ix, [n for n, _ in refs], reads, align=mm.map_align([]))
        al = mm.map_align([s for _, s in refs]); al.what = 0x40
        with pytest.raises(mm.Mm2gbError, match="MM2GB_TEXT"):
            mm.map_reads(engine, ix, [n for n, _ in refs], reads, align=al)
