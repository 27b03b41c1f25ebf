"""Single-affine gap scoring above the DP, on the device: the alignment of hits at q == q2 && e == e2 (mm2gb_align_regs_extz_gpu) against its
host form and the recorded fixtures, and the mapper with such an option set against the PAF the reference's CPU program printed for
`-O4 -E2` (tests/golden/paf_single, recorded by tests/tools/gen_golden_paf_single.py), byte for byte."""
import hashlib
import json
import os

import numpy as np
import pytest

import align_cases as ac
import golden_io
import ksw_single_cases as ks
import sim_reads
from test_seeding_cpu import DATA, read_fasta

pytestmark = pytest.mark.gpu

import mm2gb_amd as mm  # noqa: E402
VARIANTS = {"c": dict(), "cs": dict(cs="short"), "long_md": dict(cs="long", md=True)}
PAIRS = {"mt": ("MT-human.fa", "MT-orang.fa"), "inv": ("t-inv.fa", "q-inv.fa")}
SINGLE = dict(q=4, e=2, q2=4, e2=2)


@pytest.fixture(scope="module")
def engine():
    with mm.Engine() as e:
        yield e


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """case -> (references, reads): the two pairs of sequence files and the 24 simulated reads of tests/golden/paf_aln/sim.json"""
    out = {c: (read_fasta(os.path.join(DATA, t)), read_fasta(os.path.join(DATA, q))) for c, (t, q) in PAIRS.items()}
    meta = json.load(open(os.path.join(golden_io.GOLD, "paf_aln", "sim.json")))
    d = tmp_path_factory.mktemp("sim")
    ref, reads = str(d / "ref.fa"), str(d / "reads.fa")
    sim_reads.simulate(ref, reads, **meta["sim"])
    assert hashlib.md5(open(ref, "rb").read()).hexdigest() == meta["ref_md5"], "simulator drifted: regenerate the golden"
    assert hashlib.md5(open(reads, "rb").read()).hexdigest() == meta["reads_md5"]
    out["sim"] = (read_fasta(ref), read_fasta(reads))
    return out


def golden(case, variant):
    return np.load(os.path.join(ks.PAF_GOLD, f"pafs_{case}.npz"))[variant].tobytes().decode()


def same_paf(got, want, what):
    if got != want:
        g, w = got.splitlines(), want.splitlines()
        bad = [k for k in range(min(len(g), len(w))) if g[k] != w[k]]
        raise AssertionError(f"{what}: {len(bad)} of {len(w)} PAF lines differ (got {len(g)}); first: {g[bad[0]][:200] if bad else None!r} vs {w[bad[0]][:200] if bad else None!r}")


# ---------------------------------------------------------------- the alignment call
@pytest.mark.parametrize("name", list(ks.ALIGN_BATCHES))
def test_alignment_equals_host_and_fixtures(engine, name):
    b, want = ks.load_align(name)
    got, info = ks.run_align_gpu(engine, b)
    ac.assert_same(got, want, name + ": device against the fixture")
    ac.assert_same(got, ks.run_align_host(b, threads=8)[0], name + ": device against host")
    assert info["counts"]["jobs"] > 0


def test_alignment_of_a_30_kb_read(engine):
    """One 30 kb read against a 40 kb reference with 6 kb of the reference missing from the read: the fill across it is bw_long wide, beyond the
    one-wave and four-wave classes of the DP.  The chain is made here (one anchor every 500 bases, on two diagonals)."""
    rng = np.random.default_rng(8)
    ref = sim_reads.BASES[rng.integers(0, 4, 40_000)]
    read = np.concatenate([ref[2000:17_000], ref[23_000:38_000]])
    pos = [p for p in range(100, 30_000, 500) if not 14_900 < p < 15_100]
    a = np.array([[(p + 2000 if p < 15_000 else p + 8000), 15 << 32 | p] for p in pos], np.uint64)
    regs = np.zeros(1, mm.REG_DTYPE)
    regs[0] = (0, len(a), 0, 15 * len(a), pos[0] - 14, pos[-1] + 1, int(a[0, 0]) - 14, int(a[-1, 0]) + 1, 0, 0, 0, 15 * len(a), 30_000, 0, 15 * len(a), 0, 7, -1.0)
    args = (mm.align_opt("map-ont", q2=4, e2=2), 15, False, [ref.tobytes()], [bytes(read)], [regs], [a])
    want, _ = mm.align_regs_extz_host(*args, threads=1)
    got, _ = engine.align_regs_extz(*args)
    ac.assert_same(got, want, "30 kb read")
    assert sum(int(x["n_cigar"]) for x in want[0][1]) > 0
    with pytest.raises(mm.Mm2gbError, match="mm2gb_align_regs_gpu: q == q2 && e == e2 selects ksw_extz2_sse, which is not supported"):
        engine.align_regs(*args)
    args = (mm.align_opt("map-ont"),) + args[1:]
    with pytest.raises(mm.Mm2gbError, match=r"mm2gb_align_regs_extz_gpu: q != q2 \|\| e != e2"):
        engine.align_regs_extz(*args)


# ---------------------------------------------------------------- the mapper
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("case", ["mt", "inv", "sim"])
def test_paf_identical_to_the_reference(engine, inputs, case, variant):
    """map_align(refs, q=4, e=2, q2=4, e2=2) is all it takes: step 6a goes to the _extz alignment pair.  Before the single-affine DP was here
    the same call raised Mm2gbError (q == q2 && e == e2 ... not supported)."""
    refs, reads = inputs[case]
    want = golden(case, variant)
    with mm.SeedIndex([s for _, s in refs]) as ix:
        for align_on_device in (1, -1):
            for text_on_device in (1, -1):
                al = mm.map_align([s for _, s in refs], align_on_device=align_on_device, text_on_device=text_on_device, **SINGLE, **VARIANTS[variant])
                paf, st = mm.map_reads(engine, ix, [n for n, _ in refs], reads, align=al)
                same_paf(paf, want, f"{case} {variant}, alignment {align_on_device}, text {text_on_device}")
                assert st["n_reads"] == len(reads)
    if case == "sim":
        dual = np.load(os.path.join(golden_io.GOLD, "paf_aln", "pafs_sim_map-ont.npz"))[variant].tobytes().decode()
        assert want != dual, "the fixture would pass with the dual-affine DP"


def test_a_stream_of_chunks(engine, inputs):
    refs, reads = inputs["sim"]
    want = golden("sim", "long_md")
    with mm.SeedIndex([s for _, s in refs]) as ix, mm.Engine() as e2:
        al = mm.map_align([s for _, s in refs], cs="long", md=True, **SINGLE)
        paf, st = mm.map_reads_stream([engine, e2], ix, [n for n, _ in refs], reads, opt=mm.map_opt(host_threads=8), chunk_bases=12_000, align=al)
        same_paf(paf, want, "stream over two engines")
        assert st["n_reads"] == len(reads) and st["s_align"] > 0
