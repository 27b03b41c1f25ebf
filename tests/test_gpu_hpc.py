"""Homopolymer-compressed minimizers on the device (csrc/seed_kernels.hip: the sketch pipeline's HPC form; mm2gb_sketch_gpu_flag, mm2gb_index_build_gpu_flag, and
every function that takes an index built with MM2GB_I_HPC) against the host functions of csrc/seeding.cpp, which tests/test_hpc_cpu.py
pins to the reference, and against the reference's recordings and PAF under -H -k19 / -x map-pb (tests/golden/hpc).  Every comparison
is exact."""
import hashlib
import json
import os

import numpy as np
import pytest

import golden_io
import hpc_cases as hc
import index_cases as ic
import sim_reads
from test_seeding_cpu import DATA, read_fasta

pytestmark = pytest.mark.gpu

mm = pytest.importorskip("mm2gb_amd")
GOLD = golden_io.GOLD
PB = dict(k=19, w=10, hpc=True)


@pytest.fixture(scope="module")
def engine():
    with mm.Engine() as e:
        yield e


@pytest.fixture(scope="module")
def sim150(tmp_path_factory):
    d = tmp_path_factory.mktemp("sim150")
    ref_fa, reads_fa = str(d / "ref.fa"), str(d / "reads.fa")
    sim_reads.simulate(ref_fa, reads_fa, seed=5, n_reads=150, len_lo=3_000, len_hi=20_000)             # as tests/tools/gen_golden_hpc.py
    return read_fasta(ref_fa), read_fasta(reads_fa)


@pytest.fixture(scope="module")
def sim160(tmp_path_factory):
    meta = json.load(open(os.path.join(GOLD, "sim160.json")))
    d = tmp_path_factory.mktemp("sim160")
    ref, reads = str(d / "ref.fa"), str(d / "reads.fa")
    sim_reads.simulate(ref, reads, seed=meta["seed"], n_reads=meta["n_reads"], len_lo=meta["len_lo"], len_hi=meta["len_hi"], tandem=meta["tandem"])
    assert hashlib.md5(open(ref, "rb").read()).hexdigest() == meta["ref_md5"] and hashlib.md5(open(reads, "rb").read()).hexdigest() == meta["reads_md5"]
    return read_fasta(ref), read_fasta(reads)


@pytest.mark.parametrize("k,w", hc.KW)
def test_sketch_equals_the_host_sketch(engine, k, w):
    """One batch laid end to end: run, N and sequence boundaries fall anywhere relative to the kernels' 256-position blocks."""
    rng = np.random.default_rng(3000 + 31 * k + w)
    seqs = [hc.hpc_seq(rng, n) for n in (0, 1, k - 1, k, 255, 256, 257, 3000)]
    seqs += [hc.hpc_seq(rng, 300, mixed_case=False) + b"AAA", b"AAAC" + hc.hpc_seq(rng, 300), b"a" * 40, b"A" * 40, b"", b"AT", b"TTG" + hc.hpc_seq(rng, 90)]   # neighbours share a base
    seqs += [b"G" * 70_000 + ic.rand_seq(rng, 2_000), b"N" * 300, b"N", hc.hpc_seq(rng, 2500, p_long=0.01), hc.hpc_seq(rng, 600).lower()]
    seqs += [b"AC" * 600, b"GATTACA" * 300, b"AATT" * 300, b"AACCGGTT" * 200, b"ACGT" * 400, b"AAAACCCGGT" * 150]                  # twins; k-mers equal to their reverse complement
    seqs += [hc.hpc_seq(rng, 500) + b"t" * 140 + b"T" * 140 + hc.hpc_seq(rng, 500)]
    seqs += [hc.hpc_seq(rng, int(n)) for n in list(rng.integers(0, 1024, 300)) + [255, 256, 257, 511, 512, 513] * 4]
    rid = np.arange(len(seqs), dtype=np.uint32) * 7 + 1
    got = engine.sketch(seqs, w=w, k=k, rid=rid, hpc=True)
    stats, twins = {}, 0
    for r, s in enumerate(seqs):
        want = mm.sketch(s, w, k, rid=int(rid[r]), hpc=True)
        assert np.array_equal(got[r], want), f"sequence {r} (length {len(s)}): {len(got[r])} pairs, host {len(want)}"
        if len(s) < 5000:
            twins += hc.has_twins(hc.steps_by_position(s, k, stats=stats), w)
    assert stats.get("long", 0) > 0                                       # k-mers left out for a span of 256 or more
    assert stats.get("symmetric", 0) > 0 or k % 2 == 1                    # (a k-mer of odd length is never its own reverse complement)
    assert twins > 0 or w == 1
    assert sum(len(x) for x in got) > 100
    assert all(np.array_equal(a, mm.sketch(s, w, k, hpc=True)) for a, s in zip(engine.sketch(seqs[:30], w=w, k=k, hpc=True), seqs[:30]))      # rid = None
    assert all(np.array_equal(a, mm.sketch(s, w, k)) for a, s in zip(engine.sketch(seqs[:30], w=w, k=k), seqs[:30]))                          # and the plain form after it


def small_genome():
    rng = np.random.default_rng(9)                                         # the genome of test_small_genome_against_itself
    return [c.tobytes() for c in sim_reads.make_genome(rng, n_chr=3, chr_len=20_000, n_rep_families=2, rep_len=300, copies=9, tandem=0)]


def genome_300k():
    rng = np.random.default_rng(31)
    return [c.tobytes() for c in sim_reads.make_genome(rng, n_chr=3, chr_len=100_000, n_rep_families=3, rep_len=500, copies=12, tandem=1)]


@pytest.mark.parametrize("name,chunk", [("3x20kb", 25_000), ("300kb", 120_000), ("300kb", 0)])
def test_device_built_index_equals_the_host_build(engine, monkeypatch, name, chunk):
    seqs = small_genome() if name == "3x20kb" else genome_300k()
    if chunk:
        monkeypatch.setenv("MM2GB_INDEX_CHUNK_BASES", str(chunk))           # three chunks
        assert sum(len(s) for s in seqs) > 2 * chunk
    with mm.SeedIndex(seqs, threads=8, **PB) as host, mm.SeedIndex(seqs, engine=engine, **PB) as dev, mm.SeedIndex(seqs, k=19, w=10, threads=8) as plain:
        want, got = host.view(), dev.view()
        assert dev.hpc and host.hpc and not plain.hpc
        assert want["n_occ"] > 0 and want["n_occ"] != plain.view()["n_occ"]
        ic.same_index(got, want, name)
        assert (got["k"], got["w"], got["built_on"], got["uploads"]) == (19, 10, engine.device, 0)
        res = dev.fetch_device(engine.device)
        for a in ic.ARRAYS:
            assert np.array_equal(res[a], want[a]), f"{name}: resident {a}"
        for frac, lo, hi in ((2e-4, 10, 1_000_000), (0.01, 1, 1_000_000), (0.5, 1, 5)):
            m = host.mid_occ(frac, lo, hi)
            assert dev.mid_occ(frac, lo, hi) == m and dev.mid_occ(frac, lo, hi, engine=engine) == m and host.mid_occ(frac, lo, hi, engine=engine) == m
        assert dev.view()["uploads"] == 0 and host.view()["uploads"] == 1


def same_matches(got, want, what):
    for r, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a["seeds"], b["seeds"]), f"{what} read {r}: seeds ({len(a['seeds'])} vs {len(b['seeds'])})"
        assert np.array_equal(a["hits"], b["hits"]), f"{what} read {r}: hits"
        assert a["rep_len"] == b["rep_len"] and np.array_equal(a["mini_pos"], b["mini_pos"]) and a["qlen"] == b["qlen"], f"{what} read {r}"


def check_case(engine, index, reads, case):
    mid_occ = index.mid_occ()
    got = engine.collect_matches(index, [s for _, s in reads], mid_occ)
    n = 0
    for k, (_, seq) in enumerate(reads):
        path = os.path.join(hc.HPC, "seeds", f"{case}_{k}.npz")
        if not os.path.exists(path):
            continue
        g, m = golden_io.load_seeds(path), got[k]
        assert g["qlen"] == len(seq) == m["qlen"]
        assert np.array_equal(m["seeds"], g["seeds"]) and np.array_equal(m["hits"], g["hits"]), f"{case} read {k}"
        assert m["rep_len"] == g["rep_len"] and np.array_equal(m["mini_pos"], g["mini_pos"]), f"{case} read {k}: rep_len / mini_pos"
        n += 1
    return n


@pytest.mark.parametrize("on_device", [False, True], ids=["host_index", "device_index"])
def test_matches_equal_the_recordings(engine, sim150, on_device):
    for case, tgt, qry in (("mt", "MT-human.fa", "MT-orang.fa"), ("inv", "t-inv.fa", "q-inv.fa")):
        with mm.SeedIndex([s for _, s in read_fasta(os.path.join(DATA, tgt))], engine=engine if on_device else None, **mm.preset("map-pb")) as ix:
            assert check_case(engine, ix, read_fasta(os.path.join(DATA, qry)), case) == hc.meta()[case]["records"]
    refs, reads = sim150
    with mm.SeedIndex([s for _, s in refs], engine=engine if on_device else None, **mm.preset("map-pb")) as ix:
        assert check_case(engine, ix, reads, "sim") == len(hc.meta()["sim"]["reads"])


def test_matches_equal_the_host_form_under_options_that_force_every_filter(engine, sim150):
    refs, reads = sim150
    reads = [s for _, s in reads]
    with mm.SeedIndex([s for _, s in refs], **PB) as ix:
        mo = ix.mid_occ()
        sets = {"a": dict(mid_occ=mo), "b": dict(mid_occ=2, max_max_occ=8, occ_dist=50), "b2": dict(mid_occ=3, max_max_occ=4095, occ_dist=20),
                "c": dict(mid_occ=mo, occ_dist=0), "d": dict(mid_occ=1, q_occ_frac=1e-4), "d0": dict(mid_occ=1, q_occ_frac=0.0),
                "e": dict(mid_occ=1 << 30, q_occ_frac=0.0)}
        host = {}
        for name, kw in sets.items():
            host[name] = [ix.matches(s, **kw) for s in reads]
            same_matches(engine.collect_matches(ix, reads, **kw), host[name], name)
        for name in ("b", "b2"):
            assert any((m["seeds"][:, 0] > sets[name]["mid_occ"]).any() for m in host[name]) and any(m["rep_len"] > 0 for m in host[name])
        assert any(len(a["seeds"]) < len(b["seeds"]) for a, b in zip(host["d"], host["d0"]))
        assert max(int((m["seeds"][:, 2] & 0xff).max()) for m in host["e"] if len(m["seeds"])) > 19 + 10      # spans well beyond k in the seeds


def map_pb(engine, refs, reads, index_on_device, seeding_on_device):
    with mm.SeedIndex([s for _, s in refs], engine=engine if index_on_device else None, **mm.preset("map-pb")) as ix:
        return mm.map_reads(engine, ix, [n for n, _ in refs], reads, opt=mm.map_opt(seeding_on_device=seeding_on_device), k=mm.preset("map-pb")["k"])


@pytest.mark.parametrize("seeding_on_device", [0, 1], ids=["seeding_on_host", "seeding_on_device"])
@pytest.mark.parametrize("index_on_device", [False, True], ids=["host_index", "device_index"])
@pytest.mark.parametrize("case,tgt,qry", [("mt", "MT-human.fa", "MT-orang.fa"), ("inv", "t-inv.fa", "q-inv.fa")])
def test_reference_pairs_paf_identical(engine, case, tgt, qry, index_on_device, seeding_on_device):
    paf, st = map_pb(engine, read_fasta(os.path.join(DATA, tgt)), read_fasta(os.path.join(DATA, qry)), index_on_device, seeding_on_device)
    want = open(os.path.join(hc.HPC, f"real_{case}_map-pb.paf")).read()
    assert len(want.splitlines()) == hc.meta()[case]["paf_lines"] and want != open(os.path.join(GOLD, f"real_{case}_inf.paf")).read()
    assert paf == want


@pytest.mark.parametrize("on_device", [False, True], ids=["all_host_seeding_host_index", "all_device"])
def test_simulated_long_reads_paf(engine, sim160, on_device):
    refs, reads = sim160
    paf, st = map_pb(engine, refs, reads, on_device, 1 if on_device else 0)
    want = open(os.path.join(hc.HPC, "sim160_map-pb.paf")).read()
    assert want != open(os.path.join(GOLD, "sim160_inf.paf")).read() and len(want.splitlines()) == hc.meta()["sim160"]["paf_lines"]
    assert st["n_reads"] == 160 and st["n_mapped"] == hc.meta()["sim160"]["reads_mapped"]
    if paf != want:
        g, w = paf.splitlines(), want.splitlines()
        bad = [k for k in range(min(len(g), len(w))) if g[k] != w[k]]
        raise AssertionError(f"{len(bad)} of {len(w)} PAF lines differ (got {len(g)}); first: {g[bad[0]] if bad else None} vs {w[bad[0]] if bad else None}")


def test_plain_and_compressed_indexes_share_an_engine(engine):
    """A plain index before and after a compressed one on the same engine and arenas: the PAF it gives today, seeding on either side."""
    pairs = [("mt", "MT-human.fa", "MT-orang.fa"), ("inv", "t-inv.fa", "q-inv.fa")]
    for case, tgt, qry in pairs:
        refs, reads = read_fasta(os.path.join(DATA, tgt)), read_fasta(os.path.join(DATA, qry))
        names = [n for n, _ in refs]
        plain_want = open(os.path.join(GOLD, f"real_{case}_inf.paf")).read()
        pb_want = open(os.path.join(hc.HPC, f"real_{case}_map-pb.paf")).read()
        with mm.SeedIndex([s for _, s in refs]) as plain, mm.SeedIndex([s for _, s in refs], engine=engine, **PB) as pb, mm.SeedIndex([s for _, s in refs], engine=engine) as plain_dev:
            for sod in (1, 0):
                assert mm.map_reads(engine, plain, names, reads, opt=mm.map_opt(seeding_on_device=sod))[0] == plain_want
                assert mm.map_reads(engine, pb, names, reads, opt=mm.map_opt(seeding_on_device=sod), k=19)[0] == pb_want
                assert mm.map_reads(engine, plain_dev, names, reads, opt=mm.map_opt(seeding_on_device=sod))[0] == plain_want
                assert mm.map_reads(engine, plain, names, reads, opt=mm.map_opt(seeding_on_device=sod))[0] == plain_want
            a = engine.sketch([s for _, s in reads], hpc=True, k=19)
            b = engine.sketch([s for _, s in reads])
            assert all(np.array_equal(x, mm.sketch(s, 10, 19, hpc=True)) for x, (_, s) in zip(a, reads))
            assert all(np.array_equal(x, mm.sketch(s)) for x, (_, s) in zip(b, reads))
