"""The minimizer index built on the device (csrc/index_kernels.hip: mm2gb_index_build_gpu, mm2gb_index_mid_occ_gpu) against the host build of
csrc/seeding.cpp, which tests/test_index_api_cpu.py pins to a reconstruction from the sketch and tests/test_seeding_cpu.py to the reference's
recordings.  Every comparison is exact."""
import functools
import os

import numpy as np
import pytest

import index_cases as ic
import sim_reads
from test_gpu_seeding import check_case

pytestmark = pytest.mark.gpu

mm = pytest.importorskip("mm2gb_amd")
NAMES = ["golden", "genome", "odd", "none", "empty_only"]


@pytest.fixture(scope="module")
def engine():
    with mm.Engine() as e:
        yield e


@functools.lru_cache(maxsize=None)
def big_seq():
    return ic.rand_seq(np.random.default_rng(5), 3_000_000)


@functools.lru_cache(maxsize=None)
def host_view(name, k, w):
    seqs = [big_seq()] if name == "big" else ic.inputs()[name]
    with mm.SeedIndex(seqs, k=k, w=w, threads=8) as ix:
        return ix.view()


def same_as_host(engine, seqs, want, what):
    """The device-built index of seqs: its host arrays, and what is resident on the device, against the host build's view."""
    with mm.SeedIndex(seqs, k=want["k"], w=want["w"], engine=engine) as ix:
        got = ix.view()
        ic.same_index(got, want, what)
        assert (got["k"], got["w"], got["built_on"], got["uploads"]) == (want["k"], want["w"], engine.device, 0), what
        dev = ix.fetch_device(engine.device)
        for a in ic.ARRAYS:
            assert np.array_equal(dev[a], want[a]) and np.array_equal(dev[a], got[a]), f"{what}: resident {a}"
        assert ix.size() == (want["n_keys"], want["n_occ"]) and ix.view()["uploads"] == 0
        split = ix.build_split()
        assert all(v >= 0 for v in split.values()) and (want["n_occ"] == 0 or split["sort"] > 0)


@pytest.mark.parametrize("k,w", ic.KW)
@pytest.mark.parametrize("name", NAMES)
def test_arrays_equal_the_host_build(engine, name, k, w):
    want = host_view(name, k, w)
    assert want["built_on"] == -1 and (want["n_occ"] > 0) == (name in ("golden", "genome", "odd"))
    same_as_host(engine, ic.inputs()[name], want, f"{name} k={k} w={w}")


def test_arrays_equal_the_host_build_one_long_sequence(engine):
    want = host_view("big", 15, 10)
    assert want["n_occ"] > 500_000 and want["n_keys"] > 1 << 19         # more than one block of every kernel, a bucket table of 2^20 entries
    same_as_host(engine, [big_seq()], want, "3 Mbp")


@pytest.mark.parametrize("k,w", ic.KW[:2])
@pytest.mark.parametrize("chunk", [1, 1_000, 20_000])
@pytest.mark.parametrize("name", ["golden", "genome", "odd", "empty_only"])
def test_chunked_builds_are_identical(engine, monkeypatch, name, chunk, k, w):
    """MM2GB_INDEX_CHUNK_BASES is read at call time: every sequence a chunk of its own (1), sequences longer than the chunk beside ones that
    share a chunk (1 000: `odd` has 1 500- and 2 000-base sequences between empty ones and short ones), several sequences per chunk (20 000)."""
    seqs = ic.inputs()[name]
    if chunk == 1_000 and name == "odd":
        lens = [len(s) for s in seqs]
        assert max(lens) > chunk and 0 in lens and any(0 < n < chunk for n in lens)
    monkeypatch.setenv("MM2GB_INDEX_CHUNK_BASES", str(chunk))
    same_as_host(engine, seqs, host_view(name, k, w), f"{name} chunk={chunk} k={k} w={w}")


def test_chunked_build_with_a_sequence_longer_than_the_chunk(engine, monkeypatch):
    seqs = ic.inputs()["odd"] + [big_seq(), b""] + ic.inputs()["golden"]
    with mm.SeedIndex(seqs, threads=8) as ix:
        want = ix.view()
    monkeypatch.setenv("MM2GB_INDEX_CHUNK_BASES", "1000000")
    same_as_host(engine, seqs, want, "3 Mbp among short sequences, chunks of 1 Mbp")
    monkeypatch.setenv("MM2GB_INDEX_CHUNK_BASES", "not a number")       # falls back to the default
    same_as_host(engine, seqs, want, "default chunk")


@functools.lru_cache(maxsize=None)
def repeat_genome():
    rng = np.random.default_rng(21)
    return [c.tobytes() for c in sim_reads.make_genome(rng, n_chr=2, chr_len=150_000, n_rep_families=4, rep_len=2000, copies=16, tandem=2)]


FRACS = (0.0, 2e-4, 0.01, 0.5, 1.0)
CLAMPS = ((10, 1_000_000), (1, 1_000_000), (50, 60), (1, 5), (10, 10), (3, 2))


@pytest.mark.parametrize("on_device", [True, False])
def test_mid_occ_equals_the_host_value(engine, on_device):
    with mm.SeedIndex(repeat_genome(), engine=engine if on_device else None) as ix:
        host = {(f, c): ix.mid_occ(f, *c) for f in FRACS for c in CLAMPS}
        # the quantile itself decides, not the clamps: above the minimum, below the maximum, different for different fractions
        free = [host[(f, (1, 1_000_000))] for f in (2e-4, 0.01, 0.5)]
        assert all(1 < v < 1_000_000 for v in free) and len(set(free)) == 3 and host[(2e-4, (10, 1_000_000))] > 10
        for (f, c), want in host.items():
            assert ix.mid_occ(f, *c, engine=engine) == want, f"frac {f} clamps {c}"
        assert ix.view()["uploads"] == (0 if on_device else 1)           # a host-built index went up once, through index_on_device
    with mm.SeedIndex([], engine=engine if on_device else None) as ix:   # no keys: no quantile
        assert all(ix.mid_occ(f, *c, engine=engine) == ix.mid_occ(f, *c) for f in FRACS for c in CLAMPS)


def test_residency(engine):
    seqs = ic.inputs()["genome"]
    reads = [seqs[0][1_000:5_000], seqs[2][20_000:23_000]]
    with mm.SeedIndex(seqs, engine=engine) as dev, mm.SeedIndex(seqs) as host:
        got = engine.collect_matches(dev, reads, mid_occ=dev.mid_occ())
        want = engine.collect_matches(host, reads, mid_occ=host.mid_occ())
        engine.collect_matches(host, reads, mid_occ=host.mid_occ())
        assert dev.view()["uploads"] == 0 and host.view()["uploads"] == 1
        assert (dev.view()["built_on"], host.view()["built_on"]) == (engine.device, -1)
        for a, b, s in zip(got, want, reads):
            ref = host.matches(s, host.mid_occ())
            for key in ("seeds", "hits", "mini_pos"):
                assert np.array_equal(a[key], b[key]) and np.array_equal(a[key], ref[key]) and len(a["seeds"]) > 0
            assert a["rep_len"] == b["rep_len"] == ref["rep_len"]


@pytest.mark.parametrize("case,tgt,qry", [("mt", "MT-human.fa", "MT-orang.fa"), ("inv", "t-inv.fa", "q-inv.fa"),
                                          ("mt_x_self", "MT-human.fa", "MT-human.fa"), ("mt_x_smaller", "MT-orang.fa", "MT-human.fa")])
def test_the_references_recordings_with_a_device_built_index(engine, case, tgt, qry):
    with mm.SeedIndex([s for _, s in ic.read_fasta(os.path.join(ic.DATA, tgt))], engine=engine) as ix:
        assert check_case(engine, ix, ic.read_fasta(os.path.join(ic.DATA, qry)), case) >= 1
        assert ix.view()["uploads"] == 0


def test_mapper_gives_the_same_paf_on_either_index(engine, tmp_path):
    ref_fa, reads_fa = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fa")
    sim_reads.simulate(ref_fa, reads_fa, seed=8, n_reads=40, len_lo=3_000, len_hi=15_000, chr_len=400_000)
    refs, reads = ic.read_fasta(ref_fa), ic.read_fasta(reads_fa)
    names = [n for n, _ in refs]
    with mm.SeedIndex([s for _, s in refs], engine=engine) as dev, mm.SeedIndex([s for _, s in refs]) as host:
        out = {(which, sod): mm.map_reads(engine, ix, names, reads, opt=mm.map_opt(seeding_on_device=sod))
               for which, ix in (("dev", dev), ("host", host)) for sod in (0, 1)}
        want = out[("host", 0)]
        assert want[0].count("\n") >= 30 and want[1]["n_mapped"] >= 30
        for key, (paf, st) in out.items():
            assert paf == want[0], key
            assert all(st[f] == want[1][f] for f in ("n_anchors", "n_chains", "n_rechained", "n_mapped", "n_reads")), key
        assert dev.view()["uploads"] == 0 and host.view()["uploads"] == 1
