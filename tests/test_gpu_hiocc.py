"""The device forms of the index, the match selection, seeds-to-anchors and the mapper where minimizers occur 10^3 to 10^7 times
(csrc/index_kernels.hip: k_ix_hist / k_ix_pick over all four digit passes; csrc/seed_kernels.hip: k_m_select above bit 40, streaks longer
than a workgroup pass, n > max_max_occ, k_m_qflt and k_m_gather on long runs) against the host forms of csrc/seeding.cpp, which
tests/test_hiocc_cpu.py pins to the reference's recordings on the same input (tests/hiocc_cases.py, tests/golden/hiocc), against a numpy
model of mid_occ, and against those recordings.  Every comparison is exact."""
import functools
import os

import numpy as np
import pytest

import hiocc_cases as hc
import index_cases as ic
from test_gpu_index import CLAMPS, FRACS, big_seq
from test_gpu_seeding import rand_seq, same_matches
from test_hiocc_cpu import check_inputs, host

pytestmark = pytest.mark.gpu

mm = pytest.importorskip("mm2gb_amd")
PB = dict(k=19, w=10, hpc=True)
LONG_A = 17_000_000                 # a run of A before big_seq(): at k = 2, w = 1 one key with more than 2^24 occurrences
STAT_FIELDS = ("n_anchors", "n_chains", "n_rechained", "n_mapped", "n_reads")


@pytest.fixture(scope="module")
def engine():
    with mm.Engine() as e:
        yield e


@pytest.fixture(scope="module")
def host_ix():
    with mm.SeedIndex(hc.genome(), threads=8) as ix:
        yield ix


@pytest.fixture(scope="module")
def dev_ix(engine):
    with mm.SeedIndex(hc.genome(), engine=engine) as ix:
        yield ix


# ---------------------------------------------------------------------------------------------------------------- mid_occ
SELECT = {"big k=4": (lambda: [big_seq()], 4, 3), "big k=6": (lambda: [big_seq()], 6, 5), "satellites": (hc.genome, 15, 10),
          "long run k=2": (lambda: [b"A" * LONG_A + big_seq()], 2, 1)}


def bytes_of(values, b):
    """Byte b of the counts behind mid_occ values (a value is a count + 1)."""
    return [(v - 1) >> (8 * b) & 255 for v in values]


# (the index with the long run is built on the device only: its host build takes seconds)
@pytest.mark.parametrize("name,on_device", [(n, d) for n in SELECT for d in (True, False) if d or n != "long run k=2"])
def test_mid_occ_at_every_rank_equals_the_host_value_and_the_model(engine, name, on_device):
    """frac = (n - r - 0.5) / n asks for rank r.  The host's values -- which the device's must equal -- are proven to need every pass:
    digits other than zero at shift 8, 16 and 24, so the prefix filter of k_ix_hist rejects counts and k_ix_pick carries a rank on."""
    seqs, k, w = SELECT[name]
    with mm.SeedIndex(seqs(), k=k, w=w, threads=8, engine=engine if on_device else None) as ix:
        first = ix.view()["first"]
        cnt = np.diff(first)
        n = len(cnt)
        assert n == ix.size()[0] and int(cnt.sum()) == ix.size()[1] and cnt.min() > 0
        want = [ix.mid_occ(f, 1, 1 << 30) for _, f in hc.rank_fracs(n)]
        if name == "big k=4":
            assert n <= 200 and len(set(bytes_of(want, 1))) >= 5
        elif name == "satellites":
            assert cnt.max() >= 65_536 and any(bytes_of(want, 2))
        elif name == "long run k=2":
            assert cnt.max() >= 1 << 24 and all(bytes_of(want, 2)) and bytes_of(want, 3)[-1] > 0
        for (r, f), v in zip(hc.rank_fracs(n), want):
            assert v == hc.mid_occ_model(first, f, 1, 1 << 30), f"host, rank {r}"
            assert ix.mid_occ(f, 1, 1 << 30, engine=engine) == v, f"rank {r} of {n}"
        assert want[0] == cnt.min() + 1 and want[-1] == cnt.max() + 1
        if name == "satellites":
            for f in FRACS:
                for c in CLAMPS:
                    assert ix.mid_occ(f, *c, engine=engine) == ix.mid_occ(f, *c) == hc.mid_occ_model(first, f, *c), f"frac {f} clamps {c}"
        assert ix.view()["uploads"] == (0 if on_device else 1)


# ---------------------------------------------------------------------------------------------------------------- index arrays
@functools.lru_cache(maxsize=None)
def host_view(pb):
    with mm.SeedIndex(hc.genome(), threads=8, **(PB if pb else {})) as ix:
        return ix.view()


@pytest.mark.parametrize("pb", [False, True], ids=["plain", "map-pb"])
@pytest.mark.parametrize("chunk", [None, 100_000])
def test_index_arrays_equal_the_host_build(engine, monkeypatch, chunk, pb):
    """Runs of up to 70 000 equal keys through the device's sort and tables, in one chunk and with both arrays cut by chunks of 100 000 bases."""
    if chunk:
        monkeypatch.setenv("MM2GB_INDEX_CHUNK_BASES", str(chunk))
    else:
        monkeypatch.delenv("MM2GB_INDEX_CHUNK_BASES", raising=False)
    want = host_view(pb)
    assert np.diff(want["first"]).max() >= (256 if pb else 65_536)
    with mm.SeedIndex(hc.genome(), engine=engine, **(PB if pb else {})) as ix:
        got = ix.view()
        ic.same_index(got, want, f"chunk {chunk} map-pb {pb}")
        assert (got["k"], got["w"], got["built_on"], got["uploads"], ix.hpc) == (want["k"], want["w"], engine.device, 0, pb)
        dev = ix.fetch_device(engine.device)
        for a in ic.ARRAYS:
            assert np.array_equal(dev[a], want[a]), f"resident {a}"


# ---------------------------------------------------------------------------------------------------------------- matches
def batch_of(picked):
    """The picked reads with an empty read and a random 3 kb read between them, in turn: a streak at a read's end or start has a read
    without matches, or one whose matches are all rare, on its other side."""
    rng = np.random.default_rng(17)
    rd = hc.reads()
    seqs, where = [], {}
    for j, k in enumerate(picked):
        where[k] = len(seqs)
        seqs += [rd[k][1], b"" if j % 2 == 0 else rand_seq(rng, 3000)]
    return seqs, where


def set_options(name, mid_occ):
    return dict(dict(mid_occ=mid_occ), **hc.SETS[name])


def reads_of(name):
    return (hc.C2,) + hc.UNITS37 if name == "everything kept" else tuple(range(11))


@pytest.mark.parametrize("name", list(hc.SETS))
@pytest.mark.parametrize("which", ["host-built", "device-built"])
def test_matches_equal_the_host_form_and_the_recordings(engine, host_ix, dev_ix, which, name):
    ix = host_ix if which == "host-built" else dev_ix
    h = host()
    if name == "default":
        check_inputs()
    picked = reads_of(name)
    seqs, where = batch_of(picked)
    kw = set_options(name, h["mid_occ"])
    assert ix.mid_occ(engine=engine) == h["mid_occ"]
    want = [h["sets"][name][k] if name in h["sets"] else host_ix.matches(hc.reads()[k][1], **kw) for k in picked]
    if name == "everything kept":
        assert sum(len(m["hits"]) for m in want) < 5_000_000
    got = engine.collect_matches(ix, seqs, **kw)
    same_matches([got[where[k]] for k in picked], want, f"{name}, {which} index")
    fill = [r for r in range(len(seqs)) if r not in where.values()]
    same_matches([got[r] for r in fill], [host_ix.matches(seqs[r], **kw) for r in fill], f"{name}, {which} index, the reads between")
    if name == "default":
        for k in picked:
            hc.same_as_recorded(got[where[k]], hc.fixtures()[k], f"{hc.reads()[k][0]}, {which} index")


@pytest.mark.parametrize("name", list(hc.SETS))
def test_matches_equal_the_host_form_with_the_map_pb_preset(engine, name):
    """Homopolymer-compressed minimizers of 19 bases: other keys, other counts, spans that vary; no recordings, host against device."""
    picked = reads_of(name)
    seqs, _ = batch_of(picked)
    with mm.SeedIndex(hc.genome(), threads=8, **PB) as ix:
        mo = ix.mid_occ()
        kw = set_options(name, mo)
        want = [ix.matches(s, **kw) for s in seqs]
        if name == "default":
            cnt = np.diff(ix.view()["first"])
            assert cnt.max() > 4095 and mo > 10 and sum(m["rep_len"] > 0 for m in want) >= 8 and max(int(m["seeds"][:, 0].max()) for m in want if len(m["seeds"])) > 256
        if name == "everything kept":
            assert sum(len(m["hits"]) for m in want) < 5_000_000
        same_matches(engine.collect_matches(ix, seqs, **kw), want, f"{name}, map-pb")


# ---------------------------------------------------------------------------------------------------------------- seeds to anchors
def test_anchors_equal_the_host_form_and_the_recordings(engine):
    """mm2gb_collect_seeds_gpu and the per-read anchor sort on 2 M hits that came from seeding: runs of tens of thousands of hits of one seed."""
    default = host()["sets"]["default"]
    want = mm.collect_seeds_host(0, default, threads=8)
    got = engine.collect_seeds(0, default)
    fx = hc.fixtures()
    assert sum(len(a) for a in want) > 1_000_000
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and np.array_equal(a, b), fx[k]["name"]
        assert len(a) == fx[k]["n_anchors"] and hc.sha(a) == fx[k]["a_sha256"], fx[k]["name"]


# ---------------------------------------------------------------------------------------------------------------- mapper
MAPPED = {}                          # case -> (PAF, stats) of the cases run so far: every later one is compared with all of them


@pytest.mark.parametrize("case", ["host-built host-seeded", "host-built device-seeded", "device-built host-seeded", "device-built device-seeded", "stream"])
def test_mapper_equals_the_reference_on_either_index_with_either_seeding(engine, host_ix, dev_ix, case):
    """Reads with hundreds of thousands of anchors each through seeding, the anchor sort, the chaining DP and the post-pass: the PAF the
    reference printed (max-chain-skip = infinity), whichever index and whichever seeding."""
    rd = hc.reads()
    ix = dev_ix if case.startswith("device-built") else host_ix
    opt = mm.map_opt(seeding_on_device=0 if case.endswith("host-seeded") else 1)
    if case == "stream":
        paf, st = mm.map_reads_stream([engine], ix, hc.CHR_NAMES, rd, opt=opt, chunk_bases=12_000)
    else:
        paf, st = mm.map_reads(engine, ix, hc.CHR_NAMES, rd, opt=opt)
    for other, (paf2, st2) in MAPPED.items():
        assert paf == paf2, f"{case} vs {other}"
        assert all(st[f] == st2[f] for f in STAT_FIELDS), f"{case} vs {other}"
    MAPPED[case] = (paf, st)
    assert st["n_anchors"] == sum(g["n_anchors"] for g in hc.fixtures().values()) and st["n_reads"] == st["n_mapped"] == 11
    assert paf == open(os.path.join(hc.HIOCC, "sat_inf.paf")).read()
