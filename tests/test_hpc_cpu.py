"""Homopolymer-compressed minimizers (minimap2 -H, preset map-pb) on the host, without a GPU (csrc/seeding.cpp): the sketch against what
the reference's mm_sketch(..., is_hpc = 1) returned (tests/golden/hpc/sketch_*.npz, tests/tools/gen_golden_hpc.py) and against the
by-position model the device kernels implement (tests/hpc_cases.py), the index built with the flag, and match collection against the
reference's recordings under -H -k19 (tests/golden/hpc/seeds)."""
import ctypes as C
import os

import numpy as np
import pytest

import golden_io
import hpc_cases as hc
import orc
import sim_reads
from test_seeding_cpu import DATA, read_fasta

mm = pytest.importorskip("mm2gb_amd")
PB = dict(k=19, w=10, hpc=True)


def span(xy):
    return (xy[:, 0] & np.uint64(0xff)).astype(np.int64)


@pytest.mark.parametrize("k,w", hc.KW)
def test_host_sketch_equals_the_reference(k, w):
    seqs, want = hc.load_sketch(k, w)
    assert seqs == hc.sequences(1), "the committed generator no longer makes the golden's sequences"
    assert min(len(s) for s in seqs) == 1 and any(b"N" in s for s in seqs) and any(s != s.upper() for s in seqs)
    for r, (s, x) in enumerate(zip(seqs, want)):
        got = mm.sketch(s, w, k, rid=r, hpc=True)
        assert got.shape == x.shape and np.array_equal(got, x), f"k={k} w={w} sequence {r}"
        assert np.array_equal(mm.sketch(s, w, k, rid=r, hpc=False), mm.sketch(s, w, k, rid=r))     # flag 0 is the old entry point


def test_the_golden_sketches_exercise_compression():
    """At least half of all minimizers span more than k bases, and in at least one sequence k-mers were dropped for spanning 256 or more
    (the by-position steps say which: counted, l >= k, no value)."""
    n = over = 0
    for k, w in hc.KW:
        _, want = hc.load_sketch(k, w)
        n += sum(len(x) for x in want)
        over += sum(int((span(x) > k).sum()) for x in want)
    assert n > 10_000 and 2 * over >= n
    seqs, _ = hc.load_sketch(19, 10)
    dropped = [sum(1 for x, _, l in hc.steps_by_position(s, 19) if x == hc.NONE and l >= 19) for s in seqs]
    assert max(dropped) >= 19


@pytest.mark.parametrize("k,w", hc.KW)
def test_by_position_model_equals_the_host_sketch(k, w):
    """The formulation of csrc/seed_kernels.hip's sketch kernels in their HPC form (boundaries, run ends from the next boundary, spans as differences of
    positions), in Python: equal to the serial loop of csrc/seeding.cpp."""
    for r, s in enumerate(hc.load_sketch(k, w)[0] + [b"", b"N", b"a" * 300 + b"CgT" * 30, b"ACGT" * 100]):
        assert np.array_equal(hc.model_sketch(s, w, k, rid=r), mm.sketch(s, w, k, rid=r, hpc=True)), f"k={k} w={w} sequence {r}"


@pytest.mark.skipif(not os.path.exists(os.path.join(orc.REF_DIR, "libminimap2ref.so")), reason="the reference build (oracle/_ref) is not here")
def test_host_sketch_equals_mm_sketch_on_fresh_sequences():
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_golden_hpc", os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools", "gen_golden_hpc.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    lib = gen.ref_lib()
    seqs = hc.sequences(int.from_bytes(os.urandom(4), "little"), n_seq=14)
    for k, w in hc.KW:
        for r, s in enumerate(seqs):
            assert np.array_equal(mm.sketch(s, w, k, rid=r, hpc=True), gen.ref_sketch(lib, s, w, k, rid=r)), f"k={k} w={w}: {s!r}"


def test_edge_cases():
    hp = lambda s, w=3, k=4, **kw: mm.sketch(s, w, k, hpc=True, **kw)          # noqa: E731
    assert hp(b"").shape == (0, 2)
    assert hp(b"AAACCCGGG").shape == (0, 2) and len(mm.sketch(b"AAACCCGGG", 3, 4)) > 0         # nine bases, three runs: shorter than k runs
    assert hp(b"A" * 5000).shape == (0, 2) and hp(b"A" * 5000, 10, 15).shape == (0, 2)         # one run
    rng = np.random.default_rng(3)
    no_rep = bytearray()
    while len(no_rep) < 600:
        c = b"ACGT"[int(rng.integers(0, 4))]
        if not no_rep or no_rep[-1] != c:
            no_rep.append(c)
    for k, w in [(4, 3), (15, 10), (19, 10)]:                                                   # no base repeats: nothing to compress
        a = hp(bytes(no_rep), w, k)
        assert len(a) > 0 and np.array_equal(a, mm.sketch(bytes(no_rep), w, k)) and np.all(span(a) == k)
    # a sequence that ends inside a run: the run's end is the sequence's last base
    s = b"ACGTTGCA" * 4 + b"GATTACA" + b"C" * 9
    a = hp(s, 1, 5)
    assert int(a[-1, 1] & np.uint64(0xffffffff)) >> 1 == len(s) - 1 and np.array_equal(a, hc.model_sketch(s, 1, 5))
    # an N inside what would be one run makes two runs, and empties the queue of run lengths
    one, two = hp(b"ACGTTGCATG" + b"AAAAA" + b"CTGACTG", 1, 4), hp(b"ACGTTGCATG" + b"AANAA" + b"CTGACTG", 1, 4)
    assert not np.array_equal(one, two) and np.array_equal(two, hc.model_sketch(b"ACGTTGCATG" + b"AANAA" + b"CTGACTG", 1, 4))
    assert [st[2] for st in hc.steps_by_position(b"AAANAA", 2)] == [1, 0, 1]                    # run, N, run
    # lower and upper case continue a run
    mixed = b"ACGTTGCATGCCATGAaaAAaAcccCCgGtT" * 8
    assert np.array_equal(hp(mixed, 5, 6), hp(mixed.upper(), 5, 6)) and np.array_equal(hp(mixed, 5, 6), hp(mixed.lower(), 5, 6))
    assert np.all(hp(mixed, 5, 6, rid=7)[:, 1] >> np.uint64(32) == 7)
    # a span of 256 or more has no value: the six 6-run k-mers that hold the long run span 250 + 5 = 255 bases (kept) or 251 + 5 (dropped)
    kept, gone = hp(b"ACGTGT" * 5 + b"A" * 250 + b"CGTCA" + b"GTCATG" * 5, 1, 6), hp(b"ACGTGT" * 5 + b"A" * 251 + b"CGTCA" + b"GTCATG" * 5, 1, 6)
    assert span(kept).max() == 255 and span(gone).max() < 255 and len(gone) == len(kept) - 6
    L = mm.lib()
    ptr, n = C.c_void_p(), C.c_int64()
    assert L.mm2gb_sketch_flag(b"ACGT", 4, 3, 4, 0, 2, C.byref(ptr), C.byref(n)) != 0 and "flag" in L.mm2gb_last_error().decode()
    assert mm.preset("map-pb") == mm.preset("map10k") == PB
    with pytest.raises(mm.Mm2gbError):
        mm.preset("ava-pb")


@pytest.mark.parametrize("k,w", [(4, 3), (11, 10), (19, 10), (28, 19)])
def test_hpc_index_lookup_against_a_dictionary_of_the_sketch(k, w):
    rng = np.random.default_rng(200 + k)
    refs = [hc.hpc_seq(rng, n) for n in (9000, 4000, 1)]
    table = {}
    for rid, s in enumerate(refs):
        sk = mm.sketch(s, w, k, rid=rid, hpc=True)
        assert np.all(np.diff(sk[:, 1].astype(np.int64)) > 0), "y not strictly ascending within a sequence: the device build's sort relies on it"
        for x, y in sk:
            table.setdefault(int(x) >> 8, []).append(int(y))
    reads = [refs[0][2000:5000], refs[1][500:2500].lower(), hc.hpc_seq(rng, 1500), refs[0][:k], b""]
    with mm.SeedIndex(refs, k=k, w=w, threads=2, hpc=True) as ix, mm.SeedIndex(refs, k=k, w=w, threads=2) as plain:
        assert ix.hpc is True and plain.hpc is False
        assert mm.lib().mm2gb_index_flag(ix._h) == 1 and mm.lib().mm2gb_index_flag(plain._h) == 0 and mm.lib().mm2gb_index_flag(None) < 0
        assert ix.size() == (len(table), sum(len(v) for v in table.values()))
        v = ix.view()
        for a, b in zip(v["first"][:-1], v["first"][1:]):
            assert np.all(np.diff(v["where"][a:b].astype(np.int64)) > 0)
        n_found = 0
        for rd in reads:
            m = ix.matches(rd, mid_occ=1 << 30, max_max_occ=1 << 30, occ_dist=0, q_occ_frac=0.0)       # the index's flag sketches the read
            want_seeds, want_hits = [], []
            for x, y in mm.sketch(rd, w, k, hpc=True):
                occ = table.get(int(x) >> 8)
                if occ:
                    want_seeds.append((len(occ), int(y) & 0xffffffff, int(x) & 0xff))
                    want_hits += sorted(occ)
            assert [(int(a), int(b), int(c)) for a, b, c in m["seeds"][:, :3]] == want_seeds
            assert m["hits"].tolist() == want_hits
            n_found += len(want_seeds)
        assert n_found > 50
    L = mm.lib()
    assert L.mm2gb_index_build_flag(15, 10, 4, 0, None, None, 1) is None and "flag" in L.mm2gb_last_error().decode()
    assert L.mm2gb_index_build_gpu_flag(None, 15, 10, 1, 0, None, None) is None


def check_reads(index, reads, case):
    mid_occ = index.mid_occ()
    got = []
    for k, (_, seq) in enumerate(reads):
        path = os.path.join(hc.HPC, "seeds", f"{case}_{k}.npz")
        if not os.path.exists(path):
            continue
        g = golden_io.load_seeds(path)
        assert g["qlen"] == len(seq)
        m = index.matches(seq, mid_occ)
        assert np.array_equal(m["seeds"], g["seeds"]), f"{case} read {k}: seeds"
        assert np.array_equal(m["hits"], g["hits"]), f"{case} read {k}: hits"
        assert m["rep_len"] == g["rep_len"] and np.array_equal(m["mini_pos"], g["mini_pos"]), f"{case} read {k}: rep_len / mini_pos"
        a = mm.collect_seeds_host(0, [dict(seeds=m["seeds"], hits=m["hits"], qlen=len(seq))], threads=1)[0]
        assert a.shape == g["a"].shape and np.array_equal(a, g["a"]), f"{case} read {k}: anchors"
        got.append(g)
    return got


@pytest.mark.parametrize("case,tgt,qry", [("mt", "MT-human.fa", "MT-orang.fa"), ("inv", "t-inv.fa", "q-inv.fa")])
def test_matches_equal_the_recordings_reference_pairs(case, tgt, qry):
    with mm.SeedIndex([s for _, s in read_fasta(os.path.join(DATA, tgt))], **mm.preset("map-pb")) as ix:
        got = check_reads(ix, read_fasta(os.path.join(DATA, qry)), case)
        assert len(got) == hc.meta()[case]["records"] >= 1
        assert all((g["seeds"][:, 2] & 0xff).max() > 19 for g in got)                                 # spans beyond k reached the seeds


def test_matches_equal_the_recordings_simulated_reads(tmp_path):
    ref_fa, reads_fa = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fa")
    sim_reads.simulate(ref_fa, reads_fa, seed=5, n_reads=150, len_lo=3_000, len_hi=20_000)             # as tests/tools/gen_golden_hpc.py
    info = hc.meta()["sim"]
    with mm.SeedIndex([s for _, s in read_fasta(ref_fa)], **mm.preset("map-pb")) as ix:
        got = check_reads(ix, read_fasta(reads_fa), "sim")
        assert len(got) == len(info["reads"]) and [g["rep_len"] for g in got] == info["rep_len"]
        # of the 150 reads info["n_rep_len_positive"] have dropped minimizers under compression; the test requires what the reference gave
        assert sum(g["rep_len"] > 0 for g in got) == min(6, info["n_rep_len_positive"]) >= 3
        assert max(int(g["seeds"][:, 0].max()) for g in got) > ix.mid_occ()
