"""Seeding on the device (csrc/seed_kernels.hip: mm2gb_sketch_gpu, mm2gb_collect_matches_gpu, map_opt(seeding_on_device=1)) against the host
functions of csrc/seeding.cpp, which tests/test_seeding_cpu.py pins to the reference's recordings, and against those recordings.  Every
comparison is exact."""
import ctypes as C
import glob
import hashlib
import json
import os

import numpy as np
import pytest

import golden_io
import sim_reads
from test_seeding_cpu import DATA, SEEDS, read_fasta

pytestmark = pytest.mark.gpu

mm = pytest.importorskip("mm2gb_amd")
GOLD = golden_io.GOLD
TILE = 256                      # positions per workgroup of the sketch kernels (seed_dev.h: TB)
ACGT = np.frombuffer(b"ACGT", np.uint8)


@pytest.fixture(scope="module")
def engine():
    with mm.Engine() as e:
        yield e


def rand_seq(rng, n):
    return bytes(rng.choice(ACGT, n))


def n_skipped(seq, k):
    """Positions at which the host loop `continue`s: the k-mer (or the partial word at the start) equals its reverse complement."""
    code = {65: 0, 67: 1, 71: 2, 84: 3, 85: 3, 97: 0, 99: 1, 103: 2, 116: 3, 117: 3}
    fwd = rev = n = 0
    mask, top = (1 << 2 * k) - 1, 2 * (k - 1)
    for ch in seq:
        c = code.get(ch)
        if c is None:
            continue
        fwd, rev = (fwd << 2 | c) & mask, rev >> 2 | (3 ^ c) << top
        n += fwd == rev
    return n


def has_twins(xy, w):
    """Two minimizers of equal value closer than a window."""
    x, pos = xy[:, 0], (xy[:, 1] & 0xffffffff) >> 1
    for i in range(len(x) - 1):
        j = i + 1
        while j < len(x) and abs(int(pos[j]) - int(pos[i])) < w:
            if x[j] == x[i]:
                return True
            j += 1
    return False


@pytest.mark.parametrize("k,w", [(4, 3), (7, 5), (11, 10), (15, 10), (21, 11), (28, 19), (15, 1), (2, 50)])
def test_sketch_equals_the_host_sketch(engine, k, w):
    rng = np.random.default_rng(1000 + 31 * k + w)
    seqs = [s for f in sorted(glob.glob(os.path.join(DATA, "*.fa"))) for _, s in read_fasta(f)]
    seqs += [b""] + [rand_seq(rng, max(0, n)) for n in (k - 1, k, w + k - 2, w + k - 1, w + k)]
    seqs += [b"N" * 300, rand_seq(rng, 200) + b"N" * (w + k - 3 if w + k > 3 else 1) + rand_seq(rng, 200) + b"N" * (w + k + 40) + rand_seq(rng, 300)]
    seqs += [rand_seq(rng, 900).lower(), rand_seq(rng, 900).replace(b"T", b"U"), b"AC" * 600, b"GATTACA" * 300, b"AT" * 500, b"ACGT" * 400]
    seqs += [rand_seq(rng, 300_000)]
    lens = [TILE * m + d for m in (1, 2, 3) for d in (-1, 0, 1)] + [TILE - k, TILE + k, TILE - w, TILE + w, 2 * TILE - w - k, 2 * TILE + w + k]
    seqs += [rand_seq(rng, lens[i % len(lens)] if i < 4 * len(lens) else int(rng.integers(0, 4 * TILE))) for i in range(2000)]
    # an ambiguous base directly before, directly after and in the middle of a stretch of k-mers equal to their reverse complement (even k), at
    # a workgroup's edge: each of the five begins at a multiple of TILE in the batch (a filler before it), an empty sequence between two of them
    edge_rng = np.random.default_rng(77)
    r600 = bytearray(rand_seq(edge_rng, 600))
    r600[TILE - 1:TILE + 2] = b"NNN"
    edge = [b"AT" * 120 + b"N" + b"ACGT" * 70, b"N" + b"AT" * 127 + b"N" + b"AT" * 200, bytes(r600),
            b"AT" * 128 + b"N" + b"TA" * 128, b"ACGT" * 64 + b"AN" + b"CGTA" * 64]
    for j, s in enumerate(edge):
        seqs += [rand_seq(edge_rng, -sum(map(len, seqs)) % TILE), s] + ([b""] if j == 1 else [])
    rid = np.arange(len(seqs), dtype=np.uint32) * 7 + 1
    got = engine.sketch(seqs, w=w, k=k, rid=rid)
    twins = skipped = 0
    for r, s in enumerate(seqs):
        want = mm.sketch(s, w, k, rid=int(rid[r]))
        assert np.array_equal(got[r], want), f"sequence {r} (length {len(s)}): {len(got[r])} pairs, host {len(want)}"
        if len(s) < 5000:
            twins += has_twins(want, w)
            skipped += n_skipped(s, k)
    assert skipped > 0 or k % 2 == 1          # (a k-mer of odd length is never its own reverse complement)
    assert twins > 0 or w == 1                # (a window of one k-mer holds no second one)
    assert all(np.array_equal(a, mm.sketch(s, w, k)) for a, s in zip(engine.sketch(seqs[:40], w=w, k=k), seqs[:40]))     # rid = None


def check_case(engine, index, reads, case):
    mid_occ = index.mid_occ()
    got = engine.collect_matches(index, [s for _, s in reads], mid_occ)
    n = 0
    for k, (_, seq) in enumerate(reads):
        path = os.path.join(SEEDS, f"{case}_{k}.npz")
        if not os.path.exists(path):
            continue
        g, m = golden_io.load_seeds(path), got[k]
        assert g["qlen"] == len(seq) == m["qlen"]
        assert np.array_equal(m["seeds"], g["seeds"]) and np.array_equal(m["hits"], g["hits"]), f"{case} read {k}"
        assert m["rep_len"] == g["rep_len"] and np.array_equal(m["mini_pos"], g["mini_pos"]), f"{case} read {k}: rep_len / mini_pos"
        n += 1
    return n


@pytest.mark.parametrize("case,tgt,qry", [("mt", "MT-human.fa", "MT-orang.fa"), ("inv", "t-inv.fa", "q-inv.fa"),
                                          ("mt_x_self", "MT-human.fa", "MT-human.fa"), ("mt_x_smaller", "MT-orang.fa", "MT-human.fa")])
def test_matches_equal_the_references_recordings(engine, case, tgt, qry):
    with mm.SeedIndex([s for _, s in read_fasta(os.path.join(DATA, tgt))]) as ix:
        assert check_case(engine, ix, read_fasta(os.path.join(DATA, qry)), case) >= 1


def test_matches_equal_the_recordings_simulated_and_self(engine, tmp_path):
    ref_fa, reads_fa = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fa")
    sim_reads.simulate(ref_fa, reads_fa, seed=5, n_reads=150, len_lo=3_000, len_hi=20_000)     # as tests/test_seeding_cpu.py
    with mm.SeedIndex([s for _, s in read_fasta(ref_fa)]) as ix:
        assert check_case(engine, ix, read_fasta(reads_fa), "sim") == 9
    rng = np.random.default_rng(9)
    chrs = sim_reads.make_genome(rng, n_chr=3, chr_len=20_000, n_rep_families=2, rep_len=300, copies=9, tandem=0)
    seqs = [c.tobytes() for c in chrs]
    with mm.SeedIndex(seqs) as ix:
        assert check_case(engine, ix, [(None, s) for s in seqs], "self_x") == 3


def same_matches(got, want, what):
    for r, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a["seeds"], b["seeds"]), f"{what} read {r}: seeds ({len(a['seeds'])} vs {len(b['seeds'])})"
        assert np.array_equal(a["hits"], b["hits"]), f"{what} read {r}: hits"
        assert a["rep_len"] == b["rep_len"] and np.array_equal(a["mini_pos"], b["mini_pos"]) and a["qlen"] == b["qlen"], f"{what} read {r}"


def test_matches_equal_the_host_form_under_options_that_force_every_filter(engine, tmp_path):
    ref_fa, reads_fa = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fa")
    sim_reads.simulate(ref_fa, reads_fa, seed=5, n_reads=150, len_lo=3_000, len_hi=20_000)
    reads = [s for _, s in read_fasta(reads_fa)]
    assert len(reads) == 150
    with mm.SeedIndex([s for _, s in read_fasta(ref_fa)]) as ix:
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
        # a streak that reaches the cap of 128 kept seeds: one crafted read, a repeat unit of the genome many times over with random spacers
        # of 40 bases (every minimizer of the unit occurs more than 3 times in the reference; occ_dist = 1 asks for one seed per base)
        ref = read_fasta(ref_fa)[0][1]
        rng = np.random.default_rng(3)
        crafted = [b"".join(ref[100_000 + 61 * i:100_000 + 61 * i + 400] for i in range(12)) * 3, rand_seq(rng, 5000)]
        kw = dict(mid_occ=0 + 1, max_max_occ=4095, occ_dist=1, q_occ_frac=0.0)
        same_matches(engine.collect_matches(ix, crafted + reads[:20], **kw), [ix.matches(s, **kw) for s in crafted + reads[:20]], "cap")


def map_both(engine, ix, names, reads, **opt):
    dev = mm.map_reads(engine, ix, names, reads, opt=mm.map_opt(seeding_on_device=1, **opt))
    host = mm.map_reads(engine, ix, names, reads, opt=mm.map_opt(**opt))
    for key in ("n_anchors", "n_chains", "n_rechained", "n_mapped", "n_reads"):
        assert dev[1][key] == host[1][key], key
    assert dev[0] == host[0]
    return dev


@pytest.mark.parametrize("case,tgt,qry", [("mt", "MT-human.fa", "MT-orang.fa"), ("inv", "t-inv.fa", "q-inv.fa"), ("q2", "t2.fa", "q2.fa")])
def test_mapper_reference_pairs(engine, case, tgt, qry):
    refs, reads = read_fasta(os.path.join(DATA, tgt)), read_fasta(os.path.join(DATA, qry))
    with mm.SeedIndex([s for _, s in refs]) as ix:
        paf, st = map_both(engine, ix, [n for n, _ in refs], reads)
    assert paf == open(os.path.join(GOLD, f"real_{case}_inf.paf")).read() and st["n_rmq_tied"] == 0


@pytest.mark.parametrize("rechain_on_device", [1, 0, -1])
def test_mapper_simulated_long_reads(engine, tmp_path, rechain_on_device):
    meta = json.load(open(os.path.join(GOLD, "sim160.json")))
    ref, reads = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fa")
    sim_reads.simulate(ref, reads, seed=meta["seed"], n_reads=meta["n_reads"], len_lo=meta["len_lo"], len_hi=meta["len_hi"], tandem=meta["tandem"])
    assert hashlib.md5(open(reads, "rb").read()).hexdigest() == meta["reads_md5"]
    refs, rd = read_fasta(ref), read_fasta(reads)
    want = open(os.path.join(GOLD, "sim160_inf.paf")).read()
    with mm.SeedIndex([s for _, s in refs]) as ix:
        paf, st = map_both(engine, ix, [n for n, _ in refs], rd, rechain_on_device=rechain_on_device)
        assert paf == want and st["n_rechained"] >= 100
        if rechain_on_device == 0:
            with mm.Engine() as e2:
                paf2, st2 = mm.map_reads_stream([engine, e2], ix, [n for n, _ in refs], rd, opt=mm.map_opt(seeding_on_device=1, host_threads=8), chunk_bases=600_000)
                assert paf2 == want and st2["n_anchors"] == st["n_anchors"] and st2["n_chains"] == st["n_chains"]
                assert mm.map_reads_multi([engine, e2], ix, [n for n, _ in refs], rd, opt=mm.map_opt(seeding_on_device=1, host_threads=8))[0] == want


@pytest.mark.parametrize("name,tgt,qry,flag", [("mt_for", "MT-human.fa", "MT-orang.fa", 0x100000), ("mt_rev", "MT-human.fa", "MT-orang.fa", 0x200000),
                                               ("inv_rev", "t-inv.fa", "q-inv.fa", 0x200000)])
def test_mapper_strand_restricted_runs(engine, name, tgt, qry, flag):
    refs, reads = read_fasta(os.path.join(DATA, tgt)), read_fasta(os.path.join(DATA, qry))
    with mm.SeedIndex([s for _, s in refs]) as ix:
        paf, _ = map_both(engine, ix, [n for n, _ in refs], reads, flag=flag)
    assert paf == open(os.path.join(GOLD, "seeds", name + ".paf")).read()


def test_mapper_odd_input(engine):
    refs = read_fasta(os.path.join(DATA, "MT-human.fa"))
    good = read_fasta(os.path.join(DATA, "MT-orang.fa"))[0][1]
    rng = np.random.default_rng(2)
    reads = [("empty", b""), ("short", b"ACGTACGTAC"), ("n_only", b"N" * 500), ("random", rand_seq(rng, 3000)), ("upper", good), ("lower", good.lower()),
             ("with_n", good[:8000] + b"N" * 50 + good[8050:])]
    with mm.SeedIndex([s for _, s in refs]) as ix:
        paf, st = map_both(engine, ix, [n for n, _ in refs], reads)
        assert mm.map_reads(engine, ix, [n for n, _ in refs], [], opt=mm.map_opt(seeding_on_device=1))[0] == ""
        for odd in ([("empty", b"")], [("n_only", b"N" * 500), ("short", b"ACGT")]):
            assert mm.map_reads(engine, ix, [n for n, _ in refs], odd, opt=mm.map_opt(seeding_on_device=1))[0] == ""
    by = {ln.split("\t")[0]: ln for ln in paf.splitlines()}
    assert set(by) == {"upper", "lower", "with_n"} and st["n_mapped"] == 3
    assert by["upper"] == open(os.path.join(GOLD, "real_mt_inf.paf")).read().strip().replace("MT_orang", "upper", 1)


def test_batches_of_different_sizes_and_indexes_on_one_engine_and_bad_arguments(engine):
    """Arenas reused across batches of different sizes and (k, w); every index has its own device copy; an index destroyed while the engine lives,
    then a new one (which may sit at the same host address)."""
    rng = np.random.default_rng(12)
    ref = [rand_seq(rng, 60_000), rand_seq(rng, 9_000)]
    big = [ref[0][i:i + 4000] for i in range(0, 50_000, 1500)] + [b"", b"N" * 100]
    small = [ref[1][100:2100], ref[0][5:900]]
    for k, w, reads in ((15, 10, big), (11, 5, small), (15, 10, big), (21, 11, small)):
        ix = mm.SeedIndex(ref, k=k, w=w)
        same_matches(engine.collect_matches(ix, reads, mid_occ=ix.mid_occ()), [ix.matches(s, ix.mid_occ()) for s in reads], f"k={k} w={w}")
        ix.close()                                                    # mm2gb_index_destroy with the engine alive
    with mm.SeedIndex(ref) as ix1, mm.SeedIndex(ref[::-1], k=13, w=7) as ix2:
        assert mm.lib().mm2gb_index_to_device(ix1._h, 0) == 0 and mm.lib().mm2gb_index_to_device(ix1._h, 0) == 0
        for ix in (ix1, ix2, ix1):
            same_matches(engine.collect_matches(ix, small, mid_occ=10), [ix.matches(s, 10) for s in small], "two indexes")
        L = mm.lib()
        off = np.array([0, 4], np.int64)
        mini_off = np.zeros(2, np.int64)
        ptr = C.c_void_p()
        for w, k, o in ((0, 15, off), (10, 29, off), (10, 15, np.array([1, 4], np.int64)), (10, 15, np.array([0, 4, 2], np.int64))):
            assert L.mm2gb_sketch_gpu(engine._h, w, k, len(o) - 1, o.ctypes.data, b"ACGT", None, mini_off.ctypes.data if len(o) == 2 else np.zeros(3, np.int64).ctypes.data, C.byref(ptr)) != 0
            assert "mm2gb_sketch_gpu" in L.mm2gb_last_error().decode()
        opt = mm.SeedOpt(10, 4095, 500, 0.01)
        m = mm.MatchBatch()
        assert L.mm2gb_collect_matches_gpu(engine._h, None, C.byref(opt), 1, off.ctypes.data, b"ACGT", C.byref(m)) != 0
        assert "mm2gb_collect_matches_gpu" in L.mm2gb_last_error().decode()
        for o in (np.array([1, 4], np.int64), np.array([0, 4, 2], np.int64)):
            assert L.mm2gb_collect_matches_gpu(engine._h, ix1._h, C.byref(opt), len(o) - 1, o.ctypes.data, b"ACGT", C.byref(m)) != 0
            assert "mm2gb_collect_matches_gpu" in L.mm2gb_last_error().decode()
        assert engine.sketch([]) == [] and engine.collect_matches(ix1, [], mid_occ=10) == []
