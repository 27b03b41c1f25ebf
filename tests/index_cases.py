"""Inputs and a numpy model of the minimizer index for tests/test_index_api_cpu.py and tests/test_gpu_index.py: the sequences, and the
index's four arrays reconstructed from mm.sketch() by the definitions of csrc/seeding.cpp (mm2gb_index_build, SeedIndex::build_buckets)."""
import functools
import glob
import os

import numpy as np

import golden_io
import sim_reads

DATA = os.path.join(golden_io.GOLD, "data")
KW = [(15, 10), (4, 3), (28, 19), (15, 1)]
ARRAYS = ("keys", "first", "where", "bucket")
ACGT = np.frombuffer(b"ACGT", np.uint8)


def read_fasta(path):
    recs, name, seq = [], None, []
    with open(path, "rb") as fh:
        for ln in fh:
            ln = ln.strip()
            if ln.startswith(b">"):
                if name is not None:
                    recs.append((name, b"".join(seq)))
                name, seq = ln[1:].split()[0].decode(), []
            elif ln:
                seq.append(ln)
    if name is not None:
        recs.append((name, b"".join(seq)))
    return recs


def rand_seq(rng, n):
    return bytes(rng.choice(ACGT, n))


@functools.lru_cache(maxsize=None)
def inputs():
    """name -> list of sequences (bytes)."""
    rng = np.random.default_rng(77)
    golden = [s for f in sorted(glob.glob(os.path.join(DATA, "*.fa"))) for _, s in read_fasta(f)]
    genome = [c.tobytes() for c in sim_reads.make_genome(rng, n_chr=3, chr_len=100_000, n_rep_families=3, rep_len=500, copies=12, tandem=1)]
    twin = rand_seq(rng, 2_000)
    odd = [b"", b"N" * 300, b"ACG", rand_seq(rng, 1_500).lower(), rand_seq(rng, 1_500).replace(b"T", b"U"), twin, b"", b"", twin,
           rand_seq(rng, 700) + b"N" * 40 + rand_seq(rng, 700), b""]
    return {"golden": golden, "genome": genome, "odd": odd, "none": [], "empty_only": [b"", b""]}


def bucket_bits(k, n_keys):
    bits = 1
    while bits < 2 * k and (1 << bits) < n_keys:
        bits += 1
    return min(bits, 26)


@functools.lru_cache(maxsize=None)
def model(mm_name, name, k, w):
    """The index of inputs()[name] from the host sketch: dict(keys, first, where, bucket, bucket_shift, n_keys, n_occ, n_bucket, sketches)."""
    import importlib
    mm = importlib.import_module(mm_name)
    sk = [mm.sketch(s, w, k, rid=i) for i, s in enumerate(inputs()[name])]
    xy = np.concatenate(sk) if sk else np.zeros((0, 2), np.uint64)
    xy = xy.reshape(-1, 2)
    key, y = xy[:, 0] >> np.uint64(8), xy[:, 1]
    order = np.lexsort((y, key))                                   # by (x >> 8, y): the comparator of mm2gb_index_build
    key, where = key[order], y[order]
    keys, first = np.unique(key, return_index=True)
    first = np.append(first, len(key)).astype(np.int64)
    bits = bucket_bits(k, len(keys))
    shift = 2 * k - bits
    # bucket[b] = first key with (key >> shift) >= b, for all 2^bits + 1 entries
    bucket = np.searchsorted(keys >> np.uint64(shift), np.arange((1 << bits) + 1, dtype=np.uint64), side="left").astype(np.uint32)
    return dict(keys=keys.astype(np.uint64), first=first, where=where.astype(np.uint64), bucket=bucket, bucket_shift=shift, n_keys=len(keys),
                n_occ=len(where), n_bucket=len(bucket), bits=bits, sketches=sk)


def same_index(got, want, what):
    for f in ("n_keys", "n_occ", "n_bucket", "bucket_shift"):
        assert got[f] == want[f], f"{what}: {f} {got[f]} != {want[f]}"
    for a in ARRAYS:
        assert got[a].dtype == want[a].dtype and np.array_equal(got[a], want[a]), f"{what}: {a}"
