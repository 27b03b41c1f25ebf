"""Looking inside an index (mm2gb_index_view, mm2gb_index_fetch_device) and the refusals of the device build's entry points, without a GPU:
the host build's arrays against a numpy reconstruction from mm.sketch() by the definitions of csrc/seeding.cpp (tests/index_cases.py), and
the premise the device build's sort rests on (csrc/index_kernels.hip): a sequence's sketch emits its pairs in strictly ascending y."""
import ctypes as C

import numpy as np
import pytest

import index_cases as ic

mm = pytest.importorskip("mm2gb_amd")


@pytest.mark.parametrize("k,w", ic.KW)
@pytest.mark.parametrize("name", ["golden", "genome", "odd", "none", "empty_only"])
def test_view_equals_the_reconstruction_from_the_sketch(name, k, w):
    seqs = ic.inputs()[name]
    want = ic.model("mm2gb_amd", name, k, w)
    with mm.SeedIndex(seqs, k=k, w=w, threads=2) as ix:
        got = ix.view()
        ic.same_index(got, want, f"{name} k={k} w={w}")
        assert (got["k"], got["w"], got["built_on"], got["uploads"]) == (k, w, -1, 0)
        assert ix.size() == (want["n_keys"], want["n_occ"])
    # the inputs are not trivial
    counts = np.diff(want["first"])
    if name in ("golden", "genome", "odd"):
        assert (counts > 1).any(), "no key with more than one occurrence"
        rid_lo = np.minimum.reduceat(want["where"] >> np.uint64(32), want["first"][:-1])
        rid_hi = np.maximum.reduceat(want["where"] >> np.uint64(32), want["first"][:-1])
        assert (rid_lo != rid_hi).any(), "no key with occurrences in more than one sequence"
        if k == 4:
            # the widest table a k allows.  (A k-mer and its reverse complement share a key and a k-mer equal to its own is skipped, so there are
            # at most 2^(2k-1) keys -- 120 for k = 4 -- and bits stops at 2k - 1: the `bits < 2k` limit of build_buckets can never be the one
            # that binds, for any k.  What k = 4 does reach is a prefix of all but one bit of the key, buckets of at most two keys.)
            assert want["bits"] == 2 * k - 1 and want["bucket_shift"] == 1 and want["n_keys"] > 1 << (2 * k - 2)
        else:
            assert want["bits"] < 2 * k
    else:
        assert want["n_keys"] == 0 and want["n_bucket"] == 3 and not want["bucket"].any() and want["first"].tolist() == [0]
    # the ordering premise of the device build's sort: y strictly ascending within each sequence's sketch
    for r, xy in enumerate(want["sketches"]):
        assert np.all(xy[:, 1] >> np.uint64(32) == r)
        assert np.all(np.diff(xy[:, 1].astype(np.int64)) > 0), f"{name} sequence {r}: y not strictly ascending"


def test_refusals_and_a_host_built_index():
    L = mm.lib()
    seqs = (C.c_char_p * 1)(b"ACGTTGCATGCCATGA" * 20)
    lens = np.array([320], np.int32)
    assert L.mm2gb_index_build_gpu(None, 15, 10, 1, seqs, lens.ctypes.data) is None
    assert "mm2gb_index_build_gpu" in L.mm2gb_last_error().decode()
    with mm.SeedIndex([b"ACGTTGCATGCCATGA" * 20]) as ix:
        assert L.mm2gb_index_mid_occ_gpu(None, ix._h, 2e-4, 10, 1000000) < 0
        assert "mm2gb_index_mid_occ_gpu" in L.mm2gb_last_error().decode()
        v = ix.view()
        assert v["built_on"] == -1 and v["uploads"] == 0 and v["n_keys"] > 0
        with pytest.raises(mm.Mm2gbError, match="mm2gb_index_fetch_device"):
            ix.fetch_device(0)
        assert ix.build_split() == dict(h2d=0.0, sketch=0.0, sort=0.0, tables=0.0, d2h=0.0)
        assert L.mm2gb_index_view(None, C.byref(mm.IndexView())) != 0 and "mm2gb_index_view" in L.mm2gb_last_error().decode()
        assert L.mm2gb_index_view(ix._h, None) != 0
