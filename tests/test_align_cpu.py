"""The alignment of hits on host threads (mm2gb_align_regs_host, csrc/align_host.cpp) against the reference's mm_align_skeleton: the committed
fixtures (tests/golden/align), a fresh random batch per preset where oracle/_ref is built, the refusals and the edges.  Every comparison is
exact: the number and order of the records, every field, every CIGAR word."""
import copy

import numpy as np
import pytest

import align_cases as ac
import mm2gb_amd as mm


@pytest.fixture(scope="module")
def golden():
    return {name: ac.load_batch(name) for name in ac.golden_names()}


def test_fixtures_reach_every_path():
    """The stored counts: the reference's answers on the fixture batches contain at least one of each path, and one batch needs three rounds."""
    meta = ac.golden_meta()
    missing = [k for k in ac.MUST_HAVE if not meta["total"].get(k)]
    assert not missing, missing
    assert meta["total"]["rounds"] >= 3 and meta["total"]["reads_3_rounds"] >= 1
    assert set(meta["batches"]) == set(ac.golden_names())


@pytest.mark.parametrize("name", ["ont", "pb", "small_mat", "end_bonus", "inv_pair"])
def test_host_equals_fixtures(golden, name):
    b, want = golden[name]
    got, info = ac.run_host(b, threads=4)
    ac.assert_same(got, want, name)
    stored = ac.golden_meta()["batches"][name]["counts"]
    assert {k: v for k, v in info["counts"].items()} == {k: stored[k] for k in info["counts"]}, "the paths taken differ from those recorded"


@pytest.mark.skipif(not ac.ref_available(), reason="the reference is not built here")
@pytest.mark.parametrize("preset", ["map-ont", "map-pb"])
def test_host_equals_live_reference(preset):
    """About 300 fresh reads per preset, a tenth of them with unrelated sequence or an inverted block in the middle."""
    refs, reads = ac.random_batch(31 if preset == "map-ont" else 32, preset, n_reads=300)
    b, want = ac.ref_batch(refs, reads, preset)
    got, info = ac.run_host(b, threads=8)
    ac.assert_same(got, want, preset)
    assert info["counts"]["split"] > 0 and info["counts"]["fill_two_pass"] > 0 and sum(len(w[0]) for w in want) >= 250


def test_defaults_are_the_presets(golden):
    """mm2gb_align_opt_init against the options the reference's mm_set_opt left in the fixtures."""
    for name, preset in (("ont", "map-ont"), ("pb", "map-pb")):
        o, w = mm.align_opt(preset), golden[name][0]["opt"]
        assert all(getattr(o, k) == getattr(w, k) for k, _ in mm.AlignOpt._fields_)
    with pytest.raises(mm.Mm2gbError, match="sr"):
        mm.align_opt("sr")


def test_threads_give_identical_bytes(golden):
    b, _ = golden["ont"]
    one, _ = ac.run_host(b, threads=1)
    eight, _ = ac.run_host(b, threads=8)
    for (r1, a1, w1), (r8, a8, w8) in zip(one, eight):
        assert r1.tobytes() == r8.tobytes() and a1.tobytes() == a8.tobytes() and w1.tobytes() == w8.tobytes()


def test_batch_schedule_gives_identical_bytes(golden, monkeypatch):
    """MM2GB_ALIGN_ROUNDS=batch: the device form's schedule (all reads in one sequence of rounds, planning and stitching on several threads) with the
    host DP behind it, against the fixtures."""
    monkeypatch.setenv("MM2GB_ALIGN_ROUNDS", "batch")
    for name in ("ont", "pb", "inv_pair"):
        b, want = golden[name]
        got, info = ac.run_host(b, threads=8)
        ac.assert_same(got, want, name + ": batch schedule")
        assert info["counts"]["rounds"] == ac.golden_meta()["batches"][name]["counts"]["rounds"]


def test_refusals(golden):
    b, _ = golden["inv_pair"]
    for text, bad in ac.refusals(b):
        with pytest.raises(mm.Mm2gbError, match=text):
            ac.run_host(bad)


def test_refused_call_leaves_the_output_zeroed(golden):
    import ctypes as C
    b, _ = golden["inv_pair"]
    o = copy.copy(b["opt"]); o.flag |= mm.F_SR
    out = mm._AlignOut()
    C.memset(C.byref(out), 0xff, C.sizeof(out))
    fn = mm.lib().mm2gb_align_regs_host
    fn.argtypes = None
    rc = fn(C.byref(o), C.c_int(15), C.c_int(0), C.c_int32(0), None, None, C.c_int64(0), None, None, None, None, None, None, C.c_int(1), C.byref(out))
    assert rc != 0 and bytes(out) == bytes(C.sizeof(out))


def test_edges(golden):
    b, want = golden["inv_pair"]
    o = b["opt"]
    got, _ = mm.align_regs_host(o, b["k"], b["hpc"], b["refs"], [], [], [])                               # an empty batch
    assert got == []
    got, _ = mm.align_regs_host(o, b["k"], b["hpc"], b["refs"], b["reads"][:1], [np.zeros(0, mm.REG_DTYPE)], [np.zeros((0, 2), np.uint64)])
    assert len(got) == 1 and len(got[0][0]) == 0 and len(got[0][2]) == 0                                    # a read without records
    # a record with cnt == 0 beside the read's own: mm_align1 leaves it alone, mm_hit_sort drops it
    regs = np.concatenate([b["regs"][0], np.zeros(1, mm.REG_DTYPE)])
    regs[-1]["as_"] = len(b["anchors"][0]); regs[-1]["id"] = len(regs) - 1; regs[-1]["parent"] = len(regs) - 1
    got, _ = mm.align_regs_host(o, b["k"], b["hpc"], b["refs"], b["reads"][:1], [regs], [b["anchors"][0]])
    ac.assert_same(got, want[:1], "cnt == 0")
    assert mm.cigar_string(np.array([5 << 4, 3 << 4 | 1, 7 << 4 | 2], np.uint32)) == "5M3I7D"
