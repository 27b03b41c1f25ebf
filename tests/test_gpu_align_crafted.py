"""The device backend of the alignment of hits (csrc/align_kernels.hip: k_al_gather, k_al_zdrop, the second pass on resident bytes) on the crafted chains of
tests/align_crafted_cases.py: stretches across k_al_gather's 4 KiB slices on either side, strand and direction, drops on either side of mm_test_zdrop's thresholds, the
one dropping fill at list position 0, 63, 64 and last of k_al_zdrop's list, the inversion probe on either side of its score.  Device == host == the reference's recorded
answers (tests/golden/align_crafted), every record, field and word, and the counts; tests/test_align_crafted_cpu.py holds each case to the path it is built for."""
import pytest

import align_cases as ac
import align_crafted_cases as cc
import mm2gb_amd as mm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    with mm.Engine(device=0) as e:
        yield e


@pytest.fixture(scope="module")
def golden():
    return {(name, single): cc.load(name, single) for name in cc.NAMES for single in (False, True)}


@pytest.fixture(scope="module")
def host(golden):
    return {(name, single): (cc.host_single(b, 8) if single else ac.run_host(b, threads=8)) for (name, single), (b, _) in golden.items()}


def run_gpu(eng, b, single):
    return cc.gpu_single(eng, b) if single else ac.run_gpu(eng, b)


@pytest.mark.parametrize("single", [False, True], ids=["dual", "single"])
@pytest.mark.parametrize("name", cc.NAMES)
def test_device_equals_host_and_fixture(eng, golden, host, name, single):
    """A_mixed: every seam case in one call, shuffled among 30 tiny reads whose stretches are 1 .. 15 mod 16 (the arenas round a job to 16 bytes)."""
    b, want = golden[name, single]
    got, info = run_gpu(eng, b, single)
    ac.assert_same(got, want, name + ": device against the fixture")
    ac.assert_same(got, host[name, single][0], name + ": device against host")
    assert info["counts"] == host[name, single][1]["counts"]
    assert info["counts"]["rounds"] == cc.meta()["batches"][name]["counts_single" if single else "counts"]["rounds"]


@pytest.mark.parametrize("single", [False, True], ids=["dual", "single"])
def test_seam_cases_in_one_call(eng, golden, single):
    """The seam cases without the tiny reads: every job starts on a multiple of 16."""
    b, want = golden["A_mixed", single]
    one, w = cc.pick(b, want, cc.seam_reads(cc.meta()["batches"]["A_mixed"]["names"]))
    assert len(one["reads"]) == 18
    got, _ = run_gpu(eng, one, single)
    ac.assert_same(got, w, "the seam cases together")


@pytest.mark.parametrize("name", ["A_mixed", "B", "C"])
def test_every_case_alone(eng, golden, name):
    """Each case as a batch of its own: its jobs are the round's first, its slices the launch's only ones."""
    b, want = golden[name, False]
    names = cc.meta()["batches"][name]["names"]
    for i, n in enumerate(names):
        if n.startswith("tiny"):
            continue
        one, w = cc.pick(b, want, [i])
        got, info = ac.run_gpu(eng, one)
        ac.assert_same(got, w, n + ": alone")
        stored = cc.meta()["batches"][name]["alone"][n][0]
        assert {k: info["counts"][k] for k in cc.KEEP if info["counts"][k]} == stored, n


def test_arena_reuse(eng, golden):
    """The seam batch, the threshold batch, the seam batch again: identical bytes."""
    a, b = golden["A_mixed", False][0], golden["B", False][0]
    first, _ = ac.run_gpu(eng, a)
    ac.run_gpu(eng, b)
    again, _ = ac.run_gpu(eng, a)
    for x, y in zip(first, again):
        assert all(p.tobytes() == q.tobytes() for p, q in zip(x, y))
    ac.assert_same(again, golden["A_mixed", False][1], "the seam batch after another")
