"""The alignment of hits with the DP and its sequences on the device (mm2gb_align_regs_gpu, csrc/align_kernels.hip) against the host form and the
committed fixtures (tests/golden/align): every record, field and CIGAR word.  Reads fixtures only; the chains crafted for k_al_gather's slice cuts,
the drop walk's thresholds and positions and k_al_zdrop's list are tests/test_gpu_align_crafted.py's."""
import numpy as np
import pytest

import align_cases as ac
import mm2gb_amd as mm
import sim_reads

pytestmark = pytest.mark.gpu
NAMES = ["ont", "pb", "small_mat", "end_bonus", "inv_pair"]


@pytest.fixture(scope="module")
def eng():
    with mm.Engine(device=0) as e:
        yield e


@pytest.fixture(scope="module")
def golden():
    return {name: ac.load_batch(name) for name in NAMES}


@pytest.fixture(scope="module")
def host(golden):
    return {name: ac.run_host(golden[name][0], threads=8) for name in NAMES}


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_host_and_fixtures(eng, golden, host, name):
    b, want = golden[name]
    got, info = ac.run_gpu(eng, b)
    ac.assert_same(got, want, name + ": device against the fixtures")
    ac.assert_same(got, host[name][0], name + ": device against host")
    assert info["counts"] == host[name][1]["counts"]
    assert info["counts"]["rounds"] == ac.golden_meta()["batches"][name]["counts"]["rounds"]


def test_all_batches_in_one_call_shuffled(eng, golden, host):
    """The batches that share options and references, concatenated, read order shuffled: the same answers per read."""
    for names in (["ont", "inv_pair"], ["pb"]):
        b0 = golden[names[0]][0]
        refs, reads, regs, anchors, want = list(b0["refs"]), [], [], [], []
        for n in names:
            b, w = golden[n]
            shift = 0 if n == names[0] else len(refs)
            if shift:
                refs += b["refs"]
            for r in range(len(b["reads"])):
                a = b["anchors"][r].copy()
                a[:, 0] += np.uint64(shift << 32)
                wr = w[r][0].copy(); wr["rid"] += shift
                reads.append(b["reads"][r]); regs.append(b["regs"][r].copy()); anchors.append(a); want.append((wr, w[r][1], w[r][2]))
                regs[-1]["rid"] += shift
        order = np.random.default_rng(3).permutation(len(reads))
        got, _ = eng.align_regs(b0["opt"], b0["k"], b0["hpc"], refs, [reads[i] for i in order], [regs[i] for i in order], [anchors[i] for i in order])
        ac.assert_same(got, [want[i] for i in order], "+".join(names) + " shuffled")


def test_arena_reuse(eng, golden):
    """A small batch, a larger one, the small one again: identical bytes."""
    small, large = golden["inv_pair"][0], golden["ont"][0]
    first, _ = ac.run_gpu(eng, small)
    ac.run_gpu(eng, large)
    again, _ = ac.run_gpu(eng, small)
    for x, y in zip(first, again):
        assert all(p.tobytes() == q.tobytes() for p, q in zip(x, y))


def test_one_read_and_none(eng, golden):
    b, want = golden["ont"]
    got, _ = eng.align_regs(b["opt"], b["k"], b["hpc"], b["refs"], b["reads"][:1], b["regs"][:1], b["anchors"][:1])
    ac.assert_same(got, want[:1], "one read")
    got, _ = eng.align_regs(b["opt"], b["k"], b["hpc"], b["refs"], [], [], [])
    assert got == []


def test_refusals(eng, golden):
    b, _ = golden["inv_pair"]
    for text, bad in ac.refusals(b):
        with pytest.raises(mm.Mm2gbError, match=text):
            ac.run_gpu(eng, bad)


def test_three_round_read_alone(eng, golden, host):
    b, want = golden["inv_pair"]
    r = next(i for i in range(len(b["reads"])) if (want[i][0]["flags"] >> 11 & 1).any())          # the read with an inversion record
    got, info = eng.align_regs(b["opt"], b["k"], b["hpc"], b["refs"], b["reads"][r:r + 1], b["regs"][r:r + 1], b["anchors"][r:r + 1])
    ac.assert_same(got, want[r:r + 1], "three rounds")
    assert info["counts"]["rounds"] == 3 and info["counts"]["inv"] == 1


def test_long_fill_leaves_the_narrow_band_classes(eng):
    """One 30 kb read against a 40 kb reference with 6 kb of the reference missing from the read: the fill across it is bw_long wide, beyond the
    one-wave and four-wave classes of the DP.  The chain is made here (one anchor every 500 bases, on two diagonals): no chaining is under test."""
    rng = np.random.default_rng(8)
    ref = sim_reads.BASES[rng.integers(0, 4, 40_000)]
    read = np.concatenate([ref[2000:17_000], ref[23_000:38_000]])
    pos = [p for p in range(100, 30_000, 500) if not 14_900 < p < 15_100]
    a = np.array([[(p + 2000 if p < 15_000 else p + 8000), 15 << 32 | p] for p in pos], np.uint64)
    regs = np.zeros(1, mm.REG_DTYPE)
    regs[0] = (0, len(a), 0, 15 * len(a), pos[0] - 14, pos[-1] + 1, int(a[0, 0]) - 14, int(a[-1, 0]) + 1, 0, 0, 0, 15 * len(a), 30_000, 0, 15 * len(a), 0, 7, -1.0)
    o = mm.align_opt("map-ont")
    args = (o, 15, False, [ref.tobytes()], [read.tobytes()], [regs], [a])
    want, info = mm.align_regs_host(*args, threads=1)
    got, _ = eng.align_regs(*args)
    ac.assert_same(got, want, "30 kb read")
    assert len(want[0][0]) == 1 and any(int(w) >> 4 >= 5000 and int(w) & 0xf == 2 for w in want[0][2]), "the deletion was not crossed in one record"
    assert eng.ksw_info()["band"][1] < 6000
