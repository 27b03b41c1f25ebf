"""What tests/test_gpu_score_builds.py rests on and can be checked without a GPU: the generators older tests draw their batches from
have not moved, the new inputs are decisive on the oracle (they tell the cDNA penalty, the X-drop and the dd == bw edge apart), the
class cycle of fuzz_case_general, and the C ABI's accessor."""
import hashlib

import numpy as np
import pytest

import golden_io
import orc
import synth_cases as sc

mm = pytest.importorskip("mm2gb_amd")


def links(a, p):
    """(dr, dq) of every accepted link i <- p[i] of one read."""
    i = np.flatnonzero(p >= 0)
    j = p[i]
    pos = lambda col, k: (a[k, col] & np.uint64(0xffffffff)).astype(np.int64)
    return pos(0, i) - pos(0, j), pos(1, i) - pos(1, j)


def test_older_generators_return_what_they_did():
    """Existing tests' batches must not move: a hash over fuzz_case's first 12 batches (arrays, offsets, parameters) for a fixed seed and
    over one array of every older generator, recorded before the new generators were added."""
    h = hashlib.sha256()
    rng = np.random.default_rng(20240607)
    for _ in range(12):
        a, off, kw = sc.fuzz_case(rng)
        h.update(a.tobytes()); h.update(off.tobytes()); h.update(repr(sorted((k, float(v)) for k, v in kw.items())).encode())
    for a in (sc.noise(300, 1), sc.colinear(300, 2), sc.repeat_block(300, 3), sc.read_like(5000, 4), sc.rescue_case(300, 5, 20), sc.grid_ties(),
              sc.two_segments(100, 6), sc.variable_span(100, 7), sc.multi_read_batch(3, 8)[0]):
        h.update(a.tobytes())
    assert h.hexdigest() == "bcf92c7ee0ec42cc9bc63f9d22ce3acce38319a1b5d49be177394ca2df914269"


def test_the_abi_has_the_accessor():
    L = mm.lib()
    assert hasattr(L, "mm2gb_engine_last_score_mode") and "mm2gb_engine_last_score_mode" in mm.CORE_SYMBOLS
    assert L.mm2gb_engine_last_score_mode(None) == -1          # no engine: an error, not a crash
    assert hasattr(mm.Engine, "last_score_mode")


def test_new_vectors_are_there():
    names = golden_io.case_ids(golden_io.all_cases())
    for n in ("synth_spliced", "synth_spliced_iter200", "synth_qins", "synth_jump_bw5118", "synth_jump_bw5119", "synth_three_seg"):
        assert n in names


def test_spliced_read_chains_across_introns_beyond_any_table():
    a = sc.spliced(60, 5, noise_n=3000)
    o = orc.lchain_dp(a, orc.default_param(**sc.SPLICE_KW))
    assert int((o["u"] & np.uint64(0xffffffff)).max()) > 1500           # one chain through (nearly) every exon
    dr, dq = links(a, o["p"])
    assert np.count_nonzero(dr - dq > 5118) > 1000 and np.count_nonzero(dq > dr) > 100      # both branches of the cDNA penalty, far beyond a table
    assert dq.max() <= 2000                                               # max_dist_y stayed 2 000 (lchain.c:161 does not apply to cDNA)


def test_qins_chains_differ_with_and_without_the_x_drop():
    a = sc.qins_chain(150, 7)
    kw = dict(bw=100, pen_gap=np.float32(1.0), min_cnt=2, min_sc=15)
    o = orc.lchain_dp(a, orc.default_param(is_cdna=1, **kw))
    u_off, _ = orc.backtrack_compact(a, o["f"], o["p"], orc.default_param(is_cdna=1, **kw))
    u_on, _ = orc.backtrack_compact(a, o["f"], o["p"], orc.default_param(is_cdna=0, **kw))
    assert np.array_equal(u_off, o["u"]) and len(u_on) != len(u_off)


@pytest.mark.parametrize("bw", [5117, 5118, 5119, 5120])
def test_jump_chain_links_up_to_bw_exactly(bw):
    a = sc.jump_chain([5116, 5117, 5118, 5119, 5120, 5121], 9)
    _, p, _ = orc.chain_fill(a, orc.default_param(bw=bw, max_dist_x=8000, max_dist_y=8000))
    dr, dq = links(a, p)
    dd = np.abs(dr - dq)
    assert dd.max() == bw and sorted(set(dd[dd > 100].tolist())) == list(range(5116, bw + 1))


def test_fuzz_case_general_cycles_its_classes():
    rng = np.random.default_rng(3)
    for it in range(70):
        a, off, kw = sc.fuzz_case_general(rng, it)
        cls = sc.GENERAL_CLASSES[it % 7]
        seg = bool(len(a)) and bool(np.any(a[:, 1] & sc.SEG_MASK))
        single = kw["is_cdna"] == 0 and kw["n_seg"] == 1
        table = kw["bw"] + 2 <= 5120 and kw["pen_skip"] == 0
        assert off[-1] == len(a) and np.all(np.diff(off) >= 0)
        for r in range(len(off) - 1):
            x = a[off[r]:off[r + 1], 0]
            assert np.all(x[1:] >= x[:-1])                                 # sorted by x, the caller's contract
        if cls == "a":
            assert all(kw[k] == v for k, v in sc.SPLICE_KW.items())
        elif cls == "b":
            assert kw["is_cdna"] == 1 and kw["n_seg"] == 1 and kw["bw"] in (0, 100, 500)
        elif cls == "c":
            assert kw["n_seg"] in (2, 3) and kw["is_cdna"] == 0
        elif cls == "d":
            assert kw["n_seg"] in (2, 3) and kw["is_cdna"] == 1
        elif cls == "e":
            assert single and table and seg
        elif cls == "f":
            assert single and kw["bw"] in (5119, 9000, 200_000) and kw["pen_skip"] == 0 and not seg
        else:
            assert single and kw["pen_skip"] > 0 and not seg
