"""The HiFi and assembly presets (map-hifi / map-ccs, asm5, asm10, asm20) without a GPU: the option sets against the reference's mm_set_opt, the
host DP at the presets' scores, mm_align_skeleton with their options, and mg_lchain_rmq on a contig's raw anchors (bw = 1000, max_gap = 10000).
The committed fixtures everywhere (tests/tools/gen_golden_asm.py), the compiled reference where oracle/_ref is built.  Every comparison is exact."""
import numpy as np
import pytest

import align_cases as ac
import asm_cases as am
import ksw_cases as kc
import mm2gb_amd as mm
import orc

needs_ref = pytest.mark.skipif(not ac.ref_available(), reason="the reference build (oracle/_ref) is not here")


@pytest.mark.parametrize("name", am.NAMES)
def test_options_equal_the_recorded_ones(name):
    got, want = am.own_options(name), am.golden_options()[name]
    for group in ("align", "map", "index"):
        assert got[group] == want[group], (name, group, {k: (got[group][k], v) for k, v in want[group].items() if got[group][k] != v})
    if name in am.ASM:
        assert mm.map_opt_preset(name).flag == mm.F_RMQ == 0x80000000
    assert mm.map_opt_preset(name).max_chain_skip == mm.map_opt().max_chain_skip


@needs_ref
@pytest.mark.parametrize("name", am.NAMES)
def test_options_equal_mm_set_opt(name):
    assert am.own_options(name) == am.ref_options(name)


def test_ccs_is_hifi_and_the_old_names_stay():
    assert am.own_options("map-ccs") == am.own_options("map-hifi")
    for name in ("map-ont", "map-pb"):
        a, b = mm.map_opt_preset(name), mm.map_opt()
        assert bytes(a) == bytes(b)
    assert mm.map_opt_preset("asm10", max_chain_skip=25).max_chain_skip == 25


def test_refusals():
    for name in ("sr", "ava-pb", "ava-ont", "splice", "asm", "asm15", ""):
        with pytest.raises(mm.Mm2gbError, match="not supported"):
            mm.map_opt_preset(name)
    with pytest.raises(mm.Mm2gbError, match="sr"):
        mm.align_opt("sr")
    with pytest.raises(mm.Mm2gbError):
        mm.preset("ava-pb")
    with pytest.raises(mm.Mm2gbError, match="no field"):
        mm.map_opt_preset("asm5", no_such_field=1)


def test_host_dp_equals_the_fixtures():
    """200 recorded jobs per preset tuple; asm5's q + e + q2 + e2 = 124 is three below the limit of the 8-bit sums."""
    sets = am.golden_ksw()
    assert len(sets) == len(am.PRESETS) and all(len(s[1]) == 200 for s in sets)
    assert [(p.q, p.e, p.q2, p.e2) for p, *_ in sets] == [(6, 2, 26, 1), (39, 3, 81, 1), (16, 2, 41, 1), (6, 2, 26, 1)]
    for k, (p, jobs, q, t, want) in enumerate(sets):
        kc.assert_same(mm.ksw_extd2_host_batch(p, jobs, q, t, threads=2), want, f"fixture set {am.PRESETS[k]}", jobs)


@needs_ref
def test_host_dp_equals_the_reference_fuzz():
    """2 000 seeded jobs per tuple over ksw_cases' lengths, widths, flags, zdrops and end bonuses."""
    rng = np.random.default_rng(5)
    for k, p in enumerate(am.ksw_params()):
        jobs, q, t = kc.make_batch(rng, p.m, 2000, kc.LENS_CPU, p_empty=0.02)
        kc.assert_same(mm.ksw_extd2_host_batch(p, jobs, q, t, threads=4), kc.ref_batch(p, jobs, q, t), f"tuple of {am.PRESETS[k]}", jobs)


@pytest.mark.parametrize("preset", am.PRESETS)
def test_align_host_equals_the_recorded_vectors(preset):
    b, want = am.load_align(preset)
    o = mm.align_opt(preset)
    assert all(getattr(o, k) == getattr(b["opt"], k) for k, _ in mm.AlignOpt._fields_)
    b["opt"] = o
    ac.assert_same(ac.run_host(b)[0], want, preset)
    assert sum(len(w[0]) for w in want) > 0


def test_align_host_squeezes_a_contigs_anchors():
    """The plain contig with every anchor the chaining kept, those no record holds included: mm_squeeze_a inside the call moves them."""
    b, want = am.load_align("unsqueezed_asm10")
    assert sum(len(a) for a in b["anchors"]) > 4 * sum(int(r["cnt"].sum()) for r in b["regs"])
    b["opt"] = mm.align_opt("asm10")
    ac.assert_same(ac.run_host(b)[0], want, "unsqueezed")


@needs_ref
@pytest.mark.parametrize("preset", am.PRESETS)
def test_align_host_equals_the_reference_on_fresh_contigs(preset):
    refs, reads = am.fresh_contigs(61 + am.PRESETS.index(preset), n=40)
    b, want, _ = am.ref_batch(refs, reads, preset)
    b["opt"] = mm.align_opt(preset)
    ac.assert_same(ac.run_host(b)[0], want, preset)
    assert sum(len(w[0]) for w in want) >= 20


@pytest.fixture(scope="module")
def raw_anchors():
    refs, contigs = am.load_sim()
    return {tag: am.own_anchors([s for _, s in refs], [s for _, s in contigs[tag]], "asm10") for tag in ("d3", "d8")}


@needs_ref
@pytest.mark.skipif(not orc.ref_available(), reason="needs oracle/_ref/libmm2ref.so")
@pytest.mark.parametrize("skip", list(am.SKIPS))
def test_rmq_host_equals_the_reference_on_raw_anchors(raw_anchors, skip):
    """mg_lchain_rmq as map.c:691 calls it: a contig's raw sorted anchors, bw = 1000, max_gap = 10000."""
    prm = am.rmq_param_first(am.SKIPS[skip])
    for tag, anchors in raw_anchors.items():
        assert min(len(a) for a in anchors) > 1000
        got, _ = mm.rmq_chain_host(np.concatenate(anchors), am.offsets_of(anchors), am.to_lib(prm), threads=4)
        for r, a in enumerate(anchors):
            ref = orc.ref_lchain_rmq(a, prm)
            assert np.array_equal(got[r][0], ref["u"]) and np.array_equal(got[r][1], ref["a_out"]), (tag, skip, r)
            assert len(ref["u"]) > 0
