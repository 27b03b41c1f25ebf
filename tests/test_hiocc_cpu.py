"""The host forms (csrc/seeding.cpp) where minimizers occur 10^3 to 10^5 times: a reference with satellite arrays and a microsatellite
(tests/hiocc_cases.py) against what the reference's mm_collect_matches and collect_seed_hits did on it, recorded into tests/golden/hiocc
(tests/tools/gen_golden_hiocc.py), and the conditions that input must meet for tests/test_gpu_hiocc.py to reach the device code it is about.
Every comparison is exact.  No GPU needed."""
import functools

import numpy as np
import pytest

import hiocc_cases as hc

mm = pytest.importorskip("mm2gb_amd")


@functools.lru_cache(maxsize=None)
def host():
    """The host index's counts and mid_occ, and every read's matches under the sets the conditions are about."""
    rd = hc.reads()
    with mm.SeedIndex(hc.genome(), threads=8) as ix:
        view = ix.view()
        mo = ix.mid_occ()
        sets = {name: [ix.matches(s, **dict(dict(mid_occ=mo), **hc.SETS[name])) for _, s in rd] for name in ("default", "everything kept") + hc.THINNING[1:]}
        sets["q filter off"] = [ix.matches(s, **dict(hc.SETS["q filter"], q_occ_frac=0.0)) for _, s in rd]
        ranks = {f: ix.mid_occ(f, 1, 1 << 30) for _, f in hc.rank_fracs(view["n_keys"])}
    return dict(first=view["first"], mid_occ=mo, sets=sets, ranks=ranks)


def test_the_simulator_has_not_drifted(tmp_path):
    ref_fa, reads_fa = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fa")
    hc.write_fastas(ref_fa, reads_fa)
    meta = hc.meta()
    assert (hc.md5_of(ref_fa), hc.md5_of(reads_fa)) == (meta["ref_md5"], meta["reads_md5"])
    assert sorted(hc.fixtures()) == list(range(11)) and [hc.fixtures()[k]["name"] for k in range(11)] == [n for n, _ in hc.reads()]


def test_index_counts_and_mid_occ():
    h = host()
    cnt = np.diff(h["first"])
    assert cnt.max() >= 65_536 and (cnt >= 256).sum() >= 30 and (cnt > 4095).sum() >= 5
    assert h["mid_occ"] == hc.mid_occ_model(h["first"], 2e-4, 10, 1_000_000) == hc.meta()["measured"]["mid_occ"]
    vals = set()
    for f, got in h["ranks"].items():
        assert got == hc.mid_occ_model(h["first"], f, 1, 1 << 30), f"frac {f}"
        vals.add(got - 1)
    assert vals >= {int(cnt.min()), int(cnt.max())} and any(v >> 16 for v in vals)


def test_mid_occ_model_on_small_indexes_and_clamps():
    rng = np.random.default_rng(4)
    seqs = [bytes(rng.choice(hc.B, 30_000)), b"ACGTTGCA" * 500]
    for k, w in ((4, 3), (6, 5), (15, 10)):
        with mm.SeedIndex(seqs, k=k, w=w) as ix:
            first = ix.view()["first"]
            for _, f in hc.rank_fracs(len(first) - 1):
                assert ix.mid_occ(f, 1, 1 << 30) == hc.mid_occ_model(first, f, 1, 1 << 30)
            for f in (0.0, -1.0, 2e-4, 0.01, 0.5, 1.0):
                for c in ((10, 1_000_000), (1, 5), (50, 60), (10, 10), (3, 2)):
                    assert ix.mid_occ(f, *c) == hc.mid_occ_model(first, f, *c), (k, f, c)
    with mm.SeedIndex([]) as ix:
        first = ix.view()["first"]                     # no keys: no quantile, INT32_MAX before the clamps
        assert ix.mid_occ(0.5, 1, 1 << 30) == hc.mid_occ_model(first, 0.5, 1, 1 << 30) == 1 << 30
        assert ix.mid_occ(0.5, 3, 2) == hc.mid_occ_model(first, 0.5, 3, 2) == hc.INT32_MAX


@functools.lru_cache(maxsize=None)
def check_inputs():
    """The conditions the GPU tests rely on, from host results only (the figures measured when the fixtures were made: meta.json)."""
    h = host()
    rd = hc.reads()
    qlens = [len(s) for _, s in rd]
    everything, default = h["sets"]["everything kept"], h["sets"]["default"]
    s = hc.streak_figures(everything, qlens, 300, 20)
    assert s["n_long"] >= 1 and s["thinned"] >= 100 and s["capped"] >= 1 and s["dropped"] >= 20 and s["n_max"] >= 65_536
    assert hc.streak_figures(everything, qlens, 10, 100)["thinned"] >= 100
    assert max(int(m["seeds"][:, 0].max()) for m in default) > 1000
    assert all((m["rep_len"] > 0) == (k != hc.C2) for k, m in enumerate(default))
    # n > max_max_occ alone drops a match that is among its streak's `keep` rarest: in the two thinning sets where that can happen.  In "mid 50"
    # the streaks are long and the matches above 4095 never among the rarest (they sit in thinned streaks all the same), "wide thinning" puts
    # max_max_occ above every count so that the selection alone decides, and the q filter removes those values before the look-up
    for name in hc.THINNING:
        kw = dict(dict(mid_occ=h["mid_occ"], max_max_occ=4095, occ_dist=500, q_occ_frac=0.01), **hc.SETS[name])
        before = [hc.without_q_filtered(mm.sketch(s), m, kw["mid_occ"], kw["q_occ_frac"]) for (_, s), m in zip(rd, everything)]
        n = hc.dropped_by_max_max_occ_alone(before, h["sets"][name], kw["mid_occ"], kw["max_max_occ"], kw["occ_dist"])
        above = sum(int((m["seeds"][:, 0] > kw["max_max_occ"]).sum()) for m in before)
        assert n >= 1 or name not in ("default", "cap of 128"), name
        assert above >= 100 or name not in ("default", "cap of 128", "mid 50"), name
    # the q filter removes a value that fills hundreds of places of one read's sorted minimizers, and the result shows it: every such value
    # occurs more than mid_occ = 5 times in the reference as well, so the thinning drops what the filter leaves and the kept seeds are the same
    # with the filter off, but a minimizer the filter took is not counted in rep_len
    qf = hc.SETS["q filter"]
    taken = [len(m["seeds"]) - len(hc.without_q_filtered(mm.sketch(s), m, qf["mid_occ"], qf["q_occ_frac"])["seeds"]) for (_, s), m in zip(rd, everything)]
    assert max(np.unique(mm.sketch(s)[:, 0], return_counts=True)[1].max() for _, s in rd) >= 256 and max(taken) >= 256
    assert any(a["rep_len"] < b["rep_len"] for a, b in zip(h["sets"]["q filter"], h["sets"]["q filter off"]))
    assert sum(len(everything[k]["hits"]) for k in (hc.C2,) + hc.UNITS37) < 5_000_000


def test_the_inputs_reach_the_code_under_test():
    check_inputs()


def test_matches_and_anchors_equal_the_references_recordings():
    """mm2gb_collect_matches at the default options against every recorded mm_collect_matches call; mm2gb_collect_seeds_host on those
    matches against the recorded anchors (their number and digest)."""
    default = host()["sets"]["default"]
    fx = hc.fixtures()
    for k, m in enumerate(default):
        hc.same_as_recorded(m, fx[k], fx[k]["name"])
    anchors = mm.collect_seeds_host(0, default, threads=4)
    for k, a in enumerate(anchors):
        assert len(a) == fx[k]["n_anchors"] and hc.sha(a) == fx[k]["a_sha256"], fx[k]["name"]
