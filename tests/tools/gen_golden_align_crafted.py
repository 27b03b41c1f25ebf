"""Records tests/golden/align_crafted: for every batch of align_crafted_cases.all_batches() the call's input (records and anchors made by the case builder) and what the
reference's mm_align_skeleton answers when it is fed exactly these, under the batch's dual-affine options (<name>.npz, align_cases.save_batch's layout) and under
q2 = q, e2 = e (single.npz: the same layout with the inputs left out, every file's reads end to end).  Needs oracle/_ref/libminimap2ref.so.  While recording it asserts that
this project's host form equals the reference on every batch; the counts in meta.json are the host form's, for the batch and for every case run alone, and they describe the
reference's run only because every record and word agrees.  tests/test_align_crafted_cpu.py holds them against what each case is built for.

    python tests/tools/gen_golden_align_crafted.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import align_cases as ac  # noqa: E402
import align_crafted_cases as cc  # noqa: E402

KEEP = cc.KEEP


def both_ways(name, b):
    """The reference's answers under the batch's options and under q2 = q, e2 = e, each held against the host form; and the host form's counts."""
    want = cc.ref_run(b)
    got, info = ac.run_host(b, threads=4)
    ac.assert_same(got, want, f"{name}: host form against the reference")
    want1 = cc.ref_run(cc.as_single(b))
    got1, info1 = cc.host_single(b)
    ac.assert_same(got1, want1, f"{name}: host form against the reference, single-affine")
    return want, want1, dict(counts={k: info["counts"][k] for k in KEEP}, counts_single={k: info1["counts"][k] for k in KEEP})


SINGLE = {}


def save(name, b, want, want1):
    ac.save_batch(os.path.join(cc.GOLD, name + ".npz"), b, want)
    SINGLE[name] = want1


def main():
    assert ac.ref_available(), "build oracle/_ref first (make -C oracle ref)"
    os.makedirs(cc.GOLD, exist_ok=True)
    meta = dict(batches={})
    kept = {}
    for name, (b, names) in cc.all_batches().items():
        want, want1, m = both_ways(name, b)
        save(name, b, want, want1)
        kept[name] = (b, want, want1)
        nz = lambda c: {k: c[k] for k in KEEP if c[k]}
        m["alone"] = {}
        for i, n in enumerate(names if name != "B_list" else []):
            two, one = (nz(cc.counts_alone(b, i, single=s)[1]["counts"]) for s in (False, True))
            m["alone"][n] = [two, None if one == two else one]          # (single-affine: only where it differs)
        meta["batches"][name] = dict(m, names=names)
        print(name, {k: v for k, v in m["counts"].items() if v})
    # the list batches with a drop: the whole batch through the reference, stored as the one read that differs from B_list
    base, base_want, base_want1 = kept["B_list"]
    for place in cc.LIST_PLACES:
        name, r = "B_" + place, cc.list_read(place)
        b, names = cc.list_batch(place)
        want, want1, m = both_ways(name, b)
        for i in range(len(names)):
            same = b["refs"][i] == base["refs"][i] and b["reads"][i] == base["reads"][i]
            assert same == (i != r), f"{name}: read {i}"
        one, w = cc.pick(b, want, [r])
        _, w1 = cc.pick(b, want1, [r])
        save(name, one, w, w1)
        assert m["counts"]["fill_two_pass"] == 1 and m["counts_single"]["fill_two_pass"] == 1
        meta["batches"][name] = dict(m, names=names, alone={})
        print(name, {k: v for k, v in m["counts"].items() if v})
    json.dump(meta, open(os.path.join(cc.GOLD, "meta.json"), "w"), sort_keys=True, separators=(",", ":"))
    ac.save_batch(os.path.join(cc.GOLD, "single.npz"), dict(cc.as_single(kept["A_mixed"][0]), refs=[], reads=[], regs=[], anchors=[]), [w for n in cc.NAMES for w in SINGLE[n]])
    for name in cc.NAMES:                 # what the tests load is what was recorded
        for single in (False, True):
            b, want = cc.load(name, single)
            got, _ = cc.host_single(b) if single else ac.run_host(b)
            ac.assert_same(got, want, name + ": read back")
    print("bytes:", sum(os.path.getsize(os.path.join(cc.GOLD, f)) for f in os.listdir(cc.GOLD)))


if __name__ == "__main__":
    main()
