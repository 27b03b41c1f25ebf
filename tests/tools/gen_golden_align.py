"""Records tests/golden/align: for every batch of align_cases.fixture_batches() the call's input (the records and anchors as map.c has them when it
calls align_regs, made by the reference's own chaining on this project's anchors) and the reference's mm_align_skeleton's answers.  Needs
oracle/_ref/libminimap2ref.so.  While recording it asserts that this project's host form equals the reference on every batch -- the path counts
are the host form's, and they describe the reference's run only because every record and word agrees -- and that the answers contain at least
one of each path of align_cases.MUST_HAVE; the counts go to meta.json, where the tests check them.

    python tests/tools/gen_golden_align.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import align_cases as ac  # noqa: E402


def main():
    assert ac.ref_available(), "build oracle/_ref first (make -C oracle ref)"
    os.makedirs(ac.GOLD, exist_ok=True)
    meta = dict(batches={}, total={})
    for name, (refs, reads, preset, kw) in ac.fixture_batches().items():
        b, want = ac.ref_batch(refs, reads, preset, **kw)
        got, info = ac.run_host(b, threads=4)
        ac.assert_same(got, want, f"{name}: host form against the reference")
        counts = dict(info["counts"], n_ambi=sum(int(w[1]["n_ambi"].sum()) for w in want), reads=len(reads), records=sum(len(w[0]) for w in want))
        ac.save_batch(os.path.join(ac.GOLD, name + ".npz"), b, want)
        meta["batches"][name] = dict(preset=preset, options=kw, counts=counts)
        for k, v in counts.items():
            meta["total"][k] = max(meta["total"].get(k, 0), v) if k == "rounds" else meta["total"].get(k, 0) + v
        print(name, {k: v for k, v in counts.items() if v})
    missing = [k for k in ac.MUST_HAVE if not meta["total"].get(k)]
    assert not missing, f"the reference's answers contain none of: {missing}"
    assert any(c["counts"]["rounds"] >= 3 for c in meta["batches"].values())
    json.dump(meta, open(os.path.join(ac.GOLD, "meta.json"), "w"), indent=1, sort_keys=True)
    print("bytes:", sum(os.path.getsize(os.path.join(ac.GOLD, f)) for f in os.listdir(ac.GOLD)))


if __name__ == "__main__":
    main()
