#!/usr/bin/env python3
"""tests/golden/hiocc/* from the REFERENCE (dev container only): the reference mapper on the satellite reference and reads of
tests/hiocc_cases.py, at max-chain-skip = infinity (the GPU path's contract), observed through oracle/capture_hooks.c: what mm_collect_matches
(seed.c:98) returned for every read and the sorted anchors collect_seed_hits (map.c:295-331) made of it, and the PAF it printed.  Data only:
seeds, mini_pos and rep_len in full; of the hits and anchors (up to 5 MB a read) their number and the SHA-256 of their bytes.
    make -C oracle all && python tests/tools/gen_golden_hiocc.py"""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hiocc_cases as hc      # noqa: E402
import orc                    # noqa: E402

MAX_BYTES = 62_020            # the largest fixture of tests/golden/seeds


def figures():
    """The measured figures of the conditions tests/test_hiocc_cpu.py asserts, from the host build."""
    import mm2gb_amd as mm
    rd = hc.reads()
    with mm.SeedIndex(hc.genome(), threads=8) as ix:
        cnt = np.diff(ix.view()["first"])
        mo = ix.mid_occ()
        everything = [ix.matches(s, **hc.UNFILTERED) for _, s in rd]
        default = [ix.matches(s, mo) for _, s in rd]
        qlens = [len(s) for _, s in rd]
        return dict(n_keys=int(len(cnt)), n_occ=int(cnt.sum()), max_count=int(cnt.max()), keys_256=int((cnt >= 256).sum()),
                    keys_above_4095=int((cnt > 4095).sum()), mid_occ=mo, hits_default=int(sum(len(m["hits"]) for m in default)),
                    max_kept_n_default=int(max(m["seeds"][:, 0].max() for m in default)),
                    streaks_300_20=hc.streak_figures(everything, qlens, 300, 20), streaks_10_100=hc.streak_figures(everything, qlens, 10, 100))


if __name__ == "__main__":
    if not orc.ref_available():
        sys.exit("reference build missing: run `make -C oracle all` in a container that has the reference checkout")
    os.makedirs(hc.HIOCC, exist_ok=True)
    exe, hook = os.path.join(orc.REF_DIR, "minimap2_cpu"), os.path.join(orc.REF_DIR, "libcapture.so")
    with tempfile.TemporaryDirectory() as td:
        ref_fa, reads_fa, cap = os.path.join(td, "ref.fa"), os.path.join(td, "reads.fa"), os.path.join(td, "seeds.bin")
        hc.write_fastas(ref_fa, reads_fa)
        t0 = time.time()
        r = subprocess.run([exe, "-t", "1", "--max-chain-skip=2147483647", ref_fa, reads_fa], env=dict(os.environ, LD_PRELOAD=hook, MM2GB_CAPTURE_SEEDS=cap),
                           check=True, capture_output=True)
        print(f"reference run {time.time() - t0:.0f} s, {r.stdout.count(10)} PAF lines, {len(r.stdout)} bytes")
        recs = orc.read_seed_capture(cap)
        md5 = dict(ref_md5=hc.md5_of(ref_fa), reads_md5=hc.md5_of(reads_fa))
    open(os.path.join(hc.HIOCC, "sat_inf.paf"), "wb").write(r.stdout)
    rd = hc.reads()
    assert len(recs) == len(rd) and all(x["qlen"] == len(s) for x, (_, s) in zip(recs, rd))       # one record per read, in file order
    for k, x in enumerate(recs):
        m = dict(read=k, name=rd[k][0], qlen=int(x["qlen"]), rep_len=int(x["rep_len"]), n_hits=int(len(x["hits"])), hits_sha256=hc.sha(x["hits"]),
                 n_anchors=int(len(x["a"])), a_sha256=hc.sha(x["a"]), source="tests/hiocc_cases.py --max-chain-skip=2147483647")
        path = os.path.join(hc.HIOCC, f"sat_{k}.npz")
        np.savez_compressed(path, seeds=x["seeds"], mini_pos=x["mini_pos"], meta=np.frombuffer(json.dumps(m).encode(), dtype=np.uint8))
        assert os.path.getsize(path) < MAX_BYTES, (path, os.path.getsize(path))
        print(f"sat_{k}: {rd[k][0]} {len(x['seeds'])} seeds, {m['n_hits']} hits, {m['n_anchors']} anchors, rep_len {m['rep_len']}, {os.path.getsize(path)} bytes")
    json.dump(dict(md5, measured=figures()), open(os.path.join(hc.HIOCC, "meta.json"), "w"), indent=1)
