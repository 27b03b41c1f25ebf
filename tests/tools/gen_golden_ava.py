#!/usr/bin/env python3
"""Makes tests/golden/ava/ava.npz (one JSON document, compressed): the read sets of tests/ava_cases.py (sim_sets), what oracle/_ref/minimap2_cpu -t 1 prints for every run of ava_cases.RUNS
(-x ava-ont, -x ava-pb, -x map-ont -X) at --max-chain-skip 25 and 2147483647, and the option sets mm_set_opt gives for the two presets.  Inputs and PAF text
only.  Needs the reference built under oracle/_ref (make -C oracle ref, where the reference checkout exists).

The generator asserts what makes the fixture worth having: set a has at least 100 lines, a line of a read on itself, at least 10 lines on the reverse
strand and a read without a line; set c has a pair kept only because the lengths differ, and its other name traps show in the lines."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import align_cases as ac  # noqa: E402
import ava_cases as av  # noqa: E402
import orc  # noqa: E402

LIMIT = 1024 * 1024


def write_fasta(path, recs):
    with open(path, "wb") as fh:
        for name, s in recs:
            fh.write(b">" + name.encode() + b"\n" + s + b"\n")


def paf(tgt, qry, args, skip):
    exe = os.path.join(orc.REF_DIR, "minimap2_cpu")
    return subprocess.run([exe, "-t", "1"] + args + [f"--max-chain-skip={skip}", tgt, qry], check=True, capture_output=True).stdout.decode()


def check(sets, pafs):
    rows = lambda key: [ln.split("\t") for ln in pafs[key].splitlines()]
    for skip in av.SKIPS:
        a = rows(f"a.ava-ont.{skip}")
        assert len(a) >= 100, f"set a: {len(a)} lines"
        assert any(f[0] == f[5] for f in a), "set a: no line of a read on itself"
        assert sum(f[4] == "-" for f in a) >= 10, "set a: fewer than 10 lines on the reverse strand"
        assert {n for n, _ in sets["a"]} - {f[0] for f in a}, "set a: every read has a line"
        assert all(f[11] == "0" and "tp:A:S" in f for f in a), "MM_F_ALL_CHAINS: mapping quality 0, tp:A:S"
        assert rows(f"b.ava-pb.{skip}") and rows(f"a.X.{skip}")
        for kind in ("ava-ont", "X"):
            c = rows(f"c.{kind}.{skip}")
            # dup x the longer dup: same name, the anchors on the diagonal, kept only because the lengths differ
            assert any(f[0] == f[5] == "dup" and f[1] != f[6] and f[2] == f[7] and f[4] == "+" for f in c), "set c: no pair kept by length inequality"
            pairs = {(f[0], f[5]) for f in c}
            assert not any(q > t for q, t in ((q.encode(), t.encode()) for q, t in pairs)), "set c: a pair with the larger name as query"
            assert ("read10", "read9") not in pairs and any(q == "r1" and t == "r10" for q, t in pairs), "set c: prefix order"
            assert any(q != "ré" and t == "ré" for q, t in pairs), "set c: no ASCII name against the name with a byte >= 0x80 (bytes compare as unsigned)"


def main():
    assert ac.ref_available() and os.path.exists(os.path.join(orc.REF_DIR, "minimap2_cpu")), "build oracle/_ref first (make -C oracle ref)"
    sets = av.sim_sets()
    pafs = {}
    with tempfile.TemporaryDirectory() as d:
        for name, recs in sets.items():
            write_fasta(os.path.join(d, name + ".fa"), recs)
        for run, (qry, tgt, args) in av.RUNS.items():
            for tag, skip in av.SKIPS.items():
                pafs[f"{run}.{tag}"] = paf(os.path.join(d, tgt + ".fa"), os.path.join(d, qry + ".fa"), args, skip)
    check(sets, pafs)
    os.makedirs(av.GOLD, exist_ok=True)
    out = dict(seed=av.SIM_SEED, sets={k: [[n, s.decode()] for n, s in v] for k, v in sets.items()}, paf=pafs, options={n: av.ref_options(n) for n in ("ava-ont", "ava-pb")})
    path = os.path.join(av.GOLD, "ava.npz")
    np.savez_compressed(path, doc=np.frombuffer(json.dumps(out, sort_keys=True, ensure_ascii=False).encode("utf-8"), dtype=np.uint8))
    assert os.path.getsize(path) < LIMIT, f"{path} is {os.path.getsize(path)} bytes"
    for k in sorted(pafs):
        print(f"{k}: {len(pafs[k].splitlines())} lines")
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
