#!/usr/bin/env python3
"""Makes tests/golden/resident/resident.npz (one JSON document, compressed): the chimeric read set of tests/resident_cases.py (sim_chim) with its genome, and what
oracle/_ref/minimap2_cpu -t 1 prints for -x map-ont --no-long-join and -x map-pb --no-long-join on that set and on the 160 reads of tests/golden/sim160.json, and for
-x map-ont -r 500,500 on the chimeric set, each at --max-chain-skip 25 and 2147483647.  Inputs and PAF text only (of sim160 the PAFs alone: the set is regenerated
from its seed).  Needs the reference built under oracle/_ref (make -C oracle ref, where the reference checkout exists); it is run as a plain child process.

The generator asserts what makes the fixture worth having.  Every run of the chimeric set is made a second time with -P (all chains; that text is not stored): at
least 10 reads keep a record whose place among the kept records differs from its place among all chains, with another dv:f: at the two places (records are
identified by the first nine PAF columns) -- the count goes into the document.  Every sim160 PAF has at least 10 tp:A:S lines.  A read of each set has no line."""
import io
import json
import os
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import orc  # noqa: E402
import resident_cases as rc  # noqa: E402

LIMIT = 1024 * 1024
EXE = os.path.join(orc.REF_DIR, "minimap2_cpu")


def write_fasta(path, recs):
    with open(path, "wb") as fh:
        for name, s in recs:
            fh.write(b">" + name.encode() + b"\n" + s + b"\n")


def paf(tgt, qry, args, skip, more=()):
    return subprocess.run([EXE, "-t", "1"] + args + list(more) + [f"--max-chain-skip={skip}", tgt, qry], check=True, capture_output=True).stdout.decode()


def record(fasta):
    """{"paf", "moved", "tp_S"} of every run; fasta: set name -> (references' file, reads' file, the reads' names)."""
    pafs, moved, tp_s = {}, {}, {}
    for run in rc.RUNS:
        name, kind = run.split(".")
        tgt, qry, names = fasta[name]
        for tag, skip in rc.SKIPS.items():
            key = f"{run}.{tag}"
            text = pafs[key] = paf(tgt, qry, rc.KINDS[kind][0], skip)
            assert set(names) - {ln.split("\t")[0] for ln in text.splitlines()}, f"{key}: every read has a line"
            if name == "chim":
                moved[key] = len(rc.moved_reads(text, paf(tgt, qry, rc.KINDS[kind][0], skip, more=["-P"])))
                assert moved[key] >= rc.MIN_MOVED, f"{key}: {moved[key]} reads keep a record at a moved place with another dv"
            else:
                tp_s[key] = sum("tp:A:S" in ln.split("\t") for ln in text.splitlines())
                assert tp_s[key] >= rc.MIN_TP_S, f"{key}: {tp_s[key]} tp:A:S lines"
    return dict(paf=pafs, moved=moved, tp_S=tp_s)


def main():
    assert os.path.exists(EXE), "build oracle/_ref first (make -C oracle ref)"
    genome, reads = rc.sim_chim()
    refs160, reads160 = rc.sim160()
    with tempfile.TemporaryDirectory() as d:
        fasta = {}
        for name, refs, rd in (("chim", [("chim_ref", genome)], reads), ("sim160", refs160, reads160)):
            fasta[name] = (os.path.join(d, name + "_ref.fa"), os.path.join(d, name + ".fa"), [n for n, _ in rd])
            write_fasta(fasta[name][0], refs)
            write_fasta(fasta[name][1], rd)
        out = record(fasta)
    out.update(seed=rc.CHIM_SEED, ref=[["chim_ref", genome.decode()]], reads=[[n, s.decode()] for n, s in reads])
    os.makedirs(rc.GOLD, exist_ok=True)
    path = os.path.join(rc.GOLD, "resident.npz")
    before = open(path, "rb").read() if os.path.exists(path) else None
    # (np.savez_compressed with the member's time stamp fixed: the same document gives the same file)
    member = io.BytesIO()
    np.lib.format.write_array(member, np.frombuffer(json.dumps(out, sort_keys=True, ensure_ascii=False).encode("utf-8"), dtype=np.uint8), allow_pickle=False)
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        z.writestr(zipfile.ZipInfo("doc.npy", date_time=(1980, 1, 1, 0, 0, 0)), member.getvalue(), zipfile.ZIP_DEFLATED)
    assert os.path.getsize(path) < LIMIT, f"{path} is {os.path.getsize(path)} bytes"
    if before is not None:
        print("the file is byte for byte what it was" if before == open(path, "rb").read() else "THE FILE CHANGED")
    for k in sorted(out["paf"]):
        print(f"{k}: {len(out['paf'][k].splitlines())} lines" + (f", {out['moved'][k]} of {len(reads)} reads with a kept record at a moved place and another dv" if k in out["moved"]
                                                                   else f", {out['tp_S'][k]} tp:A:S lines"))
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
