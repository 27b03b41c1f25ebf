#!/usr/bin/env python3
"""Makes tests/golden/scale/scale.npz (one JSON document, compressed): {run: text}, what oracle/_ref/minimap2_cpu -t 1 prints for the genome and the 209 reads of
tests/golden/sr with the long-read options -- the defaults, -x map-pb, --no-long-join and -x map-pb --no-long-join, each with --max-chain-skip=2147483647 (the runs of
tests/scale_cases.py: LONG_RUNS).  Recorded output only; the reads and the genome are the short-read fixture's.  Needs the reference built under oracle/_ref (make -C
oracle ref, where the reference checkout exists); it is run as a plain child process.

tests/test_gpu_scale.py maps the 209 reads c times over in one batch and expects the text c times over.  That holds because the reference keeps no state from read to
read and a read's hash is its name's, mixed with its length; the generator asserts it for every run on three copies of the reads.  It writes the file with the member's
time stamp fixed: the same document gives the same bytes, and it says whether the file changed."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import scale_cases as sx  # noqa: E402

LIMIT = 142 * 1024          # no fixture larger than the largest of tests/golden/paf_aln


def main():
    assert os.path.exists(sx.REF_EXE), "build oracle/_ref first (make -C oracle ref)"
    doc = sx.record_long()
    thrice = sx.record_long(times=3)
    for run, text in doc.items():
        assert text and thrice[run] == text * 3, f"{run}: three copies of the reads do not print three copies of the text"
    os.makedirs(sx.GOLD, exist_ok=True)
    path = os.path.join(sx.GOLD, "scale.npz")
    before = open(path, "rb").read() if os.path.exists(path) else None
    data = sx.long_doc_bytes(doc)
    with open(path, "wb") as fh:
        fh.write(data)
    assert len(data) < LIMIT, f"{path} is {len(data)} bytes"
    if before is not None:
        print("the file is byte for byte what it was" if before == data else "THE FILE CHANGED")
    for run, text in doc.items():
        rows = [ln.split("\t") for ln in text.splitlines()]
        print(f"{run}: {len(rows)} lines, {len({f[0] for f in rows})} of 209 reads mapped, {sum('tp:A:S' in f for f in rows)} tp:A:S, {len(text)} bytes")
    print(f"{path}: {len(data)} bytes")


if __name__ == "__main__":
    main()
