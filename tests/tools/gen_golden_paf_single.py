"""Records tests/golden/paf_single: single-affine gap scoring (q == q2 && e == e2, where mm_align_pair runs ksw_extz2_sse) to the PAF.

pafs_<case>.npz (entries c, cs, long_md: the PAF as bytes): what the reference's CPU program prints with one number to -O and one to -E --
oracle/_ref/minimap2_cpu -t 1 --max-chain-skip=2147483647 -O4 -E2 with `-c`, `-c --cs` and `--cs=long --MD -c` -- for MT-human x MT-orang,
t-inv / q-inv and the simulated reads of tests/golden/paf_aln/sim.json.

align_ont.npz, align_pb.npz (tests/align_cases.save_batch): the reads of tests/ksw_single_cases.align_fixture -- the path reads of
tests/golden/align's `ont` and `pb` batches and six with a gap of 25-90 bases -- through the reference's mm_align_skeleton at map-ont with (q, e) = (q2, e2) = (4, 2) and at map-pb with (6, 2): the call's input and what the reference
answered.  Needs oracle/_ref, as gen_golden_align.py does.  While recording it asserts that the answers differ from the dual-affine ones
(otherwise the fixtures would show nothing) and that this project's host form gives the same records and words.

    python tests/tools/gen_golden_paf_single.py
"""
import hashlib
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
import golden_io  # noqa: E402
import ksw_single_cases as ks  # noqa: E402
import mm2gb_amd as mm  # noqa: E402
import orc  # noqa: E402
import sim_reads  # noqa: E402

LIMIT = 142 * 1024          # no fixture larger than the largest of tests/golden/paf_aln
VARIANTS = {"c": ["-c"], "cs": ["-c", "--cs"], "long_md": ["--cs=long", "--MD", "-c"]}


def paf(tgt, qry, extra):
    exe = os.path.join(orc.REF_DIR, "minimap2_cpu")
    return subprocess.run([exe, "-t", "1", "--max-chain-skip=2147483647"] + extra + [tgt, qry], check=True, capture_output=True).stdout.decode()


def save(case, pafs):
    path = os.path.join(ks.PAF_GOLD, f"pafs_{case}.npz")
    np.savez_compressed(path, **{v: np.frombuffer(t.encode(), np.uint8) for v, t in pafs.items()})
    print(case, {v: len(t.splitlines()) for v, t in pafs.items()}, "lines,", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= LIMIT


def record_pafs():
    differs = []
    for case, tgt, qry in (("mt", "MT-human.fa", "MT-orang.fa"), ("inv", "t-inv.fa", "q-inv.fa")):
        t, q = os.path.join(ac.DATA, tgt), os.path.join(ac.DATA, qry)
        pafs = {v: paf(t, q, ks.PAF_FLAGS + flags) for v, flags in VARIANTS.items()}
        differs.append(pafs["c"] != paf(t, q, ["-c"]))
        save(case, pafs)
    meta = json.load(open(os.path.join(golden_io.GOLD, "paf_aln", "sim.json")))
    with tempfile.TemporaryDirectory() as d:
        ref, reads = os.path.join(d, "ref.fa"), os.path.join(d, "reads.fa")
        sim_reads.simulate(ref, reads, **meta["sim"])
        assert hashlib.md5(open(ref, "rb").read()).hexdigest() == meta["ref_md5"] and hashlib.md5(open(reads, "rb").read()).hexdigest() == meta["reads_md5"]
        pafs = {v: paf(ref, reads, ks.PAF_FLAGS + flags) for v, flags in VARIANTS.items()}
        differs.append(pafs["c"] != paf(ref, reads, ["-c"]))
        save("sim", pafs)
    print("PAF differs from the default costs':", differs)
    assert differs[-1], "the simulated reads print the same PAF at -O4 -E2 as at the default costs: the fixture would show nothing"


def record_align():
    for name, (q, e) in ks.ALIGN_BATCHES.items():
        refs, reads, preset = ks.align_fixture(name)
        b, want = ac.ref_batch(refs, reads, preset, q=q, e=e, q2=q, e2=e)
        _, dual = ac.ref_batch(refs, reads, preset, q=q, e=e)
        assert any(w[1].tobytes() != d[1].tobytes() or w[2].tobytes() != d[2].tobytes() for w, d in zip(want, dual)), f"{name}: the single-affine answers are the dual-affine ones"
        ac.assert_same(mm.align_regs_extz_host(b["opt"], b["k"], b["hpc"], b["refs"], b["reads"], b["regs"], b["anchors"])[0], want, name)
        path = os.path.join(ks.PAF_GOLD, f"align_{name}.npz")
        ac.save_batch(path, b, want)
        print(name, sum(len(w[0]) for w in want), "records,", os.path.getsize(path), "bytes")
        assert os.path.getsize(path) <= LIMIT


if __name__ == "__main__":
    assert ac.ref_available(), "build oracle/_ref first (make -C oracle ref)"
    os.makedirs(ks.PAF_GOLD, exist_ok=True)
    record_pafs()
    record_align()
