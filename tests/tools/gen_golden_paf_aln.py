"""Records tests/golden/paf_aln.

pafs_<case>.npz (entries c, cs, long_md: the PAF as bytes; compressed, like the other fixtures): what the reference's CPU program prints with
base-level alignment -- oracle/_ref/minimap2_cpu -t 1 --max-chain-skip=2147483647 with `-c`, `-c --cs` and `--cs=long --MD -c` (which prints
MD) -- for MT-human x MT-orang, t-inv / q-inv, t2 / q2 and a simulated set (tests/sim_reads.simulate: reads of 2-12 kb on a genome of 300 kb;
its parameters and md5s go to sim.json) at the default preset and at -x map-pb.  While recording it asserts what tests/test_gpu_mapper_aln.py
relies on: an inversion line for t-inv / q-inv, and in the simulated set a secondary line, a zd:i line and a reverse-strand line.  The set has
as many reads, 24 at the most, as keep either preset's file within LIMIT, and the first seed that gives the three kinds of line.

text_*.npz: for every batch of tests/golden/align the text the reference's mm_gen_cs_or_MD (format.c:251) prints
for each of the reference's own records -- cs short, cs long and MD -- as tests/test_aln_text_cpu.py and tests/test_gpu_aln_text.py expect it.
Needs oracle/_ref/libminimap2ref.so, as gen_golden_align.py does.  While recording it asserts that this project's host form gives the same
bytes, and that the records contain what the tests rely on: a reverse-strand record, a record without a CIGAR word to spare (every batch
has records), insertions, deletions and an ambiguous base.

    python tests/tools/gen_golden_paf_aln.py
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
import aln_text_cases as tc  # noqa: E402
import mm2gb_amd as mm  # noqa: E402
import orc  # noqa: E402
import sim_reads  # noqa: E402

LIMIT = 142 * 1024          # no fixture larger than the largest committed so far


VARIANTS = {"c": ["-c"], "cs": ["-c", "--cs"], "long_md": ["--cs=long", "--MD", "-c"]}
SIM = dict(len_lo=2_000, len_hi=12_000, n_chr=3, chr_len=100_000, n_rep_families=2, rep_len=3000, copies=12, tandem=2)


def paf(tgt, qry, extra):
    exe = os.path.join(orc.REF_DIR, "minimap2_cpu")
    return subprocess.run([exe, "-t", "1", "--max-chain-skip=2147483647"] + extra + [tgt, qry], check=True, capture_output=True).stdout.decode()


def has_all(text):
    rows = [ln.split("\t") for ln in text.splitlines()]
    return any("tp:A:S" in r for r in rows) and any(f.startswith("zd:i:") for r in rows for f in r) and any(r[4] == "-" for r in rows)


def save(case, pafs):
    path = os.path.join(tc.GOLD, f"pafs_{case}.npz")
    np.savez_compressed(path, **{v: np.frombuffer(t.encode(), np.uint8) for v, t in pafs.items()})
    print(case, {v: len(t.splitlines()) for v, t in pafs.items()}, "lines,", os.path.getsize(path), "bytes")
    return os.path.getsize(path)


def record_pafs():
    for case, tgt, qry in (("mt", "MT-human.fa", "MT-orang.fa"), ("inv", "t-inv.fa", "q-inv.fa"), ("q2", "t2.fa", "q2.fa")):
        pafs = {v: paf(os.path.join(ac.DATA, tgt), os.path.join(ac.DATA, qry), flags) for v, flags in VARIANTS.items()}
        for v, text in pafs.items():
            if case == "q2":
                assert text == "", "t2 / q2 has no hit in today's goldens either (real_q2_inf.paf): it stays the case of no output"
            else:
                assert "\tcg:Z:" in text and ("\tcs:Z:" in text) == (v == "cs") and ("\tMD:Z:" in text) == (v == "long_md")
            if case == "inv":
                assert "tp:A:I" in text or "tp:A:i" in text, "no inversion line"
        assert save(case, pafs) <= LIMIT
    presets = (("map-ont", []), ("map-pb", ["-x", "map-pb"]))
    with tempfile.TemporaryDirectory() as d:
        ref, reads = os.path.join(d, "ref.fa"), os.path.join(d, "reads.fa")
        for n_reads in (24, 20, 16, 12, 8):
            for seed in range(1, 60):
                sim_reads.simulate(ref, reads, seed=seed, n_reads=n_reads, **SIM)
                if all(has_all(paf(ref, reads, extra + ["-c"])) for _, extra in presets):
                    break
            else:
                raise AssertionError(f"{n_reads} reads: no seed gives a secondary, a zd:i and a reverse-strand line at both presets")
            sizes = []
            for preset, extra in presets:
                pafs = {v: paf(ref, reads, extra + flags) for v, flags in VARIANTS.items()}
                assert all(has_all(t) for t in pafs.values())
                sizes.append(save("sim_" + preset, pafs))
            if max(sizes) <= LIMIT:
                break
        else:
            raise AssertionError("no read set fits")
        meta = dict(sim=dict(SIM, seed=seed, n_reads=n_reads), ref_md5=hashlib.md5(open(ref, "rb").read()).hexdigest(), reads_md5=hashlib.md5(open(reads, "rb").read()).hexdigest())
    json.dump(meta, open(os.path.join(tc.GOLD, "sim.json"), "w"), indent=1, sort_keys=True)


def main():
    assert ac.ref_available(), "build oracle/_ref first (make -C oracle ref)"
    os.makedirs(tc.GOLD, exist_ok=True)
    record_pafs()
    seen = dict(rev=0, fwd=0, ins=0, dele=0, n_ambi=0, records=0)
    for name in tc.BATCHES:
        args = tc.golden_args(name)
        texts = tc.ref_texts(*args)
        for m, (what, _, _) in tc.MODES.items():
            got = tc.split(*mm.aln_text_host(what, *args))
            tc.assert_texts(got, [tc.TAG[m] + t if args[4]["cigar_off"][i] >= 0 else b"" for i, t in enumerate(texts[m])], f"{name}: host form against the reference, {m}")
        path = os.path.join(tc.GOLD, f"text_{name}.npz")
        np.savez_compressed(path, **{m: np.frombuffer(b"".join(texts[m]), np.uint8) for m in tc.MODES},
                            **{m + "_off": np.cumsum([0] + [len(t) for t in texts[m]]).astype(np.int64) for m in tc.MODES})
        assert os.path.getsize(path) <= LIMIT, f"{path}: {os.path.getsize(path)} bytes"
        regs, aln, cigar = args[2], args[4], args[5]
        seen["records"] += len(regs)
        seen["rev"] += int((regs["flags"] >> 10 & 1).sum()); seen["fwd"] += int((~regs["flags"] >> 10 & 1).sum())
        seen["ins"] += int((cigar & 0xf == 1).sum()); seen["dele"] += int((cigar & 0xf == 2).sum()); seen["n_ambi"] += int(aln["n_ambi"].sum())
        print(name, len(regs), "records,", os.path.getsize(path), "bytes")
    missing = [k for k, v in seen.items() if not v]
    assert not missing, f"the recorded batches contain none of: {missing}"
    print(seen)


if __name__ == "__main__":
    main()
