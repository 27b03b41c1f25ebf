"""Records tests/golden/sam.

<case>.json.xz (one JSON document {run: text}, xz-compressed): what the reference's CPU program prints -- oracle/_ref/minimap2_cpu -t 1
--max-chain-skip=2147483647 -- for the runs of tests/sam_cases.py:
  long_map-ont / long_map-pb   the simulated set of tests/golden/paf_aln (sim_reads.simulate; 2-12 kb reads on 300 kb) plus one read of random bases, which stays
                               unmapped, at the default preset and at -x map-pb: -a, -a --eqx, -a -Y --cs, -a --MD --sam-hit-only, and for PAF -c --eqx, -c --eqx --cs
  inv                          -a and -a -Y on t-inv x q-inv (the inversion line; supplementary lines with H and with S clips)
  sr                           -x sr -a and -x sr -a --eqx on the reads of tests/golden/sr
  splice                       -x splice --cap-sw-mem=100000000 -a --cs and ... -a --eqx on the reads of tests/golden/splice/pafs.npz
sim.json: the simulated set's parameters and md5s.  The set has as many reads, 24 at the most, as keep every file within LIMIT, and the first seed (the one of
tests/golden/paf_aln first) that gives what the tests rely on; the tool asserts it: a 0x100 line with SEQ "*", a 0x10 line, a zd:i line, a flag-4 line that --sam-hit-only leaves out, = and X words
under --eqx; and in the other cases what simulated reads without a chimera cannot show: a 0x800 line with SA:Z on its read's primary line (inv, sr, splice), a record with H
clips without -Y and S clips with it (inv), and in the spliced run an N word between = words.

eqx_<batch>.npz: for every batch of tests/golden/align the words mm_align_skeleton (oracle/_ref/libminimap2ref.so) leaves with MM_F_EQX set, per record, as
tests/test_eqx_cpu.py and tests/test_gpu_eqx.py expect them.  While recording it asserts that records and scores are those recorded without the flag (the rewrite is
mm_update_extra's last statement: nothing after it tells M from = / X) and that this project's host form gives the same words.

This project's mapper needs a device; where one is there (--check) the tool also asserts that the mapper's host forms give the recorded bytes.

    python tests/tools/gen_golden_sam.py [--check]
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import align_cases as ac  # noqa: E402
import eqx_cases as ec  # noqa: E402
import mm2gb_amd as mm  # noqa: E402
import orc  # noqa: E402
import sam_cases as sc  # noqa: E402
import sim_reads  # noqa: E402

LIMIT = 142 * 1024          # no fixture larger than the largest committed so far


def run_ref(tgt, qry, extra):
    exe = os.path.join(orc.REF_DIR, "minimap2_cpu")
    return subprocess.run([exe] + sc.REF_ARGS + extra + [tgt, qry], check=True, capture_output=True).stdout.decode()


def rows(text):
    return [ln.split("\t") for ln in text.splitlines() if not ln.startswith("@")]


def long_has_all(runs):
    """The lines the tests rely on, in the runs of one preset; a list of what is missing."""
    a, eqx, y, hit = rows(runs["a"]), rows(runs["a_eqx"]), rows(runs["a_Y_cs"]), rows(runs["a_md_hit"])
    missing = []
    if not any(int(r[1]) & 0x100 and r[9] == "*" for r in a):
        missing.append("a 0x100 line with SEQ *")
    if not any(int(r[1]) & 0x10 for r in a):
        missing.append("a 0x10 line")
    if not any(int(r[1]) == 4 for r in a) or any(int(r[1]) == 4 for r in hit):
        missing.append("a flag-4 line that --sam-hit-only leaves out")
    if not all(any(f.startswith("cs:Z:") for f in r) for r in y if int(r[1]) != 4):
        missing.append("cs:Z on every line of a hit under --cs")
    if not any("=" in r[5] and "X" in r[5] for r in eqx) or any("M" in r[5] for r in eqx):
        missing.append("= and X words under --eqx")
    if not any("\tzd:i:" in "\t".join(r) for r in a):
        missing.append("a zd:i line")
    paf = rows(runs["c_eqx_cs"])
    if not all(any(f.startswith("cg:Z:") and "=" in f and "M" not in f[5:] for f in r) and any(f.startswith("cs:Z:") for f in r) for r in paf):
        missing.append("cg:Z with = and cs:Z on every PAF line under -c --eqx --cs")
    return missing


def record_long():
    presets = (("map-ont", []), ("map-pb", ["-x", "map-pb"]))
    base = json.load(open(os.path.join(sc.PAF_ALN, "sim.json")))["sim"]
    with tempfile.TemporaryDirectory() as d:
        for n_reads in (base["n_reads"], 20, 16, 12, 8):
            for seed in [base["seed"]] + [s for s in range(1, 60) if s != base["seed"]]:
                meta = dict(sim=dict(base, seed=seed, n_reads=n_reads))
                refs, reads = sc.long_inputs(d, meta)
                qry = os.path.join(d, "reads_all.fa")
                sc.write_fasta(qry, reads)
                with ThreadPoolExecutor(os.cpu_count() or 1) as pool:          # (a run takes about a minute: max-chain-skip is off)
                    futs = {(p, r): pool.submit(run_ref, os.path.join(d, "ref.fa"), qry, extra + flags) for p, extra in presets for r, (flags, _, _) in sc.LONG_RUNS.items()}
                runs = {p: {r: futs[(p, r)].result() for r in sc.LONG_RUNS} for p, _ in presets}
                missing = {p: long_has_all(runs[p]) for p, _ in presets}
                if not any(missing.values()):
                    break
                print(f"{n_reads} reads, seed {seed}: missing {missing}")
            else:
                raise AssertionError(f"{n_reads} reads: no seed gives every kind of line at both presets")
            sizes = [sc.save_runs("long_" + p, runs[p]) for p, _ in presets]
            print(f"{n_reads} reads, seed {seed}:", sizes, "bytes")
            if max(sizes) <= LIMIT:
                break
        else:
            raise AssertionError("no read set fits")
        meta["ref_md5"] = hashlib.md5(open(os.path.join(d, "ref.fa"), "rb").read()).hexdigest()
        meta["reads_md5"] = hashlib.md5(open(os.path.join(d, "reads.fa"), "rb").read()).hexdigest()
    json.dump(meta, open(os.path.join(sc.GOLD, "sim.json"), "w"), indent=1, sort_keys=True)


def has_supplementary(r_):
    """a 0x800 line, and SA:Z on its read's primary line"""
    supp = {r[0] for r in r_ if int(r[1]) & 0x800}
    return bool(supp) and all(any(f.startswith("SA:Z:") for f in r) for r in r_ if r[0] in supp and int(r[1]) & 0x900 == 0)


def record_inv():
    runs = {r: run_ref(os.path.join(ac.DATA, "t-inv.fa"), os.path.join(ac.DATA, "q-inv.fa"), flags) for r, (flags, _, _) in sc.INV_RUNS.items()}
    assert "tp:A:I" in runs["a"] or "tp:A:i" in runs["a"], "no inversion line"
    a, y = rows(runs["a"]), rows(runs["a_Y"])
    assert has_supplementary(a), "no 0x800 line with SA:Z on its read's primary line"
    assert any(int(r[1]) & 0x800 and "H" in r[5] and "S" in s[5] and "H" not in s[5] and len(s[9]) > len(r[9]) for r, s in zip(a, y)), "no record with H clips without -Y and S clips with it"
    assert sc.save_runs("inv", runs) <= LIMIT


def record_sr():
    import sr_cases
    g = sr_cases.gold()
    with tempfile.TemporaryDirectory() as d:
        sc.write_fasta(os.path.join(d, "ref.fa"), [("ref", g["genome"].encode())])
        sc.write_fasta(os.path.join(d, "reads.fa"), sr_cases.reads())
        runs = {r: subprocess.run([os.path.join(orc.REF_DIR, "minimap2_cpu"), "-t", "1"] + flags + [os.path.join(d, "ref.fa"), os.path.join(d, "reads.fa")], check=True,
                                  capture_output=True).stdout.decode() for r, (flags, _, _) in sc.SR_RUNS.items()}
    a = rows(runs["a"])
    assert any(int(r[1]) == 4 for r in a) and any(int(r[1]) & 0x10 for r in a), "the short reads give no flag-4 or no 0x10 line"
    assert not any(int(r[1]) & 0x100 for r in a), "MM_F_NO_PRINT_2ND leaves no secondary line"
    assert has_supplementary(a)
    assert any("X" in r[5] for r in rows(runs["a_eqx"])) and not any("M" in r[5] for r in rows(runs["a_eqx"]))
    size = sc.save_runs("sr", runs)
    assert size <= LIMIT, size
    print("sr", {k: len(rows(v)) for k, v in runs.items()}, size, "bytes")


def record_splice():
    import re
    import splice_cases
    refs, reads, _ = splice_cases.load_pafs()
    with tempfile.TemporaryDirectory() as d:
        sc.write_fasta(os.path.join(d, "ref.fa"), refs)
        sc.write_fasta(os.path.join(d, "reads.fa"), reads)
        runs = {r: subprocess.run([os.path.join(orc.REF_DIR, "minimap2_cpu")] + splice_cases.PAF_OPTIONS + flags + [os.path.join(d, "ref.fa"), os.path.join(d, "reads.fa")],
                                  check=True, capture_output=True).stdout.decode() for r, (flags, _, _) in sc.SPLICE_RUNS.items()}
    assert any(re.search(r"=\d+N\d+=", r[5]) for r in rows(runs["a_eqx"])), "no N word between = words"
    assert "~" in runs["a_cs"] and "\tts:A:" in runs["a_cs"] and has_supplementary(rows(runs["a_cs"]))
    size = sc.save_runs("splice", runs)
    assert size <= LIMIT, size
    print("splice", {k: len(rows(v)) for k, v in runs.items()}, size, "bytes")


def record_eqx_words():
    fx = ac.fixture_batches()
    seen = {k: 0 for k in ("eq", "x", "rev", "records")}
    for name in ec.BATCHES:
        refs, reads, preset, over = fx[name]
        b, _ = ac.load_batch(name)
        args = ec.golden_args(name)
        regs, read_of, aln, cigar = args[2:]
        eregs, _, ealn, ecigar = ec.ref_words(refs, reads, preset, anchors=b["anchors"], **over)
        assert np.array_equal(regs, eregs), f"{name}: MM_F_EQX changes the records"
        for k in ("dp_score", "dp_max", "dp_max2", "n_ambi", "trans_strand"):
            assert np.array_equal(aln[k], ealn[k]), f"{name}: MM_F_EQX changes {k}"
        want = ec.split(ealn, ecigar)
        ec.assert_words(mm.cigar_eqx_host(*args), want, f"{name}: host form against the reference")
        path = os.path.join(sc.GOLD, f"eqx_{name}.npz")
        np.savez_compressed(path, words=ecigar, off=np.where(ealn["cigar_off"] >= 0, ealn["cigar_off"], 0).astype(np.int64),
                            n=np.where(ealn["cigar_off"] >= 0, ealn["n_cigar"], -1).astype(np.int32))
        assert os.path.getsize(path) <= LIMIT, f"{path}: {os.path.getsize(path)} bytes"
        seen["eq"] += int((ecigar & 0xf == 7).sum()); seen["x"] += int((ecigar & 0xf == 8).sum()); seen["rev"] += int((regs["flags"] >> 10 & 1).sum()); seen["records"] += len(regs)
        assert not (ecigar & 0xf == 0).any()
        print(name, len(regs), "records,", len(cigar), "->", len(ecigar), "words,", os.path.getsize(path), "bytes")
    assert all(seen.values()), seen
    # the same for the `default` batch of tests/golden/splice: N words from the reference's own splice path
    import splice_cases
    refs, batches = splice_cases.fixture_batches()
    reads, preset, kw = batches["default"]
    b, _, _ = splice_cases.load_batch("default")
    args = ec.golden_splice_args()
    _, ewant, _ = splice_cases.ref_batch(refs, reads, preset, anchors=b["anchors"], flag_set=mm.F_EQX, **kw)
    eregs, _, ealn, ecigar = mm.flatten_aligned(ewant)
    assert np.array_equal(args[2], eregs) and (ecigar & 0xf == 3).any(), "splice: MM_F_EQX changes the records, or no N word"
    ec.assert_words(mm.cigar_eqx_host(*args), ec.split(ealn, ecigar), "splice default: host form against the reference")
    path = os.path.join(sc.GOLD, "eqx_splice_default.npz")
    np.savez_compressed(path, words=ecigar, off=np.where(ealn["cigar_off"] >= 0, ealn["cigar_off"], 0).astype(np.int64), n=np.where(ealn["cigar_off"] >= 0, ealn["n_cigar"], -1).astype(np.int32))
    assert os.path.getsize(path) <= LIMIT
    print("splice default", len(eregs), "records,", len(ecigar), "words,", os.path.getsize(path), "bytes")


def check_mapper():
    """This project's mapper on host threads against what has just been recorded (needs a device: the chaining runs there)."""
    import splice_cases
    import sr_cases
    with mm.Engine() as e, tempfile.TemporaryDirectory() as d:
        inputs = {"long_map-ont": sc.long_inputs(d), "inv": sc.inv_inputs(), "sr": ([("ref", sr_cases.gold()["genome"].encode())], sr_cases.reads()), "splice": splice_cases.load_pafs()[:2]}
        inputs["long_map-pb"] = inputs["long_map-ont"]
        for case, runs in sc.CASES.items():
            for run in runs:
                got, _ = sc.map_case(e, case, run, inputs[case], align_on_device=-1, eqx_on_device=-1, text_on_device=-1)
                sc.assert_case(got, case, run, f"{case} {run}: the mapper's host forms")
                print(case, run, "ok")


def main():
    assert ac.ref_available() and os.path.exists(os.path.join(orc.REF_DIR, "minimap2_cpu")), "build oracle/_ref first (make -C oracle ref)"
    os.makedirs(sc.GOLD, exist_ok=True)
    record_eqx_words()
    record_long()
    record_inv()
    record_sr()
    record_splice()
    if "--check" in sys.argv:
        check_mapper()


if __name__ == "__main__":
    main()
