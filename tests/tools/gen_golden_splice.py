"""Records tests/golden/splice: the genome of splice_cases.genes() and, for every option set of splice_cases.fixture_batches(), the call's input
(records and anchors as map.c has them under -x splice when it calls align_regs, made by the reference's own chaining on this project's
anchors) and the answers of the reference's mm_align_skeleton, run with mm_set_opt(preset) and max_sw_mat = 100 000 000 (the stated departure).
Needs oracle/_ref/libminimap2ref.so.  While recording it asserts that this project's host form equals the reference on every batch -- the path
counts are the host form's, and they describe the reference's run only because every record and word agrees -- that the batches together
reach every path of splice_cases.MUST_HAVE, and that only the batch made for it goes over max_sw_mat; counts and the inputs' md5 go to meta.json.  For two of the batches it also records the cs (short, long) and MD strings the reference's
mm_gen_cs_or_MD prints for the reference's records, and asserts that this project's text call gives them.

    python tests/tools/gen_golden_splice.py
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np  # noqa: E402

import align_cases as ac  # noqa: E402
import splice_cases as sc  # noqa: E402


def record_pafs(refs, meta):
    """What the reference's CPU program prints for about 120 reads under -x splice with the stated max_sw_mat, in four forms."""
    import subprocess
    import tempfile
    import orc
    import sim_reads
    reads = sc.paf_reads()
    exe = os.path.join(orc.REF_DIR, "minimap2_cpu")
    with tempfile.TemporaryDirectory() as d:
        ref_fa, read_fa = os.path.join(d, "ref.fa"), os.path.join(d, "reads.fa")
        sim_reads.write_fasta(ref_fa, [(f"ref{i}", np.frombuffer(s, np.uint8)) for i, s in enumerate(refs)])
        sim_reads.write_fasta(read_fa, [(n, np.frombuffer(s, np.uint8)) for n, s in reads])
        pafs = {v: subprocess.run([exe] + sc.PAF_OPTIONS + flags + [ref_fa, read_fa], check=True, capture_output=True).stdout.decode() for v, flags in sc.PAF_VARIANTS.items()}
    text = pafs["cs"]
    lines = text.splitlines()
    assert "\tts:A:+" in text and "\tts:A:-" in text and any("\tts:A:" not in ln for ln in lines), "ts:A:+, ts:A:- and lines without ts must all occur"
    assert "~" in text and "N" in pafs["c"] and "\tMD:Z:" in pafs["md"] and "\tcs:Z:=" in pafs["cs_long"]
    mapped = {ln.split("\t")[0] for ln in lines}
    sc.save_pafs(reads, pafs)
    meta["paf"] = dict(reads=len(reads), lines=len(lines), reads_mapped=len(mapped), options=sc.PAF_OPTIONS, reads_md5=hashlib.md5(b"\n".join(s for _, s in reads)).hexdigest(),
                       ts_plus=text.count("\tts:A:+"), ts_minus=text.count("\tts:A:-"), no_ts=sum("\tts:A:" not in ln for ln in lines))
    print("paf", meta["paf"])


def main():
    assert ac.ref_available(), "build oracle/_ref first (make -C oracle ref)"
    os.makedirs(sc.GOLD, exist_ok=True)
    refs, batches = sc.fixture_batches()
    sc.save_genome(refs)
    meta = dict(batches={}, total={}, genome_md5=hashlib.md5(b"".join(refs)).hexdigest(), max_sw_mat=sc.MAX_SW_MAT)
    planted = [n for n, _ in sc.planted_reads(refs, sc.genes()[1])]
    meta["default_names"] = planted + ["random"] * (len(batches["default"][0]) - len(planted))
    for name, (reads, preset, kw) in batches.items():
        b, want, preset_values = sc.ref_batch(refs, reads, preset, **kw)
        got, info = sc.run_host(b, threads=4)
        ac.assert_same(got, want, f"{name}: host form against the reference")
        assert (info["splice_counts"]["over_sw_mat"] > 0) == (name == "small_mat"), name
        sc.save_batch(name, b, want, preset_values)
        meta["batches"][name] = dict(preset=preset, options=kw, reads=len(reads), records=sum(len(w[0]) for w in want), reads_md5=hashlib.md5(b"\n".join(reads)).hexdigest(),
                                     splice_counts=info["splice_counts"], counts=info["counts"])
        for k, v in info["splice_counts"].items():
            meta["total"][k] = meta["total"].get(k, 0) + v
        print(name, len(reads), "reads", {k: v for k, v in info["splice_counts"].items() if v})
    import aln_text_cases as at
    import mm2gb_amd as mm
    for name in sc.TEXT_BATCHES:          # what mm_gen_cs_or_MD prints for the reference's own records, and this project's host form against it
        args = sc.golden_text_args(name)
        texts = at.ref_texts(*args)
        sc.save_texts(name, texts)
        for what in (mm.TEXT_CS, mm.TEXT_CS | mm.TEXT_CS_LONG, mm.TEXT_MD, mm.TEXT_CG | mm.TEXT_CS):
            off, text = mm.aln_text_splice_host(what, *args)
            at.assert_texts(at.split(off, text), at.want_for(args, texts, what), f"{name}: text {what}")
        meta["batches"][name]["text_records"] = len(texts["cs"])
        meta["batches"][name]["text_introns"] = sum(x.count(b"~") for x in texts["cs"])
    record_pafs(refs, meta)
    missing = [k for k in sc.MUST_HAVE if not meta["total"].get(k)]
    assert not missing, f"the reference's answers contain none of: {missing}"
    json.dump(meta, open(os.path.join(sc.GOLD, "meta.json"), "w"), indent=1, sort_keys=True)
    print({f: os.path.getsize(os.path.join(sc.GOLD, f)) for f in sorted(os.listdir(sc.GOLD))})


if __name__ == "__main__":
    main()
