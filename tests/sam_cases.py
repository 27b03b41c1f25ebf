"""Cases for SAM output and = / X CIGARs from the mapper (the calls named _out): the recorded runs of the reference's CPU program
(tests/golden/sam/*.json.xz, written by tests/tools/gen_golden_sam.py: one JSON document each, {run: text}), the inputs they were made from, and
this project's mapper on the same inputs.  Test infrastructure only: imported by tests/test_sam_cpu.py, tests/test_gpu_sam.py,
tests/tools/gen_golden_sam.py and profiles/eqx_rate.py."""
import hashlib
import json
import lzma
import os

import numpy as np

import align_cases as ac
import golden_io
import mm2gb_amd as mm
import sim_reads

GOLD = os.path.join(golden_io.GOLD, "sam")
PAF_ALN = os.path.join(golden_io.GOLD, "paf_aln")
UNMAPPED = "read_of_random_bases"          # the read appended to the simulated set: it has no hit
UNMAPPED_LEN, UNMAPPED_SEED = 1500, 77

# run -> (the reference program's flags, map_align / map_sr / map_splice keywords, map_out keywords)
LONG_RUNS = {
    "a": (["-a"], dict(), dict(sam=True)),
    "a_eqx": (["-a", "--eqx"], dict(), dict(sam=True, eqx=True)),
    "a_Y_cs": (["-a", "-Y", "--cs"], dict(cs="short"), dict(sam=True, softclip=True)),
    "a_md_hit": (["-a", "--MD", "--sam-hit-only"], dict(md=True), dict(sam=True, hit_only=True)),
    "c_eqx": (["-c", "--eqx"], dict(), dict(eqx=True)),
    "c_eqx_cs": (["-c", "--eqx", "--cs"], dict(cs="short"), dict(eqx=True)),
}
INV_RUNS = {"a": LONG_RUNS["a"], "a_Y": (["-a", "-Y"], dict(), dict(sam=True, softclip=True))}
SR_RUNS = {"a": (["-x", "sr", "-a"], dict(align=True), dict(sam=True)), "a_eqx": (["-x", "sr", "-a", "--eqx"], dict(align=True), dict(sam=True, eqx=True))}
SPLICE_RUNS = {"a_cs": (["-a", "--cs"], dict(cs="short"), dict(sam=True)), "a_eqx": (["-a", "--eqx"], dict(), dict(sam=True, eqx=True))}
REF_ARGS = ["-t", "1", "--max-chain-skip=2147483647"]
CASES = {"long_map-ont": LONG_RUNS, "long_map-pb": LONG_RUNS, "inv": INV_RUNS, "sr": SR_RUNS, "splice": SPLICE_RUNS}


def save_runs(case, runs):
    """runs: {run: text}.  One JSON document, xz-compressed: the SEQ column repeats in every SAM run, which xz's window spans and deflate's does not."""
    path = os.path.join(GOLD, case + ".json.xz")
    with open(path, "wb") as fh:
        fh.write(lzma.compress(json.dumps(runs, sort_keys=True).encode(), preset=9 | lzma.PRESET_EXTREME))
    return os.path.getsize(path)


_runs = {}


def golden(case, run):
    if case not in _runs:
        _runs[case] = json.loads(lzma.decompress(open(os.path.join(GOLD, case + ".json.xz"), "rb").read()).decode())
    return _runs[case][run]


def split_sam(text):
    """(header lines without @PG, record lines)"""
    lines = text.splitlines()
    return [ln for ln in lines if ln.startswith("@") and not ln.startswith("@PG")], [ln for ln in lines if not ln.startswith("@")]


def same_text(got, want, what):
    """got / want: lists of lines"""
    if got != want:
        bad = [k for k in range(min(len(got), len(want))) if got[k] != want[k]]
        if not bad:
            raise AssertionError(f"{what}: {len(got)} lines against {len(want)}; the first {min(len(got), len(want))} agree")
        g, w = got[bad[0]], want[bad[0]]
        at = next((i for i, (x, y) in enumerate(zip(g, w)) if x != y), min(len(g), len(w)))
        raise AssertionError(f"{what}: {len(bad)} of {len(want)} lines differ (got {len(got)}); first: line {bad[0]}, byte {at}: {g[max(at - 60, 0):at + 60]!r} vs {w[max(at - 60, 0):at + 60]!r}")


# ---------------------------------------------------------------- the inputs
def long_meta():
    return json.load(open(os.path.join(GOLD, "sim.json")))


def unmapped_read():
    return UNMAPPED, sim_reads.BASES[np.random.default_rng(UNMAPPED_SEED).integers(0, 4, UNMAPPED_LEN)].tobytes()


def long_inputs(tmp_dir, meta=None):
    """(references, reads) as lists of (name, bytes): the simulated set of tests/golden/sam/sim.json, then the read of random bases."""
    meta = meta or long_meta()
    ref, reads = os.path.join(tmp_dir, "ref.fa"), os.path.join(tmp_dir, "reads.fa")
    sim_reads.simulate(ref, reads, **meta["sim"])
    if "ref_md5" in meta:
        assert hashlib.md5(open(ref, "rb").read()).hexdigest() == meta["ref_md5"], "simulator drifted: regenerate the golden"
        assert hashlib.md5(open(reads, "rb").read()).hexdigest() == meta["reads_md5"]
    return fasta(ref), fasta(reads) + [unmapped_read()]


def fasta(path):
    names = [ln[1:].split()[0].decode() for ln in open(path, "rb") if ln.startswith(b">")]
    return list(zip(names, ac.read_fasta(path)))


def inv_inputs():
    return fasta(os.path.join(ac.DATA, "t-inv.fa")), fasta(os.path.join(ac.DATA, "q-inv.fa"))


def write_fasta(path, recs):
    with open(path, "wb") as fh:
        for n, s in recs:
            fh.write(b">" + n.encode() + b"\n" + bytes(s) + b"\n")


# ---------------------------------------------------------------- this project's mapper on a case
def map_case(engine, case, run, inputs, align_on_device=0, eqx_on_device=0, text_on_device=0, stream=None, index=None):
    """(header + lines as the reference program prints them: SAM with the header in front, PAF as it is, stats).  inputs: (references, reads); stream: chunk_bases, or None
    for the single call; engine: one engine, or a list for the stream."""
    refs, reads = inputs
    flags, akw, okw = CASES[case][run]
    out = mm.map_out(eqx_on_device=eqx_on_device, **okw)
    names, seqs = [n for n, _ in refs], [s for _, s in refs]
    dev = dict(align_on_device=align_on_device, text_on_device=text_on_device)
    if case == "sr":
        import sr_cases as sc
        ix, opt, k, al = index or sc.index(), mm.map_opt_sr(host_threads=4), mm.preset_sr()["k"], mm.map_sr(refs=seqs, **akw, **dev)
    elif case == "splice":
        ix, opt, k, al = index or mm.SeedIndex(seqs, **mm.preset("splice")), mm.map_opt_splice(host_threads=4), 15, mm.map_splice(seqs, **akw, **dev)
    else:
        preset = "map-pb" if case.endswith("map-pb") else "map-ont"
        ix = index or mm.SeedIndex(seqs, **(mm.preset("map-pb") if preset == "map-pb" else {}))
        opt, k, al = mm.map_opt(host_threads=4), 19 if preset == "map-pb" else 15, mm.map_align(seqs, preset=preset, **akw, **dev)
    if stream is None:
        text, st = mm.map_reads(engine, ix, names, reads, opt=opt, k=k, align=al, out=out)
    else:
        text, st = mm.map_reads_stream(engine if isinstance(engine, list) else [engine], ix, names, reads, opt=opt, k=k, chunk_bases=stream, align=al, out=out)
    head = mm.sam_header(names, [len(s) for s in seqs]) if okw.get("sam") else ""
    return head + text, st


def assert_case(got, case, run, what):
    want = golden(case, run)
    if CASES[case][run][2].get("sam"):
        (gh, gl), (wh, wl) = split_sam(got), split_sam(want)
        same_text(gh, wh, what + ": header")
        same_text(gl, wl, what)
    else:
        same_text(got.splitlines(), want.splitlines(), what)
