#!/usr/bin/env python3
"""The text of the alignment tags and the mapper's -c, two legs on one batch: the records the device form of the alignment call gives for reads of 5-60 kb at 8 %
error from tests/sim_reads.simulate against its 3 Mbp genome, map-ont.  Forms, alternated in one process, `--runs` timed runs each after a warm-up
that also checks that all agree byte for byte:
  reference  the reference's mm_gen_cs_or_MD through ctypes, one record per call on `--threads` threads (ctypes releases the interpreter lock
             for the call; the records it reads are laid out before the clock starts).  It has no call for cg:Z alone: that row has no reference leg;
Leg (a), the text alone:
  host       mm2gb_aln_text_host on `--threads` threads;
  device     mm2gb_aln_text_gpu: the whole call (residues up, words up, kernels, text back), and the same without the copies of the residues
             (what the mapper pays when the alignment call left them resident) and the kernels with the words' upload alone.
For cg:Z, cs:Z short and MD:Z.  The yardstick for the mapper's default (text_on_device = 0) is the host form: the device form takes over only
if it is faster WITH its copies in every repeat.
Leg (b), the whole mapper: map_reads(..., align=map_align(refs)) on one engine with `--threads` host threads, index built before the clock
starts (its seconds are reported), against oracle/_ref/minimap2_cpu -c -t `--threads` --max-chain-skip=2147483647 on the same two files, a whole
program from start to exit: it reads the files and builds its index inside its time.  After a warm-up of both, `--runs` runs each, alternated;
the stage seconds of every run, and how many PAF lines differ (reads that met a tie in the range-minimum query are a documented divergence).   python profiles/aln_text_rate.py [--reads N] [--out FILE]"""
import argparse, json, os, subprocess, sys, tempfile, time
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=300); ap.add_argument("--threads", type=int, default=16); ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aln_text_rate.json"))
    args = ap.parse_args()
    import ctypes as C
    import numpy as np, mm2gb_amd as mm, align_cases as ac, aln_text_cases as tc, sim_reads
    if mm.device_count() < 1:
        raise SystemExit("aln_text_rate: no GPU visible (nothing is measured without one)")
    assert ac.ref_available(), "aln_text_rate: oracle/_ref is not built"
    tmp = tempfile.TemporaryDirectory()
    ref_fa, reads_fa = os.path.join(tmp.name, "ref.fa"), os.path.join(tmp.name, "reads.fa")
    bases = sim_reads.simulate(ref_fa, reads_fa, n_reads=args.reads, len_lo=5_000, len_hi=60_000)
    refs, reads = ac.read_fasta(ref_fa), ac.read_fasta(reads_fa)
    anchors = ac.own_anchors(refs, reads, "map-ont", threads=args.threads)
    ri = ac.RefIndex(refs, "map-ont")
    L = ac.ref_lib()
    L.mm_gen_cs_or_MD.restype = C.c_int
    L.mm_gen_cs_or_MD.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_int]
    prep = [ac.ref_prepare(ri, s, a, r) for r, (s, a) in enumerate(zip(reads, anchors))]
    b = dict(opt=ac.opt_from_ref(ri.mo), k=15, hpc=False, refs=refs, reads=reads, regs=[p[3] for p in prep], anchors=[p[4] for p in prep])
    for p in prep:
        if p[1]:
            ac._libc.free(p[0]); ac._libc.free(p[2])
    out = dict(reads=len(reads), bases=int(bases), threads=args.threads, runs=args.runs, preset="map-ont", reference="mm_gen_cs_or_MD, one record per call", rows={})
    with mm.Engine() as e:
        res, _ = ac.run_gpu(e, b)
        regs, read_of, aln, cigar = mm.flatten_aligned(res)
        have = np.flatnonzero(aln["cigar_off"] >= 0)
        out.update(records=int(len(have)), words=int(len(cigar)), columns=int((cigar >> 4).sum()))
        print(f"aln_text_rate: {len(reads)} reads, {bases} bases, {len(have)} records, {out['columns']} columns", file=sys.stderr, flush=True)
        # the reference's records, laid out once
        keep = []
        for i in have:
            w = np.ascontiguousarray(cigar[int(aln["cigar_off"][i]):int(aln["cigar_off"][i] + aln["n_cigar"][i])], np.uint32)
            extra = C.create_string_buffer(bytes(ac._Extra(len(w), 0, 0, 0, 0, len(w))) + w.tobytes())
            r1 = tc._Reg1(); C.memmove(r1.head, regs[i:i + 1].tobytes(), 72); r1.p = C.addressof(extra)
            keep.append((r1, extra, reads[int(read_of[i])]))

        def reference_leg(is_md, no_iden):
            def one(k):
                buf, cap = C.c_void_p(0), C.c_int(0)
                n = L.mm_gen_cs_or_MD(None, C.byref(buf), C.byref(cap), ri.mi, C.byref(keep[k][0]), keep[k][2], is_md, no_iden, 0)
                s = C.string_at(buf.value, n); ac._libc.free(buf)
                return s
            t = time.perf_counter()
            with ThreadPoolExecutor(args.threads) as ex:
                texts = list(ex.map(one, range(len(keep))))
            return time.perf_counter() - t, texts

        targs = (refs, reads, regs, read_of, aln, cigar)
        for name, what, ref_mode in (("cg", mm.TEXT_CG, None), ("cs", mm.TEXT_CS, (0, 1)), ("md", mm.TEXT_MD, (1, 0))):
            h_off, h_text = mm.aln_text_host(what, *targs, threads=args.threads)
            d_off, d_text = e.aln_text(what, *targs)
            assert d_text == h_text and np.array_equal(d_off, h_off), f"{name}: the device form differs from the host form"
            if ref_mode:
                _, texts = reference_leg(*ref_mode)
                got = tc.split(h_off, h_text)
                assert [got[i][6:] for i in have] == texts, f"{name}: the host form differs from the reference"
            row = dict(bytes=len(h_text), reference_s=[], host_s=[], device_s=[], device_without_residue_copies_s=[], device_prepare_on_host_s=[], device_kernels_and_words_s=[], device_text_back_s=[])
            for _ in range(args.runs):
                if ref_mode:
                    row["reference_s"].append(reference_leg(*ref_mode)[0])
                t = time.perf_counter(); mm.aln_text_host(what, *targs, threads=args.threads); row["host_s"].append(time.perf_counter() - t)
                t = time.perf_counter(); e.aln_text(what, *targs); dt = time.perf_counter() - t
                info = e.aln_text_info()
                row["device_s"].append(dt); row["device_without_residue_copies_s"].append(dt - info["s_upload"]); row["device_kernels_and_words_s"].append(info["s_kernels"])
                row["device_prepare_on_host_s"].append(info["s_prepare"]); row["device_text_back_s"].append(info["s_back"])
            row["device_faster_than_host_in_every_run"] = all(d < h for d, h in zip(row["device_s"], row["host_s"]))
            out["rows"][name] = row
            print(name, json.dumps({k: (min(v) if isinstance(v, list) and v else v) for k, v in row.items()}), file=sys.stderr, flush=True)
    ri.close()
    out["mapper"] = mapper_leg(args, ref_fa, reads_fa)
    tmp.cleanup()
    out["text_on_device_default"] = "device" if all(r["device_faster_than_host_in_every_run"] for r in out["rows"].values()) else "host"
    json.dump(out, open(args.out, "w"))
    print(json.dumps({k: out[k] for k in ("reads", "bases", "records", "columns", "text_on_device_default")}))


def mapper_leg(args, ref_fa, reads_fa):
    import mm2gb_amd as mm, orc
    from test_seeding_cpu import read_fasta
    refs, reads = read_fasta(ref_fa), read_fasta(reads_fa)
    exe = os.path.join(orc.REF_DIR, "minimap2_cpu")

    def reference():
        t = time.perf_counter()
        r = subprocess.run([exe, "-c", "-t", str(args.threads), "--max-chain-skip=2147483647", ref_fa, reads_fa], check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL)
        return time.perf_counter() - t, r.stdout.decode()

    leg = dict(reference="minimap2_cpu -c -t %d --max-chain-skip=2147483647, whole program (reads the files, builds its index)" % args.threads,
               mapper="map_reads(align=map_align(refs)): alignment on the device, text on host threads; index built before the clock starts",
               reference_s=[], mapper_s=[], stages=[])
    t = time.perf_counter()
    with mm.SeedIndex([s for _, s in refs], threads=args.threads) as ix, mm.Engine() as e:
        leg["mapper_index_s"] = time.perf_counter() - t
        al, opt, names = mm.map_align([s for _, s in refs]), mm.map_opt(host_threads=args.threads), [n for n, _ in refs]
        got, st = mm.map_reads(e, ix, names, reads, opt=opt, align=al)                       # warm-up of both, and the comparison
        _, want = reference()
        g, w = got.splitlines(), want.splitlines()
        leg.update(paf_lines=len(w), paf_lines_got=len(g), paf_lines_differing=sum(x != y for x, y in zip(g, w)) + abs(len(g) - len(w)), n_rmq_tied=st["n_rmq_tied"])
        for _ in range(args.runs):
            leg["reference_s"].append(reference()[0])
            t = time.perf_counter(); _, st = mm.map_reads(e, ix, names, reads, opt=opt, align=al); leg["mapper_s"].append(time.perf_counter() - t)
            leg["stages"].append({k: v for k, v in st.items() if k.startswith("s_")})
    print("mapper", json.dumps({k: leg[k] for k in ("reference_s", "mapper_s", "mapper_index_s", "paf_lines", "paf_lines_differing", "n_rmq_tied")}), file=sys.stderr, flush=True)
    print("mapper stages", json.dumps(leg["stages"][-1]), file=sys.stderr, flush=True)
    return leg


if __name__ == "__main__":
    main()
