#!/usr/bin/env python3
"""Spliced reads end to end: simulated spliced reads of 300-3 000 bases at 0-8 % error (tests/splice_cases.py: its genes in a genome
of about 5 Mbp) under the `splice` preset with max_sw_mat = 100 000 000 on both sides.  Legs, alternated in one process, `--runs` timed runs each
after a warm-up that also checks that all agree record for record and word for word (the mapper: line for line):
  reference  the reference's mm_align_skeleton through the test harness, one read per call on `--threads` threads; the records and anchors it
             consumes are made again, untimed, before every run;
  host       mm2gb_align_regs_splice_host on `--threads` threads;
  device     mm2gb_align_regs_splice_gpu, with seconds per stage (seconds[8]), DP jobs, cells, the share of jobs launched in the global-image
             class and the share of gap fills that ran a second pass;
  mapper     map_reads(..., opt=map_opt_splice(), align=map_splice(refs, cs="short")) against
             minimap2_cpu -t `--threads` --max-chain-skip=2147483647 -x splice --cap-sw-mem=100000000 -c --cs, as a program (it reads its files
             and builds its index inside the time; the mapper's index is built outside it and reported).
The yardsticks are the reference legs.   python profiles/splice_rate.py [--reads N] [--out FILE]"""
import argparse, json, os, subprocess, sys, tempfile, time
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2000); ap.add_argument("--threads", type=int, default=16); ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "splice_rate.json"))
    args = ap.parse_args()
    import ctypes as C
    import numpy as np, mm2gb_amd as mm, align_cases as ac, splice_cases as sc, orc, sim_reads
    if mm.device_count() < 1:
        raise SystemExit("splice_rate: no GPU visible (nothing is measured without one)")
    assert ac.ref_available(), "splice_rate: oracle/_ref is not built"
    refs, gs = sc.genes(seed=3, chr_lens=(2_000_000, 1_500_000, 1_500_000))
    rng = np.random.default_rng(5)
    reads = [bytes(np.asarray(sc.random_read(rng, refs, gs), np.uint8)) for _ in range(args.reads)]
    bases = sum(map(len, reads))
    t0 = time.perf_counter()
    anchors = sc.own_anchors(refs, reads, threads=args.threads)
    ri = sc.RefIndex(refs, "splice")
    L = ac.ref_lib()
    print(f"splice_rate: {len(reads)} reads, {bases} bases, genome {sum(map(len, refs))}, anchors in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)

    def prepare():
        return [sc.ref_prepare(ri, s, a, r) for r, (s, a) in enumerate(zip(reads, anchors))]

    def reference_leg(prep, collect):
        ns = [C.c_int(p[1]) for p in prep]
        outs = [None] * len(prep)
        def one(r):
            if prep[r][1]:
                outs[r] = L.mm_align_skeleton(None, C.byref(ri.mo), ri.mi, len(reads[r]), reads[r], C.byref(ns[r]), prep[r][0], prep[r][2])
        t = time.perf_counter()
        with ThreadPoolExecutor(args.threads) as ex:
            list(ex.map(one, range(len(prep))))
        dt = time.perf_counter() - t
        res = []
        for r, p in enumerate(prep):
            if not p[1]:
                res.append((np.zeros(0, mm.REG_DTYPE), np.zeros(0, mm.ALN_DTYPE), np.zeros(0, np.uint32)))
                continue
            rec, ps = ac._snap_regs(outs[r], ns[r].value)
            aln = np.zeros(ns[r].value, mm.ALN_DTYPE); words = []; total = 0
            for k, ptr in enumerate(ps):
                if not ptr:
                    aln[k]["cigar_off"] = -1
                    continue
                x = ac._Extra.from_address(ptr)
                aln[k] = (x.dp_score, x.dp_max, x.dp_max2, x.ambi_strand & 0x3fffffff, x.ambi_strand >> 30, x.n_cigar, total)
                if collect and x.n_cigar:
                    words.append(np.ctypeslib.as_array(C.cast(ptr + C.sizeof(ac._Extra), C.POINTER(C.c_uint32)), shape=(x.n_cigar,)).copy())
                total += x.n_cigar
                ac._libc.free(ptr)
            ac._libc.free(outs[r]); ac._libc.free(p[2])
            res.append((rec, aln, np.concatenate(words) if words else np.zeros(0, np.uint32)))
        return dt, res

    prep = prepare()
    b = dict(opt=sc.opt_from_ref(ri.mo), k=sc.K, hpc=False, refs=refs, reads=reads, regs=[p[3] for p in prep], anchors=[p[4] for p in prep])
    out = dict(reads=len(reads), bases=int(bases), genome=int(sum(map(len, refs))), threads=args.threads, runs=args.runs, preset="splice", max_sw_mat=sc.MAX_SW_MAT,
               reference="mm_align_skeleton, one read per call; minimap2_cpu as a program", records_in=int(sum(len(x) for x in b["regs"])),
               anchors=int(sum(len(x) for x in b["anchors"])), legs={})
    ref_names = [f"ref{i}" for i in range(len(refs))]
    named = [(f"read{i:05d}", s) for i, s in enumerate(reads)]
    exe = os.path.join(orc.REF_DIR, "minimap2_cpu")
    with mm.Engine() as e, tempfile.TemporaryDirectory() as d:
        ref_fa, read_fa = os.path.join(d, "ref.fa"), os.path.join(d, "reads.fa")
        sim_reads.write_fasta(ref_fa, [(n, np.frombuffer(s, np.uint8)) for n, s in zip(ref_names, refs)])
        sim_reads.write_fasta(read_fa, [(n, np.frombuffer(s, np.uint8)) for n, s in named])
        cmd = [exe, "-t", str(args.threads)] + sc.PAF_OPTIONS[2:] + ["-c", "--cs", ref_fa, read_fa]

        def program():
            t = time.perf_counter(); text = subprocess.run(cmd, check=True, capture_output=True).stdout.decode(); return time.perf_counter() - t, text

        t_ref, want = reference_leg(prep, True)
        t = time.perf_counter(); host, hinfo = sc.run_host(b, threads=args.threads); t_host = time.perf_counter() - t
        ac.assert_same(host, want, "host form against the reference")
        t = time.perf_counter(); dev, info = sc.run_gpu(e, b); t_dev = time.perf_counter() - t
        ac.assert_same(dev, want, "device form against the reference")
        t = time.perf_counter(); ix = mm.SeedIndex(refs, threads=args.threads, **mm.preset("splice")); t_index = time.perf_counter() - t
        al = mm.map_splice(refs, cs="short")
        t = time.perf_counter(); paf, st = mm.map_reads(e, ix, ref_names, named, opt=mm.map_opt_splice(host_threads=args.threads), k=sc.K, align=al); t_map = time.perf_counter() - t
        t_prog, paf_ref = program()
        differing = sum(x != y for x, y in zip(paf.splitlines(), paf_ref.splitlines())) + abs(len(paf.splitlines()) - len(paf_ref.splitlines()))
        out["agree"] = True
        out["mapper_paf"] = dict(lines=len(paf_ref.splitlines()), lines_differing=differing, ts_lines=paf_ref.count("\tts:A:"))
        out["warm_up_s"] = dict(reference=t_ref, host=t_host, device=t_dev, mapper=t_map, mapper_index=t_index, minimap2_cpu=t_prog)
        legs = dict(reference=[], host=[], device=[], mapper=[], minimap2_cpu=[])
        stages, map_stages = [], []
        for _ in range(args.runs):
            legs["reference"].append(reference_leg(prepare(), False)[0])
            t = time.perf_counter(); sc.run_host(b, threads=args.threads); legs["host"].append(time.perf_counter() - t)
            before = e.ksw_class_jobs()
            t = time.perf_counter(); _, info = sc.run_gpu(e, b); legs["device"].append(time.perf_counter() - t)
            after = e.ksw_class_jobs()
            stages.append(info["seconds"])
            t = time.perf_counter(); _, st = mm.map_reads(e, ix, ref_names, named, opt=mm.map_opt_splice(host_threads=args.threads), k=sc.K, align=al); legs["mapper"].append(time.perf_counter() - t)
            map_stages.append(st)
            legs["minimap2_cpu"].append(program()[0])
        ix.close() if hasattr(ix, "close") else None
        c, s = info["counts"], info["splice_counts"]
        launched = [after[0] - before[0], after[1] - before[1]]
        fills = c["fill_one_pass"] + c["fill_two_pass"]
        out["legs"] = legs
        out["device"] = dict(stages_s=stages, rounds=c["rounds"], jobs=c["jobs"], cells=c["cells"], cells_discarded=c["cells_discarded"],
                             launched_in_lds_image_class=launched[0], launched_in_global_image_class=launched[1], global_image_share=launched[1] / max(sum(launched), 1),
                             gap_fills_of_kept_trials=fills, second_pass_share=c["fill_two_pass"] / max(fills, 1), counts=c, splice_counts=s)
        out["mapper_stages_s"] = map_stages
        out["records_out"] = int(sum(len(w[0]) for w in want))
    ri.close()
    json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps({k: out[k] for k in ("reads", "bases", "legs", "warm_up_s", "mapper_paf")}))
    print(json.dumps({k: v for k, v in out["device"].items() if k not in ("counts", "splice_counts")}))


if __name__ == "__main__":
    main()
