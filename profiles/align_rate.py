#!/usr/bin/env python3
"""The alignment of hits, three legs on one batch: reads of 5-80 kb at 8 % error from tests/sim_reads.simulate against its 3 Mbp genome,
map-ont.  Legs, alternated in one process, `--runs` timed runs each after a warm-up that also checks that all three agree record for record
and word for word:
  reference  the reference's mm_align_skeleton through tests/align_cases.py's harness, one read per call on `--threads` threads (ctypes
             releases the interpreter lock for the call); the records and anchors it consumes are made again, untimed, before every run;
  host       mm2gb_align_regs_host on `--threads` threads;
  device     mm2gb_align_regs_gpu, with seconds per stage, the number of rounds and the share of DP cells spent on discarded speculation.
The yardstick is the reference leg.   python profiles/align_rate.py [--reads N] [--out FILE]"""
import argparse, json, os, sys, tempfile, time
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2000); ap.add_argument("--threads", type=int, default=16); ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--skip-host", action="store_true", help="leave the host form's timed runs out (its warm-up run, which checks agreement, stays)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_rate.json"))
    args = ap.parse_args()
    import ctypes as C
    import numpy as np, mm2gb_amd as mm, align_cases as ac, sim_reads
    if mm.device_count() < 1:
        raise SystemExit("align_rate: no GPU visible (nothing is measured without one)")
    assert ac.ref_available(), "align_rate: oracle/_ref is not built"
    with tempfile.TemporaryDirectory() as d:
        bases = sim_reads.simulate(os.path.join(d, "ref.fa"), os.path.join(d, "reads.fa"), n_reads=args.reads)
        refs, reads = ac.read_fasta(os.path.join(d, "ref.fa")), ac.read_fasta(os.path.join(d, "reads.fa"))
    t0 = time.perf_counter()
    anchors = ac.own_anchors(refs, reads, "map-ont", threads=args.threads)
    ri = ac.RefIndex(refs, "map-ont")
    L = ac.ref_lib()
    print(f"align_rate: {len(reads)} reads, {bases} bases, anchors in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)

    def prepare():
        return [ac.ref_prepare(ri, s, a, r) for r, (s, a) in enumerate(zip(reads, anchors))]

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
        for r, p in enumerate(prep):          # what ref_align does after the call: snapshot (when asked) and free
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
    b = dict(opt=ac.opt_from_ref(ri.mo), k=15, hpc=False, refs=refs, reads=reads, regs=[p[3] for p in prep], anchors=[p[4] for p in prep])
    out = dict(reads=len(reads), bases=int(bases), threads=args.threads, runs=args.runs, preset="map-ont", reference="mm_align_skeleton, -DKSW_SSE2_ONLY -msse2, one read per call",
               records_in=int(sum(len(x) for x in b["regs"])), anchors=int(sum(len(x) for x in b["anchors"])), legs={})
    with mm.Engine() as e:
        t_ref, want = reference_leg(prep, True)
        t = time.perf_counter(); host, _ = ac.run_host(b, threads=args.threads); t_host = time.perf_counter() - t
        ac.assert_same(host, want, "host form against the reference")
        t = time.perf_counter(); dev, info = ac.run_gpu(e, b); t_dev = time.perf_counter() - t
        ac.assert_same(dev, want, "device form against the reference")
        out["agree"] = True
        out["warm_up_s"] = dict(reference=t_ref, host=t_host, device=t_dev)
        legs = dict(reference=[], host=[], device=[])
        stages = []
        for _ in range(args.runs):
            legs["reference"].append(reference_leg(prepare(), False)[0])
            if not args.skip_host:
                t = time.perf_counter(); ac.run_host(b, threads=args.threads); legs["host"].append(time.perf_counter() - t)
            t = time.perf_counter(); _, info = ac.run_gpu(e, b); legs["device"].append(time.perf_counter() - t)
            stages.append(info["seconds"])
        c = info["counts"]
        out["legs"] = legs
        out["device"] = dict(stages_s=stages, rounds=c["rounds"], jobs=c["jobs"], cells=c["cells"], cells_discarded=c["cells_discarded"],
                             discarded_share=c["cells_discarded"] / max(c["cells"], 1), counts=c)
        out["records_out"] = int(sum(len(w[0]) for w in want))
    ri.close()
    json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps({k: out[k] for k in ("reads", "bases", "legs", "warm_up_s")}))


if __name__ == "__main__":
    main()
