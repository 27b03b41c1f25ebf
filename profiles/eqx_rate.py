#!/usr/bin/env python3
"""The = / X rewrite on the records of a long-read batch: the records the device form of the alignment call gives for reads of 5-60 kb at
8 % error from tests/sim_reads.simulate against its 3 Mbp genome, map-ont (the batch of profiles/aln_text_rate.py).  Forms, alternated in one process,
`--runs` timed runs each after a warm-up that also checks that both give the same words:
  host     mm2gb_cigar_eqx_host on `--threads` threads;
  device   mm2gb_cigar_eqx_gpu: the whole call (residues up, the host's pass over the words, words up, kernels, new words back), and the same without
           the copies of the residues -- what the mapper pays when the alignment call left them resident.
The Python wrapper's own work (arrays in, arrays out) is inside every figure alike.  The yardstick for the mapper's default (eqx_on_device = 0) is the
host form: the device form takes over only if it is faster in every repeat.   python profiles/eqx_rate.py [--reads N] [--out FILE]"""
import argparse, json, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=300); ap.add_argument("--threads", type=int, default=16); ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eqx_rate.json"))
    args = ap.parse_args()
    import numpy as np, mm2gb_amd as mm, align_cases as ac, sim_reads
    if mm.device_count() < 1:
        raise SystemExit("eqx_rate: no GPU visible (nothing is measured without one)")
    assert ac.ref_available(), "eqx_rate: oracle/_ref is not built (the batch's records come from the reference's chaining)"
    tmp = tempfile.TemporaryDirectory()
    ref_fa, reads_fa = os.path.join(tmp.name, "ref.fa"), os.path.join(tmp.name, "reads.fa")
    bases = sim_reads.simulate(ref_fa, reads_fa, n_reads=args.reads, len_lo=5_000, len_hi=60_000)
    refs, reads = ac.read_fasta(ref_fa), ac.read_fasta(reads_fa)
    anchors = ac.own_anchors(refs, reads, "map-ont", threads=args.threads)
    ri = ac.RefIndex(refs, "map-ont")
    prep = [ac.ref_prepare(ri, s, a, r) for r, (s, a) in enumerate(zip(reads, anchors))]
    b = dict(opt=ac.opt_from_ref(ri.mo), k=15, hpc=False, refs=refs, reads=reads, regs=[p[3] for p in prep], anchors=[p[4] for p in prep])
    for p in prep:
        if p[1]:
            ac._libc.free(p[0]); ac._libc.free(p[2])
    ri.close()
    out = dict(reads=len(reads), bases=int(bases), threads=args.threads, runs=args.runs, preset="map-ont")
    with mm.Engine() as e:
        res, _ = ac.run_gpu(e, b)
        call = (refs, reads) + mm.flatten_aligned(res)
        cigar = call[5]
        host = mm.cigar_eqx_host(*call, threads=args.threads)
        dev = e.cigar_eqx(*call)                                      # warm-up, and the check
        assert np.array_equal(host[0], dev[0]) and np.array_equal(host[1], dev[1]), "host and device form differ"
        out.update(records=int((call[4]["cigar_off"] >= 0).sum()), words_in=int(len(cigar)), words_out=int(len(host[1])), columns=int((cigar >> 4).sum()))
        rows = dict(host_s=[], device_s=[], device_without_residue_copies_s=[], device_prepare_on_host_s=[], device_kernels_and_words_s=[], device_words_back_s=[])
        for _ in range(args.runs):
            t0 = time.perf_counter(); mm.cigar_eqx_host(*call, threads=args.threads); rows["host_s"].append(time.perf_counter() - t0)
            t0 = time.perf_counter(); e.cigar_eqx(*call); t = time.perf_counter() - t0
            info = e.cigar_eqx_info()
            rows["device_s"].append(t); rows["device_without_residue_copies_s"].append(t - info["s_upload"])
            rows["device_prepare_on_host_s"].append(info["s_prepare"]); rows["device_kernels_and_words_s"].append(info["s_kernels"]); rows["device_words_back_s"].append(info["s_back"])
    rows["device_resident_faster_than_host_in_every_run"] = all(d < h for d, h in zip(rows["device_without_residue_copies_s"], rows["host_s"]))
    rows["device_with_upload_faster_than_host_in_every_run"] = all(d < h for d, h in zip(rows["device_s"], rows["host_s"]))
    out["rows"] = rows
    out["eqx_on_device_default"] = "device" if rows["device_with_upload_faster_than_host_in_every_run"] else "host"
    json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
