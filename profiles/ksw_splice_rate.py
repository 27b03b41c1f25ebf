#!/usr/bin/env python3
"""The splice-aware DP, three forms on two batches from the read simulator (tests/sim_reads.py through tests/ksw_splice_cases.py):
  (a) gap fills across introns: global, APPROX_MAX | SPLICE_FOR, two-exon queries of 200-600 bases against targets of 1-50 kb with one
      planted GTr..yAG intron, 5 % divergence, half of them with the junction annotated in junc;
  (b) end extensions: EXTZ_ONLY | SPLICE_FOR, zdrop 200, 300-1 500 bases a side, 10 % divergence;
both at the `splice` preset's numbers a=1 b=2 q=2 e=1 q2=32 noncan=9 junc_bonus=9.  Forms: the reference's ksw_exts2_sse (oracle/_ref, SSE2
build), one job per call on `--threads` threads; the host form (mm2gb_ksw_exts2_host) on as many; the device form (mm2gb_ksw_exts2_gpu) with
its copies, and its kernels alone (events on the engine's stream).  The forms are alternated in one process, `--runs` timed runs each after
one untimed warm-up of each; the warm-up also checks that all three give the same records and words.  cells: qlen * tlen of every job (there
is no band; a job that drops computes fewer).  --device-only: the device form alone, for a rocprofv3 --kernel-trace --stats run.
The measurement runs in a child process under a time limit of its own:   python profiles/ksw_splice_rate.py [--jobs-a N] [--jobs-b N] [--out FILE]"""
import argparse, json, os, subprocess, sys, time
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def batches(args):
    import numpy as np, mm2gb_amd as mm, ksw_cases as kc, ksw_splice_cases as sc
    rng = np.random.default_rng(43)
    a = []
    for _ in range(args.jobs_a):
        n, tlen = int(rng.integers(200, 601)), int(rng.integers(1000, 50001))
        q, t, junc = sc.make_intron_pair(rng, 5, n // 2, n - n // 2, tlen - n, sc.MOTIFS[1], 0.05, p_wild=0.0)
        a.append((q, t, dict(junc=junc)))
    b = [kc.make_pair(rng, 5, int(n), int(n), err=0.1, p_wild=0.0) for n in rng.integers(300, 1501, args.jobs_b)]
    return {"intron_gap_fill": mm.ksw_splice_jobs(a, zdrop=-1, flag=mm.KSW_APPROX_MAX | mm.KSW_SPLICE_FOR),
            "extension": mm.ksw_splice_jobs(b, zdrop=200, flag=mm.KSW_EXTZ_ONLY | mm.KSW_SPLICE_FOR)}


def reference(param, jobs, q, t, junc, threads):
    """ksw_exts2_sse for every job, one call each, from `threads` threads (ctypes releases the interpreter lock for the call)."""
    import numpy as np, ksw_splice_cases as sc
    cuts = np.linspace(0, len(jobs), threads * 8 + 1).astype(int)
    with ThreadPoolExecutor(threads) as ex:
        parts = list(ex.map(lambda k: sc.ref_batch(param, jobs[cuts[k]:cuts[k + 1]], q, t, junc), range(len(cuts) - 1)))
    res = np.concatenate([p[0] for p in parts]); words = np.concatenate([p[1] for p in parts])
    res["cigar_off"] = np.concatenate([[0], np.cumsum(res["n_cigar"][:-1], dtype=np.int64)])
    return res, words


def measure(args):
    import mm2gb_amd as mm, ksw_cases as kc, ksw_splice_cases as sc
    if mm.device_count() < 1:
        raise SystemExit("ksw_splice_rate: no GPU visible (nothing is measured without one)")
    param = mm.ksw_splice_param()
    out = {"threads": args.threads, "runs": args.runs, "scores": dict(a=1, b=2, q=2, e=1, q2=32, noncan=9, junc_bonus=9), "reference": "ksw_exts2_sse, -DKSW_SSE2_ONLY -msse2, one job per call", "batches": {}}
    have_ref = kc.ref_available() and not args.device_only
    t0 = time.perf_counter()
    sets = batches(args)
    print(f"ksw_splice_rate: batches made in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
    with mm.Engine() as e:
        for name, (jobs, q, t, junc) in sets.items():
            rec = {"jobs": len(jobs), "query_bases": int(jobs["qlen"].sum()), "target_bases": int(jobs["tlen"].sum()), "cells": int((jobs["qlen"].astype("int64") * jobs["tlen"]).sum()), "flag": int(jobs["flag"][0]), "with_junc": junc is not None}
            forms = {"device": lambda: e.ksw_exts2_batch(param, jobs, q, t, junc)}
            if not args.device_only:
                forms["host"] = lambda: mm.ksw_exts2_host_batch(param, jobs, q, t, junc, threads=args.threads)
            if have_ref:
                forms["reference"] = lambda: reference(param, jobs, q, t, junc, args.threads)
            warm = {k: f() for k, f in forms.items()}                       # untimed, and the forms must agree
            for k in warm:
                kc.assert_same(warm[k], warm["device"], f"{name}: {k} against device", jobs)
            rec["identical"] = sorted(warm)
            rec["shares"] = {k: round(float(v), 4) for k, v in kc.shares(warm["device"][0]).items()}
            rec["jobs_with_N"] = int(sc.has_N(*warm["device"]).sum())
            rec["cigar_words"] = int(len(warm["device"][1]))
            del warm
            secs = {k: [] for k in forms}
            secs["device_kernels"] = []; pack = []
            for run in range(args.runs):
                for k, f in forms.items():
                    t0 = time.perf_counter(); f(); secs[k].append(round(time.perf_counter() - t0, 4))
                    if k == "device":
                        info = e.ksw_info()
                        secs["device_kernels"].append(round((info["ms_fill"] + info["ms_pack"]) / 1e3, 4)); pack.append(round(info["ms_pack"] / 1e3, 5))
                print(f"ksw_splice_rate: {name} run {run}: " + ", ".join(f"{k} {v[-1]} s" for k, v in secs.items()), file=sys.stderr, flush=True)
            rec["seconds"] = secs
            rec["pack_kernel_seconds"] = pack
            rec["gcells_per_s"] = {k: round(rec["cells"] / min(v) / 1e9, 3) for k, v in secs.items() if v}
            out["batches"][name] = rec
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs-a", type=int, default=20000)
    ap.add_argument("--jobs-b", type=int, default=5000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=1000, help="seconds the measuring child process may take")
    ap.add_argument("--device-only", action="store_true", help="the device form alone (for a kernel trace)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        print(json.dumps(measure(args)))
        return 0
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--worker", "--jobs-a", str(args.jobs_a), "--jobs-b", str(args.jobs_b),
           "--threads", str(args.threads), "--runs", str(args.runs)] + (["--device-only"] if args.device_only else [])
    r = subprocess.run(cmd, stdout=subprocess.PIPE)
    if r.returncode != 0:
        print(f"ksw_splice_rate: the measurement ended with status {r.returncode}", file=sys.stderr)
        return r.returncode
    line = r.stdout.decode().strip().splitlines()[-1]
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(json.loads(line), indent=1) + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
