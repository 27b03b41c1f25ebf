#!/usr/bin/env python3
"""The single-affine extension DP on the two batches of profiles/ksw_rate.py at (q, e) = (4, 2):
  (a) gap fills: global, APPROX_MAX, 200-2 000 bases a side, 10 % divergence, w 500;
  (b) end extensions: EXTZ_ONLY, zdrop 400, end_bonus -1, 1-5 kb a side, 10 % divergence, w 500.
Forms: the reference's ksw_extz2_sse (oracle/_ref, SSE2 build), one job per call on `--threads` threads; the device's single-affine form
(mm2gb_ksw_extz2_gpu) with its copies and its kernels alone; and the device's DUAL-affine form (mm2gb_ksw_extd2_gpu) on the same jobs with
(4, 2, 24, 1), the form whose image has three more bytes a position.  The forms are alternated in one process, `--runs` timed runs each after
one untimed warm-up of each; the warm-up checks that the single-affine device form, the host form and the reference give the same records
and words (the dual-affine form computes another DP and is only timed).
The measurement runs in a child process under a time limit of its own:   python profiles/ksw_single_rate.py [--jobs-a N] [--jobs-b N] [--out FILE]"""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "profiles"))


def reference(param, jobs, q, t, threads):
    """ksw_extz2_sse for every job, one call each, from `threads` threads (ctypes releases the interpreter lock for the call)."""
    import numpy as np, ksw_single_cases as ks
    from concurrent.futures import ThreadPoolExecutor
    cuts = np.linspace(0, len(jobs), threads * 8 + 1).astype(int)
    with ThreadPoolExecutor(threads) as ex:
        parts = list(ex.map(lambda k: ks.ref_batch(param, jobs[cuts[k]:cuts[k + 1]], q, t), range(len(cuts) - 1)))
    res = np.concatenate([p[0] for p in parts]); words = np.concatenate([p[1] for p in parts])
    res["cigar_off"] = np.concatenate([[0], np.cumsum(res["n_cigar"][:-1], dtype=np.int64)])
    return res, words


def measure(args):
    import mm2gb_amd as mm, ksw_cases as kc, ksw_single_cases as ks, ksw_rate
    if mm.device_count() < 1:
        raise SystemExit("ksw_single_rate: no GPU visible (nothing is measured without one)")
    single, dual = ks.param(4, 2), mm.ksw_param()
    out = {"threads": args.threads, "runs": args.runs, "scores": dict(a=2, b=4, q=4, e=2), "dual_scores": dict(a=2, b=4, q=4, e=2, q2=24, e2=1),
           "reference": "ksw_extz2_sse, -DKSW_SSE2_ONLY -msse2, one job per call", "batches": {}}
    have_ref = kc.ref_available()
    sets = ksw_rate.batches(args)
    with mm.Engine() as e:
        for name, (jobs, q, t) in sets.items():
            rec = {"jobs": len(jobs), "cells": ksw_rate.band_cells(jobs), "flag": int(jobs["flag"][0]), "w": 500}
            forms = {"single": lambda: e.ksw_extz2_batch(single, jobs, q, t), "dual": lambda: e.ksw_extd2_batch(dual, jobs, q, t)}
            if have_ref:
                forms["reference"] = lambda: reference(single, jobs, q, t, args.threads)
            warm = {k: f() for k, f in forms.items()}
            kc.assert_same(warm["single"], mm.ksw_extz2_host_batch(single, jobs, q, t, threads=args.threads), f"{name}: device against host", jobs)
            if have_ref:
                kc.assert_same(warm["single"], warm["reference"], f"{name}: device against the reference", jobs)
            rec["identical"] = ["single", "host"] + (["reference"] if have_ref else [])
            rec["shares"] = {k: round(float(v), 4) for k, v in kc.shares(warm["single"][0]).items()}
            before = e.ksw_class_jobs()
            e.ksw_extz2_batch(single, jobs, q, t); mid = e.ksw_class_jobs()
            e.ksw_extd2_batch(dual, jobs, q, t); after = e.ksw_class_jobs()
            rec["jobs_with_image_in_global_memory"] = {"single": mid[1] - before[1], "dual": after[1] - mid[1]}
            del warm
            secs = {k: [] for k in forms}
            secs["single_kernels"] = []; secs["dual_kernels"] = []
            for run in range(args.runs):
                for k, f in forms.items():
                    t0 = time.perf_counter(); f(); secs[k].append(round(time.perf_counter() - t0, 4))
                    if k != "reference":
                        info = e.ksw_info()
                        secs[k + "_kernels"].append(round((info["ms_fill"] + info["ms_pack"]) / 1e3, 4))
                print(f"ksw_single_rate: {name} run {run}: " + ", ".join(f"{k} {v[-1]} s" for k, v in secs.items()), file=sys.stderr, flush=True)
            rec["seconds"] = secs
            rec["gcells_per_s"] = {k: round(rec["cells"] / min(v) / 1e9, 3) for k, v in secs.items() if v}
            out["batches"][name] = rec
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs-a", type=int, default=50000)
    ap.add_argument("--jobs-b", type=int, default=5000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=1000, help="seconds the measuring child process may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        print(json.dumps(measure(args)))
        return 0
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--worker", "--jobs-a", str(args.jobs_a), "--jobs-b", str(args.jobs_b),
           "--threads", str(args.threads), "--runs", str(args.runs)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE)
    if r.returncode != 0:
        print(f"ksw_single_rate: the measurement ended with status {r.returncode}", file=sys.stderr)
        return r.returncode
    line = r.stdout.decode().strip().splitlines()[-1]
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(json.loads(line), indent=1) + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
