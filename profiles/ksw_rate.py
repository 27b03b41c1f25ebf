#!/usr/bin/env python3
"""The extension DP, three forms on two batches from the read simulator (tests/sim_reads.py through tests/ksw_cases.py):
  (a) gap fills: global, APPROX_MAX, 200-2 000 bases a side, 10 % divergence, w 500;
  (b) end extensions: EXTZ_ONLY, zdrop 400, end_bonus -1, 1-5 kb a side, 10 % divergence, w 500;
both at the map-ont scores a=2 b=4 q=4 e=2 q2=24 e2=1.  Forms: the reference's ksw_extd2_sse (oracle/_ref, SSE2 build), one job per call
on `--threads` threads; the host form (mm2gb_ksw_extd2_host) on as many; the device form (mm2gb_ksw_extd2_gpu) with its copies, and its
kernels alone (events on the engine's stream).  The forms are alternated in one process, `--runs` timed runs each after one untimed warm-up
of each; the warm-up also checks that all three give the same records and words.  cells: the cells of the band over every anti-diagonal
of every job (a job that drops computes fewer).  --device-only: the device form alone, for a rocprofv3 --kernel-trace --stats run.
The measurement runs in a child process under a time limit of its own:   python profiles/ksw_rate.py [--jobs-a N] [--jobs-b N] [--out FILE]"""
import argparse, json, os, subprocess, sys, time
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def batches(args):
    import numpy as np, mm2gb_amd as mm, ksw_cases as kc
    rng = np.random.default_rng(42)
    a = [kc.make_pair(rng, 5, int(n), int(n), err=0.1, p_wild=0.0) for n in rng.integers(200, 2001, args.jobs_a)]
    b = [kc.make_pair(rng, 5, int(n), int(n), err=0.1, p_wild=0.0) for n in rng.integers(1000, 5001, args.jobs_b)]
    return {"gap_fill": mm.ksw_jobs(a, w=500, zdrop=-1, end_bonus=0, flag=mm.KSW_APPROX_MAX),
            "extension": mm.ksw_jobs(b, w=500, zdrop=400, end_bonus=-1, flag=mm.KSW_EXTZ_ONLY)}


def band_cells(jobs):
    import numpy as np
    total = 0
    for j in jobs:
        q, t, w = int(j["qlen"]), int(j["tlen"]), int(j["w"])
        r = np.arange(q + t - 1)
        st = np.maximum(np.maximum(0, r - q + 1), (r - w + 1) >> 1)
        en = np.minimum(np.minimum(t - 1, r), (r + w) >> 1)
        total += int(np.maximum(en - st + 1, 0).sum())
    return total


def reference(param, jobs, q, t, threads):
    """ksw_extd2_sse for every job, one call each, from `threads` threads (ctypes releases the interpreter lock for the call)."""
    import numpy as np, ksw_cases as kc
    cuts = np.linspace(0, len(jobs), threads * 8 + 1).astype(int)
    with ThreadPoolExecutor(threads) as ex:
        parts = list(ex.map(lambda k: kc.ref_batch(param, jobs[cuts[k]:cuts[k + 1]], q, t), range(len(cuts) - 1)))
    res = np.concatenate([p[0] for p in parts]); words = np.concatenate([p[1] for p in parts])
    res["cigar_off"] = np.concatenate([[0], np.cumsum(res["n_cigar"][:-1], dtype=np.int64)])
    return res, words


def measure(args):
    import mm2gb_amd as mm, ksw_cases as kc
    if mm.device_count() < 1:
        raise SystemExit("ksw_rate: no GPU visible (nothing is measured without one)")
    param = mm.ksw_param()
    out = {"threads": args.threads, "runs": args.runs, "scores": dict(a=2, b=4, q=4, e=2, q2=24, e2=1), "reference": "ksw_extd2_sse, -DKSW_SSE2_ONLY -msse2, one job per call", "batches": {}}
    have_ref = kc.ref_available() and not args.device_only
    t0 = time.perf_counter()
    sets = batches(args)
    print(f"ksw_rate: batches made in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
    with mm.Engine() as e:
        for name, (jobs, q, t) in sets.items():
            rec = {"jobs": len(jobs), "query_bases": int(jobs["qlen"].sum()), "target_bases": int(jobs["tlen"].sum()), "cells": band_cells(jobs), "flag": int(jobs["flag"][0]), "w": 500}
            forms = {"device": lambda: e.ksw_extd2_batch(param, jobs, q, t)}
            if not args.device_only:
                forms["host"] = lambda: mm.ksw_extd2_host_batch(param, jobs, q, t, threads=args.threads)
            if have_ref:
                forms["reference"] = lambda: reference(param, jobs, q, t, args.threads)
            warm = {k: f() for k, f in forms.items()}                       # untimed, and the forms must agree
            for k in warm:
                kc.assert_same(warm[k], warm["device"], f"{name}: {k} against device", jobs)
            rec["identical"] = sorted(warm)
            rec["shares"] = {k: round(float(v), 4) for k, v in kc.shares(warm["device"][0]).items()}
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
                print(f"ksw_rate: {name} run {run}: " + ", ".join(f"{k} {v[-1]} s" for k, v in secs.items()), file=sys.stderr, flush=True)
            rec["seconds"] = secs
            rec["pack_kernel_seconds"] = pack
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
        print(f"ksw_rate: the measurement ended with status {r.returncode}", file=sys.stderr)
        return r.returncode
    line = r.stdout.decode().strip().splitlines()[-1]
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(json.loads(line), indent=1) + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
