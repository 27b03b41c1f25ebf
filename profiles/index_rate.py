#!/usr/bin/env python3
"""Index build and mid_occ, host form against device form (csrc/seeding.cpp: mm2gb_index_build at 16 threads, mm2gb_index_mid_occ;
csrc/index_kernels.hip: mm2gb_index_build_gpu, mm2gb_index_mid_occ_gpu) on sim_reads.make_genome genomes of three sizes.  Both forms run in
one process, alternated, `--runs` timed runs each after one untimed warm-up of each; the warm-up also checks that the two indexes are
identical.  For the host form the time until the index is usable on the device is reported too (build + mm2gb_index_to_device); the device
form's split (H2D, sketch, sort, tables, D2H) comes from events on the engine's streams (H2D overlaps the sketch).  --hpc: both forms
with homopolymer-compressed minimizers at k = 19, w = 10 (preset map-pb; the HPC form of csrc/seed_kernels.hip's sketch pipeline).
The measurement runs in a child process under a time limit of its own:   python profiles/index_rate.py [--mbp 10,100,1000] [--hpc] [--out FILE]"""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def genome(mbp, seed):
    import numpy as np, sim_reads
    n_chr = max(1, min(10, mbp // 10))
    chr_len = mbp * 1_000_000 // n_chr
    rng = np.random.default_rng(seed)
    t0 = time.perf_counter()
    seqs = [c.tobytes() for c in sim_reads.make_genome(rng, n_chr=n_chr, chr_len=chr_len, n_rep_families=6, rep_len=3000, copies=40 * n_chr, tandem=3)]
    return seqs, time.perf_counter() - t0


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, time.perf_counter() - t0


def measure(args):
    import numpy as np, mm2gb_amd as mm
    if mm.device_count() < 1:
        raise SystemExit("index_rate: no GPU visible (nothing is measured without one)")
    L = mm.lib()
    kw = mm.preset("map-pb") if args.hpc else {}
    out = {"host_threads": args.threads, "runs": args.runs, "hpc": bool(args.hpc), "k": kw.get("k", 15), "w": kw.get("w", 10), "chunk_bases": int(os.environ.get("MM2GB_INDEX_CHUNK_BASES", 256 << 20)), "sizes": []}
    with mm.Engine() as e:
        for mbp in args.mbp:
            seqs, t_gen = genome(mbp, 1000 + mbp)
            rec = {"mbp": mbp, "bases": sum(len(s) for s in seqs), "n_seq": len(seqs), "genome_seconds": round(t_gen, 2)}
            print(f"index_rate: {mbp} Mbp generated in {t_gen:.1f} s", file=sys.stderr, flush=True)
            # warm-up of each form, untimed; the two indexes must be the same index
            with mm.SeedIndex(seqs, threads=args.threads, **kw) as h, mm.SeedIndex(seqs, engine=e, **kw) as d:
                hv, dv, rv = h.view(), d.view(), d.fetch_device(e.device)
                rec["identical"] = bool(all(np.array_equal(hv[a], dv[a]) and np.array_equal(hv[a], rv[a]) for a in ("keys", "first", "where", "bucket"))
                                        and hv["bucket_shift"] == dv["bucket_shift"])
                rec.update(n_keys=hv["n_keys"], n_occ=hv["n_occ"], n_bucket=hv["n_bucket"])
                rec["mid_occ"] = h.mid_occ()
                rec["mid_occ_identical"] = bool(h.mid_occ() == d.mid_occ(engine=e) == h.mid_occ(engine=e))
                del hv, dv, rv
            rec.update(host_build_s=[], host_to_device_s=[], device_build_s=[], device_split_ms=[], mid_occ_host_s=[], mid_occ_device_s=[])
            for run in range(args.runs):
                h, t = timed(lambda: mm.SeedIndex(seqs, threads=args.threads, **kw))
                rec["host_build_s"].append(round(t, 4))
                rc, t = timed(lambda: L.mm2gb_index_to_device(h._h, e.device))
                assert rc == 0
                rec["host_to_device_s"].append(round(t, 4))
                _, t = timed(lambda: h.mid_occ())
                rec["mid_occ_host_s"].append(round(t, 5))
                h.close()
                d, t = timed(lambda: mm.SeedIndex(seqs, engine=e, **kw))
                rec["device_build_s"].append(round(t, 4))
                rec["device_split_ms"].append({k: round(v, 3) for k, v in d.build_split().items()})
                _, t = timed(lambda: d.mid_occ(engine=e))
                rec["mid_occ_device_s"].append(round(t, 5))
                d.close()
                print(f"index_rate: {mbp} Mbp run {run}: host {rec['host_build_s'][-1]} + {rec['host_to_device_s'][-1]} s, device {rec['device_build_s'][-1]} s", file=sys.stderr, flush=True)
            rec["host_usable_on_device_s"] = [round(a + b, 4) for a, b in zip(rec["host_build_s"], rec["host_to_device_s"])]
            out["sizes"].append(rec)
            del seqs
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbp", type=lambda s: [int(x) for x in s.split(",")], default=[10, 100, 1000])
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=1000, help="seconds the measuring child process may take")
    ap.add_argument("--hpc", action="store_true", help="homopolymer-compressed minimizers, k = 19, w = 10 (preset map-pb)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        print(json.dumps(measure(args)))
        return 0
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--worker", "--mbp", ",".join(map(str, args.mbp)),
           "--threads", str(args.threads), "--runs", str(args.runs)] + (["--hpc"] if args.hpc else [])
    r = subprocess.run(cmd, stdout=subprocess.PIPE)
    if r.returncode != 0:
        print(f"index_rate: the measurement ended with status {r.returncode}", file=sys.stderr)
        return r.returncode
    line = r.stdout.decode().strip().splitlines()[-1]
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(json.loads(line), indent=1) + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
