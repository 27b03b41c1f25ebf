#!/usr/bin/env python3
"""Short single-end reads end to end: `--reads` simulated 150-base reads (1 % error, either strand) on a `--mbp` Mbp genome
(tests/sim_reads.make_genome: repeat families and tandem arrays), index at the sr preset's k = 21, w = 11 built outside the time:
  mapper        map_reads(..., opt=map_opt_sr(host_threads=T, ...), k=21, align=map_sr(...)) without and with base-level alignment (-c), seeded on host threads
                (seeding_on_device = 0) and on the device (1), and -- without alignment -- with the host's matches collected through the device (seeds_on_device = 1):
                wall seconds (best of `--repeat`), seconds per stage, and the call's own counts: reads whose anchors the host's heap ordered (n_tied_reads), rescued reads,
                chaining calls, fills left ungapped, fills run again, stretches shorter than their chain
  minimap2_cpu  oracle/_ref/minimap2_cpu -t T -x sr [-c] on the same files, as a program (it reads its files and builds its index inside the time); lines and reads that differ
What is measured is written down as it is, faster or slower.
   python profiles/sr_rate.py [--reads N] [--mbp N] [--threads N] [--out FILE]"""
import argparse, json, os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def per_read(text):
    d = {}
    for ln in text.splitlines():
        d.setdefault(ln.split("\t", 1)[0], []).append(ln)
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=200_000); ap.add_argument("--mbp", type=int, default=20); ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--repeat", type=int, default=3); ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sr_rate.json"))
    args = ap.parse_args()
    import numpy as np, mm2gb_amd as mm, orc, sim_reads
    if mm.device_count() < 1:
        raise SystemExit("sr_rate: no GPU visible (nothing is measured without one)")
    rng = np.random.default_rng(23)
    g = sim_reads.make_genome(rng, n_chr=1, chr_len=args.mbp * 1_000_000)[0]
    starts, flip = rng.integers(0, len(g) - 150, args.reads), rng.random(args.reads) < 0.5
    reads = []
    for r, (st, fl) in enumerate(zip(starts, flip)):
        s = sim_reads.mutate(rng, g[st:st + 150], 0.01)
        reads.append((f"read{r:07d}", bytes(sim_reads.revcomp(s) if fl else s)))
    out = dict(genome=len(g), reads=len(reads), read_len=150, error=0.01, k=21, w=11, threads=args.threads, legs={})
    print(f"sr_rate: genome {len(g)}, {len(reads)} reads", file=sys.stderr, flush=True)
    pafs = {}
    legs = (("chains.seed_host", False, dict(seeding_on_device=0, seeds_on_device=-1)), ("chains.seed_host.anchors_device", False, dict(seeding_on_device=0, seeds_on_device=1)),
            ("chains.seed_device", False, dict(seeding_on_device=1)), ("aligned.seed_host", True, dict(seeding_on_device=0, seeds_on_device=-1)),
            ("aligned.seed_device", True, dict(seeding_on_device=1)))
    with mm.Engine() as eng:
        t0 = time.perf_counter()
        ix = mm.SeedIndex([g.tobytes()], threads=args.threads, **mm.preset_sr())
        out["index_build_s"] = round(time.perf_counter() - t0, 3)
        for name, aligned, kw in legs:
            opt = mm.map_opt_sr(host_threads=args.threads, **kw)
            sr = mm.map_sr([g.tobytes()], align=True) if aligned else mm.map_sr()
            go = lambda: mm.map_reads(eng, ix, ["chr1"], reads, opt=opt, k=21, align=sr)
            go()                                                   # (the warm-up: arenas, first launches, fresh pages)
            best = None
            for _ in range(args.repeat):
                t0 = time.perf_counter()
                paf, st = go()
                dt = time.perf_counter() - t0
                best, best_st = (dt, st) if best is None or dt < best else (best, best_st)
            pafs[name] = paf
            out["legs"][name] = dict(seconds=round(best, 4), reads_per_s=round(len(reads) / best), lines=paf.count("\n"), stats=best_st)
            print(f"sr_rate: {name} {best:.3f} s", file=sys.stderr, flush=True)
    out["legs_equal"] = dict(chains=pafs["chains.seed_host"] == pafs["chains.seed_device"] == pafs["chains.seed_host.anchors_device"], aligned=pafs["aligned.seed_host"] == pafs["aligned.seed_device"])
    exe = os.path.join(orc.REF_DIR, "minimap2_cpu")
    if os.path.exists(exe):
        out["minimap2_cpu"] = {}
        with tempfile.TemporaryDirectory() as d:
            with open(os.path.join(d, "ref.fa"), "wb") as fh:
                fh.write(b">chr1\n" + g.tobytes() + b"\n")
            with open(os.path.join(d, "reads.fa"), "wb") as fh:
                for n, s in reads:
                    fh.write(b">" + n.encode() + b"\n" + s + b"\n")
            for name, extra, ours in (("chains", [], "chains.seed_host"), ("aligned", ["-c"], "aligned.seed_host")):
                t0 = time.perf_counter()
                r = subprocess.run([exe, "-t", str(args.threads), "-x", "sr"] + extra + [os.path.join(d, "ref.fa"), os.path.join(d, "reads.fa")], check=True, capture_output=True)
                dt = time.perf_counter() - t0
                want = r.stdout.decode()
                a, b = per_read(pafs[ours]), per_read(want)
                out["minimap2_cpu"][name] = dict(seconds_with_index_and_io=round(dt, 3), lines=want.count("\n"), our_lines=pafs[ours].count("\n"),
                                                 reads_with_different_lines=sum(1 for k in set(a) | set(b) if a.get(k) != b.get(k)))
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
