#!/usr/bin/env python3
"""Paired-end short reads end to end: `--pairs` simulated pairs of 2 x 150 bases (1 % error, insert 300-600, either mate first) on the `--mbp` Mbp genome of
profiles/sr_rate.py (the same generator and seed), index at the sr preset's k = 21, w = 11 built outside the time.  Two sets: "full" (every mate 150 bases before its
errors) and "trimmed" (every mate cut to a uniform random 100-150 bases, so the chaining calls per distinct (n_seg, max_dist_x, max_dist_y) show).  Per set:
  mapper        map_reads(..., opt=map_opt_sr(host_threads=T, seeding_on_device=0 / 1), k=21, align=map_sr(), frags=frag_offsets(names)): wall seconds (median of
                `--repeat` runs after a warm-up, and the fastest), seconds per stage, n_chain_calls, n_rescued
  minimap2_cpu  oracle/_ref/minimap2_cpu -t T -x sr on the same two files, as a program (it reads its files and builds its index inside the time); whether every line is equal
What is measured is written down as it is, faster or slower.
   python profiles/pe_rate.py [--pairs N] [--mbp N] [--threads N] [--repeat N] [--out FILE]"""
import argparse, json, os, statistics, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=100_000); ap.add_argument("--mbp", type=int, default=20); ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--repeat", type=int, default=5); ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pe_rate.json"))
    args = ap.parse_args()
    import numpy as np, mm2gb_amd as mm, orc, sim_reads
    if mm.device_count() < 1:
        raise SystemExit("pe_rate: no GPU visible (nothing is measured without one)")
    rng = np.random.default_rng(23)
    g = sim_reads.make_genome(rng, n_chr=1, chr_len=args.mbp * 1_000_000)[0]
    insert = rng.integers(300, 601, args.pairs)
    starts, flip = rng.integers(0, len(g) - 600, args.pairs), rng.random(args.pairs) < 0.5
    trim = rng.integers(100, 151, (args.pairs, 2))
    sets = {"full": [], "trimmed": []}
    for r, (st, ins, fl) in enumerate(zip(starts.tolist(), insert.tolist(), flip.tolist())):
        m1 = sim_reads.mutate(rng, g[st:st + 150], 0.01)
        m2 = sim_reads.revcomp(sim_reads.mutate(rng, g[st + ins - 150:st + ins], 0.01))
        if fl:
            m1, m2 = m2, m1
        sets["full"] += [(f"pair{r:07d}/1", bytes(m1)), (f"pair{r:07d}/2", bytes(m2))]
        sets["trimmed"] += [(f"pair{r:07d}/1", bytes(m1[:trim[r, 0]])), (f"pair{r:07d}/2", bytes(m2[:trim[r, 1]]))]
    out = dict(genome=len(g), pairs=args.pairs, mate_len=150, insert=[300, 600], error=0.01, k=21, w=11, threads=args.threads, repeat=args.repeat, sets={})
    print(f"pe_rate: genome {len(g)}, {args.pairs} pairs", file=sys.stderr, flush=True)
    exe = os.path.join(orc.REF_DIR, "minimap2_cpu")
    with mm.Engine() as eng:
        t0 = time.perf_counter()
        ix = mm.SeedIndex([g.tobytes()], threads=args.threads, **mm.preset_sr())
        out["index_build_s"] = round(time.perf_counter() - t0, 3)
        for name, reads in sets.items():
            frags = mm.frag_offsets([n for n, _ in reads])
            assert len(frags) == args.pairs + 1
            res, pafs = dict(distinct_summed_lengths=len({len(reads[2 * f][1]) + len(reads[2 * f + 1][1]) for f in range(args.pairs)}), legs={}), {}
            for leg, kw in (("seed_host", dict(seeding_on_device=0)), ("seed_device", dict(seeding_on_device=1))):
                opt = mm.map_opt_sr(host_threads=args.threads, **kw)
                go = lambda: mm.map_reads(eng, ix, ["chr1"], reads, opt=opt, k=21, align=mm.map_sr(), frags=frags)
                go()                                                   # (the warm-up: arenas, first launches, fresh pages)
                times = []
                for _ in range(args.repeat):
                    t0 = time.perf_counter()
                    paf, st = go()
                    times.append(time.perf_counter() - t0)
                pafs[leg] = paf
                med = statistics.median(times)
                res["legs"][leg] = dict(seconds_median=round(med, 4), seconds_min=round(min(times), 4), seconds_max=round(max(times), 4), pairs_per_s=round(args.pairs / med),
                                        lines=paf.count("\n"), n_chain_calls=st["n_chain_calls"], n_rescued=st["n_rescued"], stats=st)
                print(f"pe_rate: {name} {leg} median {med:.3f} s, {st['n_chain_calls']} chaining calls", file=sys.stderr, flush=True)
            res["legs_equal"] = pafs["seed_host"] == pafs["seed_device"]
            if os.path.exists(exe):
                with tempfile.TemporaryDirectory() as d:
                    with open(os.path.join(d, "ref.fa"), "wb") as fh:
                        fh.write(b">chr1\n" + g.tobytes() + b"\n")
                    for k in (0, 1):
                        with open(os.path.join(d, f"r{k + 1}.fa"), "wb") as fh:
                            for n, s in reads[k::2]:
                                fh.write(b">" + n.encode() + b"\n" + s + b"\n")
                    times = []
                    for _ in range(args.repeat + 1):                   # (the first run warms the page cache)
                        t0 = time.perf_counter()
                        r = subprocess.run([exe, "-t", str(args.threads), "-x", "sr", os.path.join(d, "ref.fa"), os.path.join(d, "r1.fa"), os.path.join(d, "r2.fa")], check=True, capture_output=True)
                        times.append(time.perf_counter() - t0)
                    want = r.stdout.decode()
                    res["minimap2_cpu"] = dict(seconds_with_index_and_io_median=round(statistics.median(times[1:]), 3), lines=want.count("\n"), every_line_equal=want == pafs["seed_host"])
            out["sets"][name] = res
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
