#!/usr/bin/env python3
"""Read-against-read overlap end to end: a simulated read set of `--mbp` Mbp of 5-30 kb reads at about `--depth`x over one genome
(tests/sim_reads.make_genome: repeats and tandem arrays; 8 % error, either strand), every read against every read with the ava-ont preset:
  staged        map_reads_stream(..., opt=map_opt_ava("ava-ont", max_chain_skip=S, seeding_on_device=1)) on one engine, in chunks of `--chunk-mbp` Mbp
  resident      the same with seeding_on_device=2: anchors, chains and kept anchors stay on the device
  minimap2_cpu  oracle/_ref/minimap2_cpu -t `--threads` -x ava-ont on the same file, as a program (it reads its file and builds its index inside the time)
each at S = 25 and S = infinity.  Per leg: wall seconds, seconds per stage (summed over chunks), the bytes the stages copied to the device and back and which
path each chunk took (the mapper's MM2GB_DEBUG_PHASES lines), and whether the PAFs are equal.  The index is built outside the time and reported.
A run can be cut into calls: --legs and --skips select, and the results are merged into --out.
   python profiles/ava_rate.py [--mbp N] [--depth N] [--legs staged,resident,ref] [--skips 25,inf] [--out FILE]"""
import argparse, hashlib, json, os, re, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
INF = 2**31 - 1


def with_phase_lines(run):
    """run() with MM2GB_DEBUG_PHASES set and the library's stderr in a file: the mapper's `map path` lines."""
    with tempfile.TemporaryFile() as f:
        keep = os.dup(2)
        os.environ["MM2GB_DEBUG_PHASES"] = "1"
        try:
            os.dup2(f.fileno(), 2)
            run()
        finally:
            os.dup2(keep, 2); os.close(keep); del os.environ["MM2GB_DEBUG_PHASES"]
        f.seek(0); text = f.read().decode(errors="replace")
    rows = re.findall(r"map path: (resident|staged)[^;]*; (\d+) anchors, (\d+) chains; copied to the device (\d+) B, back (\d+) B", text)
    return dict(chunks=len(rows), chunks_resident=sum(r[0] == "resident" for r in rows), anchors=sum(int(r[1]) for r in rows), chains=sum(int(r[2]) for r in rows),
                bytes_to_device=sum(int(r[3]) for r in rows), bytes_back=sum(int(r[4]) for r in rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbp", type=int, default=100); ap.add_argument("--depth", type=int, default=30); ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--chunk-mbp", type=int, default=8); ap.add_argument("--legs", default="staged,resident,ref"); ap.add_argument("--skips", default="25,inf")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ava_rate.json"))
    args = ap.parse_args()
    import numpy as np, mm2gb_amd as mm, orc, sim_reads
    legs, skips = args.legs.split(","), args.skips.split(",")
    if mm.device_count() < 1 and legs != ["ref"]:
        raise SystemExit("ava_rate: no GPU visible (nothing is measured without one)")
    exe = os.path.join(orc.REF_DIR, "minimap2_cpu")
    rng = np.random.default_rng(17)
    g = sim_reads.make_genome(rng, n_chr=1, chr_len=args.mbp * 1_000_000 // args.depth)[0]
    reads, total = [], 0
    while total < args.mbp * 1_000_000:
        L = int(rng.integers(5_000, 30_000)); st = int(rng.integers(0, len(g) - L))
        s = sim_reads.mutate(rng, g[st:st + L].copy(), 0.08)
        reads.append((f"read{len(reads):06d}", bytes(sim_reads.revcomp(s) if rng.random() < 0.5 else s)))
        total += len(reads[-1][1])
    names, seqs = [n for n, _ in reads], [s for _, s in reads]
    out = json.load(open(args.out)) if os.path.exists(args.out) else {}
    head = dict(genome=len(g), reads=len(reads), bases=total, depth=args.depth, error=0.08, preset="ava-ont", threads=args.threads, chunk_bases=args.chunk_mbp * 1_000_000)
    if {k: out.get(k) for k in head} != head:
        out = dict(head, skips={})
    print(f"ava_rate: genome {len(g)}, {len(reads)} reads, {total} bases", file=sys.stderr, flush=True)
    md5 = lambda text: hashlib.md5(text.encode()).hexdigest()
    with tempfile.TemporaryDirectory() as d:
        fa = os.path.join(d, "reads.fa")
        sim_reads.write_fasta(fa, [(n, np.frombuffer(s, np.uint8)) for n, s in reads])
        if legs != ["ref"]:
            e = mm.Engine()
            t = time.perf_counter(); ix = mm.SeedIndex(seqs, threads=args.threads, **mm.preset_ava("ava-ont")); out["mapper_index_s"] = time.perf_counter() - t
        for tag in skips:
            skip = INF if tag == "inf" else int(tag)
            leg_out = out["skips"].setdefault(tag, {})
            for leg in legs:
                if leg == "ref":
                    assert os.path.exists(exe), "ava_rate: oracle/_ref is not built"
                    cmd = [exe, "-t", str(args.threads), "-x", "ava-ont", f"--max-chain-skip={skip}", fa, fa]
                    t = time.perf_counter(); want = subprocess.run(cmd, check=True, capture_output=True).stdout.decode(); t_ref = time.perf_counter() - t
                    leg_out["minimap2_cpu"] = dict(wall_s=t_ref, lines=len(want.splitlines()), paf_md5=md5(want))
                else:
                    opt = mm.map_opt_ava("ava-ont", max_chain_skip=skip, host_threads=args.threads, seeding_on_device=2 if leg == "resident" else 1)
                    mm.map_reads(e, ix, names, reads[:50], opt=opt, k=15)          # warm-up
                    got = []
                    def run():
                        t = time.perf_counter(); got.append(mm.map_reads_stream([e], ix, names, reads, opt=opt, k=15, chunk_bases=args.chunk_mbp * 1_000_000)); got.append(time.perf_counter() - t)
                    link = with_phase_lines(run)
                    (paf, st), t_map = got
                    leg_out[leg] = dict(wall_s=t_map, stages_s={k: v for k, v in st.items() if k.startswith("s_")}, counts={k: v for k, v in st.items() if k.startswith("n_")},
                                        link=link, lines=len(paf.splitlines()), paf_md5=md5(paf))
                print(f"ava_rate: skip {tag} {leg}: {json.dumps(leg_out['minimap2_cpu' if leg == 'ref' else leg])}", file=sys.stderr, flush=True)
                have = {k: v["paf_md5"] for k, v in leg_out.items() if isinstance(v, dict) and "paf_md5" in v}
                leg_out["pafs_equal"] = {"legs": sorted(have), "equal": len(set(have.values())) == 1}
                json.dump(out, open(args.out, "w"), indent=1)          # (after every leg: a later one may be cut off)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
