#!/usr/bin/env python3
"""Assembly-to-reference mapping end to end (MM_F_RMQ): a simulated genome of `--genome-mbp` Mbp (tests/sim_reads.make_genome: repeats and
tandem arrays) and `--contigs` contigs of 0.2-1 Mbp cut from it at 1 % divergence, either strand, mapped with the asm5 preset:
  mapper        map_reads(..., opt=map_opt_preset("asm5", max_chain_skip=S), align=map_align(refs, preset="asm5")), the index built outside the time
                and reported, for S = 25 (the reference's default) and S = infinity; wall seconds, seconds per stage, and how many contigs met a
                deciding tie on the device and were redone by the host form, in the first chaining stage and in the re-chaining stage (read from
                the mapper's MM2GB_DEBUG_PHASES lines of the timed run, after a warm-up on two contigs);
  minimap2_cpu  oracle/_ref/minimap2_cpu -t `--threads` -x asm5 -c on the same files, as a program (it reads its files and builds its index inside
                the time), at the same two skip values.
The PAFs are compared line for line.   python profiles/asm_rate.py [--genome-mbp N] [--contigs N] [--out FILE]"""
import argparse, json, os, re, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
INF = 2**31 - 1


def tie_counts(run):
    """run() with MM2GB_DEBUG_PHASES set and the library's stderr in a file: (reads, tied) of the first chaining stage and of the re-chaining stage."""
    with tempfile.TemporaryFile() as f:
        keep = os.dup(2)
        os.environ["MM2GB_DEBUG_PHASES"] = "1"
        try:
            os.dup2(f.fileno(), 2)
            run()
        finally:
            os.dup2(keep, 2); os.close(keep); del os.environ["MM2GB_DEBUG_PHASES"]
        f.seek(0); text = f.read().decode(errors="replace")
    first = re.search(r"first chaining \(MM_F_RMQ\) (\d+) reads \((\d+) redone", text)
    again = re.search(r"re-chaining (\d+) reads \((\d+) redone", text)
    n1, t1 = (int(first.group(1)), int(first.group(2))) if first else (0, 0)
    n2, t2 = (int(again.group(1)), int(again.group(2))) if again else (0, 0)
    deals = [ln.strip() for ln in text.splitlines() if " deal: " in ln]
    return dict(first_chaining=dict(reads=n1, tied=t1), re_chaining=dict(reads=n2, tied=t2), deals=deals)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-mbp", type=int, default=20); ap.add_argument("--contigs", type=int, default=40); ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "asm_rate.json"))
    args = ap.parse_args()
    import numpy as np, mm2gb_amd as mm, orc, sim_reads
    if mm.device_count() < 1:
        raise SystemExit("asm_rate: no GPU visible (nothing is measured without one)")
    exe = os.path.join(orc.REF_DIR, "minimap2_cpu")
    assert os.path.exists(exe), "asm_rate: oracle/_ref is not built"
    rng = np.random.default_rng(7)
    n_chr = 4
    chrs = sim_reads.make_genome(rng, n_chr=n_chr, chr_len=args.genome_mbp * 1_000_000 // n_chr)
    contigs = []
    for i in range(args.contigs):
        c = int(rng.integers(0, n_chr)); L = int(rng.integers(200_000, 1_000_000)); st = int(rng.integers(0, len(chrs[c]) - L))
        s = sim_reads.mutate(rng, chrs[c][st:st + L].copy(), 0.01)
        contigs.append((f"ctg{i:02d}_chr{c + 1}_{st}_{L}", bytes(sim_reads.revcomp(s) if rng.random() < 0.5 else s)))
    refs = [(f"chr{k + 1}", bytes(c)) for k, c in enumerate(chrs)]
    names, seqs = [n for n, _ in refs], [s for _, s in refs]
    out = dict(genome=int(sum(map(len, seqs))), contigs=len(contigs), bases=int(sum(len(s) for _, s in contigs)), divergence=0.01, preset="asm5", threads=args.threads, skips={})
    print(f"asm_rate: genome {out['genome']}, {out['contigs']} contigs, {out['bases']} bases", file=sys.stderr, flush=True)
    with mm.Engine() as e, tempfile.TemporaryDirectory() as d:
        ref_fa, q_fa = os.path.join(d, "ref.fa"), os.path.join(d, "contigs.fa")
        sim_reads.write_fasta(ref_fa, [(n, np.frombuffer(s, np.uint8)) for n, s in refs])
        sim_reads.write_fasta(q_fa, [(n, np.frombuffer(s, np.uint8)) for n, s in contigs])
        t = time.perf_counter(); ix = mm.SeedIndex(seqs, threads=args.threads, **mm.preset("asm5")); out["mapper_index_s"] = time.perf_counter() - t
        al = mm.map_align(seqs, preset="asm5")
        for tag, skip in (("25", 25), ("inf", INF)):
            opt = mm.map_opt_preset("asm5", max_chain_skip=skip, host_threads=args.threads)
            mm.map_reads(e, ix, names, contigs[:2], opt=opt, k=19, align=al)          # warm-up: two contigs
            got = []
            def run():
                t = time.perf_counter(); got.append(mm.map_reads(e, ix, names, contigs, opt=opt, k=19, align=al)); got.append(time.perf_counter() - t)
            ties = tie_counts(run)                                  # (the mapper's own MM2GB_DEBUG_PHASES lines are two fprintf per stage: they stay in the timed run)
            (paf, st), t_map = got
            out["skips"][tag] = dict(mapper_s=t_map, stages_s={k: v for k, v in st.items() if k.startswith("s_")}, counts={k: v for k, v in st.items() if k.startswith("n_")}, ties=ties)
            json.dump(out, open(args.out, "w"), indent=1)          # (before the reference's run as well: a later step may be cut off)
            print(f"asm_rate: skip {tag}: mapper {t_map:.2f} s, ties {ties['first_chaining']} / {ties['re_chaining']}", file=sys.stderr, flush=True)
            cmd = [exe, "-t", str(args.threads), "-x", "asm5", "-c"] + (["--max-chain-skip=2147483647"] if skip == INF else []) + [ref_fa, q_fa]
            t = time.perf_counter(); want = subprocess.run(cmd, check=True, capture_output=True).stdout.decode(); t_ref = time.perf_counter() - t
            g, w = paf.splitlines(), want.splitlines()
            out["skips"][tag].update(minimap2_cpu_s=t_ref, paf=dict(lines=len(w), lines_differing=sum(x != y for x, y in zip(g, w)) + abs(len(g) - len(w))))
            print(f"asm_rate: skip {tag}: mapper {t_map:.2f} s, minimap2_cpu {t_ref:.2f} s, {out['skips'][tag]['paf']}", file=sys.stderr, flush=True)
            json.dump(out, open(args.out, "w"), indent=1)          # (after every leg: a later one may be cut off)
        ix.close() if hasattr(ix, "close") else None
    print(json.dumps(out))


if __name__ == "__main__":
    main()
