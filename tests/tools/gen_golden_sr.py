#!/usr/bin/env python3
"""Makes tests/golden/sr: seeds.npz (one JSON document, compressed) -- the genome and reads of tests/sr_cases.py (sim_set), the option set mm_set_opt gives for "sr", and
every read's anchors in the order collect_seed_hits_heap left them: the SD lines oracle/_ref/minimap2_cpu -t 1 -x sr --print-seeds writes to stderr (strand, both
positions, span), with the RS line's rep_len --, pafs.npz -- what the program prints for the runs of sr_cases.RUNS: -x sr, with -c, -c --cs and --cs=long --MD -c,
-f 4,50 (the max_occ rescue), -f 4,4 (no rescue: for comparison), --secondary=yes (for comparison) and --heap-sort=no -- and aln.npz: every read's records and kept
anchors as map.c has them when it calls align_regs, and what mm_align_skeleton of oracle/_ref/libminimap2ref.so made of them (records, mm_extra_t rows, CIGAR words).
Inputs and recorded output only.  Needs the reference built under oracle/_ref (make -C oracle ref, where the reference checkout exists).

The generator asserts what makes the fixture worth having -- (a) at least 3 reads in which two seeds share an index entry and at least half of all reads with none,
anchors of both strands in one read, a read without anchors, (b) at least 2 reads that get a line only through the rescue, (c) at least 2 fills that z-drop and split
their chain (the reads with a substituted middle), (d) a chain whose best stretch is shorter than the chain, (e) a reverse-strand line, (f) a read without a line, (g) a
read whose ONLY secondary hit MM_F_NO_PRINT_2ND suppresses (it has one S line with --secondary=yes), five read lengths -- and that this project's host forms already
reproduce the seed order and the alignment records (the mapper needs a device: tests/test_gpu_sr.py holds it to the PAFs)."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import align_cases as ac  # noqa: E402
import orc  # noqa: E402
import sr_cases as sc  # noqa: E402
import mm2gb_amd as mm  # noqa: E402

LIMIT = 142 * 1024          # no fixture larger than the largest of tests/golden/paf_aln


def main():
    assert ac.ref_available() and os.path.exists(os.path.join(orc.REF_DIR, "minimap2_cpu")), "build oracle/_ref first (make -C oracle ref)"
    genome, reads = sc.sim_set()
    assert len({n for n, _ in reads}) == len(reads)
    seeds = sc.record_seeds(genome, reads)
    assert set(seeds) == {n for n, _ in reads}
    options = sc.ref_options()
    doc = dict(seed=sc.SIM_SEED, genome=genome.decode(), reads=[[n, s.decode()] for n, s in reads], options=options, seeds=seeds,
               made_by="tests/tools/gen_golden_sr.py: minimap2_cpu -t 1 -x sr --print-seeds (SD lines); mm_set_opt(\"sr\")")
    os.makedirs(sc.GOLD, exist_ok=True)
    path = os.path.join(sc.GOLD, "seeds.npz")
    np.savez_compressed(path, doc=np.frombuffer(json.dumps(doc, sort_keys=True).encode("utf-8"), dtype=np.uint8))
    assert os.path.getsize(path) < LIMIT, f"{path} is {os.path.getsize(path)} bytes"
    # conditions on the fixture, then: the host form reproduces it
    sc._gold = None
    m = sc.matches([s for _, s in sc.reads()])
    n_shared = sum(sc.has_equal_cr(x) for x in m)
    assert n_shared >= 3 and n_shared * 2 <= len(m), f"{n_shared} of {len(m)} reads with two seeds on one index entry"
    assert any(len({r[0] for r in v["sd"]}) == 2 for v in seeds.values()), "no read with anchors of both strands"
    assert any(not v["sd"] for v in seeds.values()), "every read has anchors"
    assert sc.own_options()["map"] == options["map"] and sc.own_options()["index"] == options["index"], "mm2gb_map_opt_init_sr differs from mm_set_opt(\"sr\")"
    got, n_tied = mm.collect_seeds_heap_host(mm.map_opt_sr().flag, m)
    assert n_tied == n_shared
    bad = [n for (n, _), a, x in zip(reads, got, m) if sc.sd_rows(a) != seeds[n]["sd"] or x["rep_len"] != seeds[n]["rep_len"]]
    assert not bad, f"the host form differs from the recorded order for {bad}"
    # the mapper's runs (no base-level alignment) and what they must show
    pafs = {run: sc.record_paf(genome, reads, args) for run, (args, _, _) in sc.RUNS.items()}
    rows = {run: [ln.split("\t") for ln in text.splitlines()] for run, text in pafs.items()}
    rescued = {f[0] for f in rows["sr.f4_50"]} - {f[0] for f in rows["sr.f4_4"]}
    assert len(rescued) >= 2, f"-f 4,50: {len(rescued)} reads with no chain at mid_occ (no line at -f 4,4) and a line after the rescue"
    assert any(f[4] == "-" for f in rows["sr"]) and {n for n, _ in reads} - {f[0] for f in rows["sr"]}, "no reverse-strand line, or every read has a line"
    n_2nd = {}
    for f in rows["sr.2nd"]:
        if "tp:A:S" in f:
            n_2nd[f[0]] = n_2nd.get(f[0], 0) + 1
    only_2nd = {n for n, k in n_2nd.items() if k == 1}
    assert only_2nd and not any("tp:A:S" in f for run in ("sr",) + sc.ALIGNED for f in rows[run]), "no read whose only secondary hit MM_F_NO_PRINT_2ND suppresses"
    assert all(any(x.startswith("cg:Z:") for x in f) for run in sc.ALIGNED for f in rows[run]) and any(x.startswith("MD:Z:") for f in rows["sr.csmd"] for x in f)
    # the alignment records: mm_align_skeleton on this project's heap-order anchors, and the host form against them
    batch, want = sc.sr_ref_batch(genome, [s for _, s in reads])
    got, info = sc.run_sr_host(batch)
    ac.assert_same(got, want, "mm2gb_align_regs_sr_host against mm_align_skeleton")
    assert info["counts"]["split"] >= 2 and info["sr_counts"]["fill_rerun"] >= 2, f"(c) {info['counts']['split']} fills that z-drop and split"
    split_reads = [n for (n, _), (r, _, _) in zip(reads, want) if (r["flags"] & (1 << 8)).any()]
    assert sum(n.startswith("drop") for n in split_reads) >= 2, f"(c) the reads with a substituted middle do not split: {split_reads}"
    assert info["sr_counts"]["stretch_short"] >= 1, "(d) no chain whose stretch is shorter than the chain"
    apath = os.path.join(sc.GOLD, "aln.npz")
    sc.save_aligned(apath, batch, want)
    assert os.path.getsize(apath) < LIMIT, f"{apath} is {os.path.getsize(apath)} bytes"
    print(f"{apath}: {os.path.getsize(apath)} bytes; {info['sr_counts']}, split {info['counts']['split']}")
    assert len({f[1] for f in rows["sr"]}) >= 5, "fewer than five read lengths: several max_dist_x groups and the max_gap floor are wanted"
    ppath = os.path.join(sc.GOLD, "pafs.npz")
    np.savez_compressed(ppath, doc=np.frombuffer(json.dumps(pafs, sort_keys=True).encode("utf-8"), dtype=np.uint8))
    assert os.path.getsize(ppath) < LIMIT, f"{ppath} is {os.path.getsize(ppath)} bytes"
    print(f"{ppath}: {os.path.getsize(ppath)} bytes; lines " + ", ".join(f"{k} {len(v)}" for k, v in rows.items()) + f"; rescued {len(rescued)}; secondaries suppressed for {len(only_2nd)} reads")
    print(f"{path}: {os.path.getsize(path)} bytes, {len(reads)} reads, {sum(len(v['sd']) for v in seeds.values())} anchors, {n_shared} reads with shared index entries")


if __name__ == "__main__":
    main()
