#!/usr/bin/env python3
"""Makes tests/golden/pe: pe.npz (one JSON document, compressed) -- the two contigs and the pairs of tests/pe_cases.py (sim_set), the option set mm_set_opt gives for "sr"
with what main.c makes of max_chain_skip, what oracle/_ref/minimap2_cpu -t 1 prints for the runs of pe_cases.RUNS (-x sr; -f 4,50 and -f 4,4; --secondary=yes;
--heap-sort=no) on the interleaved file, the same reads mapped as two single-end files ("se": mate 1's lines, then mate 2's; for comparison only) and every fragment's anchors
and rep_len from the SD / RS lines of --print-seeds -- and post.npz: per two-mate fragment the records before and after mm_select_sub_multi and what mm_seg_gen of
oracle/_ref/libminimap2ref.so made of them.  Inputs and recorded output only.  Needs the reference built under oracle/_ref (make -C oracle ref).

The generator asserts what makes the set worth having (pe_cases.worth_having: a mate whose line differs from its single-end line in target or mapq, -f 4,50 differs from
-f 4,4, a line with cm:i:1, a mate with two tp:A:P lines, tp:A:S lines with --secondary=yes), that the interleaved file and the two files give the same bytes, at least four
distinct summed lengths, and that this project's host forms already reproduce the seeds and the two steps (the mapper needs a device: tests/test_gpu_pe.py holds it to the
PAFs).  If a redrawn set misses a condition, change pe_cases.SIM_SEED, not the assertion."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import align_cases as ac  # noqa: E402
import orc  # noqa: E402
import pe_cases as pc  # noqa: E402
import sr_cases as sc  # noqa: E402
import mm2gb_amd as mm  # noqa: E402

LIMIT = 142 * 1024          # no fixture larger than the largest of tests/golden/paf_aln


def main():
    assert ac.ref_available() and os.path.exists(pc.REF_EXE), "build oracle/_ref first (make -C oracle ref)"
    seqs, reads = pc.sim_set()
    ctg = [(n, s) for (n, _), s in zip(pc.CONTIGS, seqs)]
    options = sc.ref_options()
    assert sc.own_options()["map"] == options["map"] and sc.own_options()["index"] == options["index"], "mm2gb_map_opt_init_sr differs from mm_set_opt(\"sr\")"
    options["max_chain_skip"] = 2**31 - 1               # main.c:316-318 under MM_F_SR
    pafs = {run: pc.record_paf(ctg, reads, args) for run, (args, _, _) in pc.RUNS.items()}
    frags = pc.fragments(reads)
    pairs = [f for f in frags if len(f) == 2]
    assert len(frags) >= 100 and sum(len(f) == 1 for f in frags) == 1 and all(len(f) <= 2 for f in frags)
    assert pc.record_paf(ctg, reads, ["-x", "sr"], two_files=([f[0] for f in pairs], [f[1] for f in pairs])) == \
        pc.record_paf(ctg, [r for f in pairs for r in f], ["-x", "sr"]), "two files and the interleaved file differ"
    # single-end, for comparison: with MM_F_FRAG_MODE off the program maps every read by itself
    se = pc.record_paf(ctg, [f[0] for f in pairs], ["-x", "sr"]) + pc.record_paf(ctg, [f[1] for f in pairs], ["-x", "sr"])
    worth = pc.worth_having(pafs, se)
    assert all(worth.values()), worth
    assert len({sum(len(s) for _, s in f) for f in pairs}) >= 4, "fewer than four distinct summed lengths"
    seeds = pc.record_seeds(ctg, reads)
    assert [s["name"] for s in seeds] == [f[0][0] for f in frags]
    doc = dict(seed=pc.SIM_SEED, contigs=[[n, s.decode()] for n, s in ctg], reads=[[n, s.decode()] for n, s in reads], options=options, pafs=pafs, se=se,
               seeds=[dict(rep_len=s["rep_len"], sd=s["sd"]) for s in seeds],
               made_by="tests/tools/gen_golden_pe.py: minimap2_cpu -t 1 (pe_cases.RUNS; --print-seeds for the SD / RS lines); mm_set_opt(\"sr\")")
    os.makedirs(pc.GOLD, exist_ok=True)
    path = os.path.join(pc.GOLD, "pe.npz")
    np.savez_compressed(path, doc=np.frombuffer(json.dumps(doc, sort_keys=True).encode("utf-8"), dtype=np.uint8))
    assert os.path.getsize(path) < LIMIT, f"{path} is {os.path.getsize(path)} bytes"
    # the host forms on the set: seeds, then the two steps against the reference's exported functions
    pc._gold = None
    o = mm.map_opt_sr()
    m = pc.matches_frag(frags)
    got, _ = mm.collect_seeds_heap_host(o.flag, m)
    bad = [f[0][0] for f, a, x, s in zip(frags, got, m, seeds) if pc.sd_rows(a) != s["sd"] or x["rep_len"] != s["rep_len"]]
    assert not bad, f"the host form differs from the recorded seeds for {bad}"
    ri = sc.SrRef([s for _, s in ctg])
    try:
        posts, qlens = [], []
        for f_id, (f, a) in enumerate(zip(frags, got)):
            if len(f) == 2:
                qlens.append([len(s) for _, s in f])
                posts.append(pc.ref_post(a, qlens[-1], f_id, ri.mo, ri.io.k))
    finally:
        ri.close()
    ppath = os.path.join(pc.GOLD, "post.npz")
    pc.save_post(ppath, posts, qlens)
    assert os.path.getsize(ppath) < LIMIT, f"{ppath} is {os.path.getsize(ppath)} bytes"
    gp = pc.golden_post()
    sr = mm.map_sr()
    kept = mm.select_sub_multi_host([p["regs_in"] for p in gp], [p["qlens"] for p in gp], [pc.max_dist_x(o, sr, sum(p["qlens"])) for p in gp], pri_ratio=o.pri_ratio,
                                    min_diff=2 * pc.K, best_n=o.best_n)
    assert all(np.array_equal(k, p["regs_kept"]) for k, p in zip(kept, gp)), "mm2gb_select_sub_multi_host differs from mm_select_sub_multi"
    ids = [f_id for f_id, f in enumerate(frags) if len(f) == 2]
    seg = mm.seg_gen_host([p["regs_kept"] for p in gp], [p["anchors"] for p in gp], [p["qlens"] for p in gp], [pc.frag_hash(i) for i in ids])
    assert all(np.array_equal(g[s][0], p["seg"][s][0]) and np.array_equal(g[s][1], p["seg"][s][1]) for g, p in zip(seg, gp) for s in range(2)), "mm2gb_seg_gen_host differs from mm_seg_gen"
    n_dropped = sum(len(p["regs_in"]) - len(p["regs_kept"]) for p in gp)
    print(f"{path}: {os.path.getsize(path)} bytes, {len(frags)} fragments; lines " + ", ".join(f"{k} {len(v.splitlines())}" for k, v in pafs.items()))
    print(f"{ppath}: {os.path.getsize(ppath)} bytes; {sum(len(p['regs_in']) for p in gp)} records, {n_dropped} dropped by mm_select_sub_multi")


if __name__ == "__main__":
    main()
