#!/usr/bin/env python3
"""tests/golden/ksw/exts2_cases.npz from the REFERENCE, as data only (needs oracle/_ref, made by __graft_entry__.build() where the reference
checkout exists): about 2 000 jobs over the grid of tests/ksw_splice_cases.py -- mutated pairs and two-exon queries across planted introns,
sequences from this project's read simulator -- and what the reference's ksw_exts2_sse answered for each: the result fields and the CIGAR
words.  SCORE_ONLY jobs are recorded from the reference run WITHOUT that flag (ksw_splice_cases.ref_batch says why).
    python tests/tools/gen_golden_ksw_splice.py"""
import os
import sys

import numpy as np

TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(TESTS))
sys.path.insert(0, TESTS)
import ksw_cases as kc              # noqa: E402
import ksw_splice_cases as sc       # noqa: E402
import mm2gb_amd as mm              # noqa: E402

PER_SET, SEED, INTRON_HI = 100, 21, 600


def pack_param(p):
    return np.array([p.m] + list(p.mat) + [p.q, p.e, p.q2, p.noncan, p.junc_bonus], np.int8)


if __name__ == "__main__":
    if not kc.ref_available():
        sys.exit("reference build missing (oracle/_ref)")
    rng = np.random.default_rng(SEED)
    # the condition on the inputs, on the reference's own records for the planted kind at the first tuple
    p0 = sc.params()[0]
    j, q, t, junc = mm.ksw_splice_jobs(sc.planted_batch(rng, 1000, sc.LENS_CPU))
    sh = sc.input_shares(j, *sc.ref_batch(p0, j, q, t, junc))
    print("planted set, first tuple: " + ", ".join(f"{k} {v:.3f}" for k, v in sh.items()))
    sc.check_input_shares(sh)
    prm, jobs, qs, ts, js, res, words = [], [], [], [], [], [], []
    for p in sc.params():
        j, q, t, junc = mm.ksw_splice_jobs(sc.make_batch(rng, p.m, PER_SET, sc.LENS_CPU, p_empty=0.02, intron_hi=INTRON_HI))
        junc = np.zeros(len(t), np.uint8) if junc is None else junc
        r, w = sc.ref_batch(p, j, q, t, junc)
        prm.append(pack_param(p)); jobs.append(j); qs.append(q); ts.append(t); js.append(junc); res.append(r); words.append(w)
    ends = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)
    os.makedirs(os.path.dirname(sc.GOLD), exist_ok=True)
    np.savez_compressed(sc.GOLD, params=np.stack(prm), job_end=ends(jobs), q_end=ends(qs), t_end=ends(ts), word_end=ends(words), jobs=np.concatenate(jobs),
                        queries=np.concatenate(qs), targets=np.concatenate(ts), junc=np.concatenate(js), res=np.concatenate(res), words=np.concatenate(words))
    allr, allw = np.concatenate(res), np.concatenate(words)
    print(f"{sum(len(j) for j in jobs)} jobs in {len(prm)} parameter sets, {os.path.getsize(sc.GOLD)} bytes; "
          f"{int(((allw & 0xf) == 3).sum())} N words, {int((allr['zdropped'] != 0).sum())} z-dropped")
