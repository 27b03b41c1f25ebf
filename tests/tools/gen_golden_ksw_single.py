#!/usr/bin/env python3
"""tests/golden/ksw/extz2_cases.npz from the REFERENCE, as data only (needs oracle/_ref, made by __graft_entry__.build() where the reference
checkout exists): 2 000 jobs over the grid of tests/ksw_single_cases.py -- sequences from this project's read simulator -- and what the
reference's ksw_extz2_sse answered for each: the eleven result fields and the CIGAR words.
    python tests/tools/gen_golden_ksw_single.py"""
import os
import sys

import numpy as np

TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(TESTS))
sys.path.insert(0, TESTS)
import ksw_cases as kc      # noqa: E402
import ksw_single_cases as ks      # noqa: E402

PER_SET, SEED = 100, 21


def pack_param(p):
    return np.array([p.m] + list(p.mat) + [p.q, p.e, p.q2, p.e2], np.int8)


if __name__ == "__main__":
    if not kc.ref_available():
        sys.exit("reference build missing (oracle/_ref)")
    rng = np.random.default_rng(SEED)
    prm, jobs, qs, ts, res, words = [], [], [], [], [], []
    for p in ks.params():
        j, q, t = kc.make_batch(rng, p.m, PER_SET, kc.LENS_CPU, p_empty=0.02)
        r, w = ks.ref_batch(p, j, q, t)
        prm.append(pack_param(p)); jobs.append(j); qs.append(q); ts.append(t); res.append(r); words.append(w)
    traps = ks.trap_batches()
    for name in ks.TRAPS:          # behind the grid's sets
        p, j, q, t = traps[name]
        r, w = ks.ref_batch(p, j, q, t)
        prm.append(pack_param(p)); jobs.append(j); qs.append(q); ts.append(t); res.append(r); words.append(w)
    ends = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)
    os.makedirs(os.path.dirname(ks.GOLD), exist_ok=True)
    np.savez_compressed(ks.GOLD, params=np.stack(prm), job_end=ends(jobs), q_end=ends(qs), t_end=ends(ts), word_end=ends(words), jobs=np.concatenate(jobs),
                        queries=np.concatenate(qs), targets=np.concatenate(ts), res=np.concatenate(res), words=np.concatenate(words))
    sh = kc.shares(np.concatenate(res))
    print(f"{sum(len(j) for j in jobs)} jobs in {len(prm)} parameter sets, {os.path.getsize(ks.GOLD)} bytes; shares " + ", ".join(f"{k} {v:.3f}" for k, v in sh.items()))
