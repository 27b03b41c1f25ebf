"""Inputs and models for the homopolymer-compressed sketch (tests/test_hpc_cpu.py, tests/test_gpu_hpc.py, tests/tools/gen_golden_hpc.py):
sequences with long homopolymers, a Python model of the sketch BY POSITION -- the formulation csrc/seed_kernels.hip's HPC-form kernels
implement --, and the loaders of tests/golden/hpc."""
import glob
import json
import os

import numpy as np

import golden_io

HPC = os.path.join(golden_io.GOLD, "hpc")
KW = [(4, 3), (6, 5), (11, 10), (15, 10), (19, 10), (19, 5), (28, 19), (15, 1), (2, 50)]
NONE = (1 << 64) - 1
CODE = np.full(256, 4, np.uint8)
for _c, _v in zip(b"ACGTUacgtu", (0, 1, 2, 3, 3, 0, 1, 2, 3, 3)):
    CODE[_c] = _v


def hpc_seq(rng, n, p_n=0.004, p_long=0.0, mixed_case=True):
    """n bases in runs of geometric length (mean 2; with probability p_long 200-400), runs of N now and then, lower case in stretches."""
    out = bytearray()
    prev = -1
    while len(out) < n:
        if rng.random() < p_n:
            out += b"N" * int(rng.integers(1, 6))
            prev = -1
            continue
        c = int(rng.integers(0, 4))
        if c == prev:
            continue
        prev = c
        ln = int(rng.integers(200, 401)) if rng.random() < p_long else int(rng.geometric(0.5))
        out += bytes([b"ACGT"[c]]) * ln
    out = out[:n]
    if mixed_case and n > 0:
        for _ in range(1 + n // 400):
            a = int(rng.integers(0, n))
            b = min(n, a + int(rng.integers(1, 60)))
            out[a:b] = bytes(out[a:b]).lower()
    return bytes(out)


def sequences(seed, n_seq=24, max_len=1200):
    """The sequences of the golden sketches (seed 1) and of the fresh draws: lengths from 1 on, one with a run of 300 in the middle."""
    rng = np.random.default_rng(seed)
    lens = [1, 2, 3, 7, 19, 40] + [int(x) for x in rng.integers(50, max_len, n_seq - 8)]
    seqs = [hpc_seq(rng, n) for n in lens]
    seqs.append(hpc_seq(rng, 500) + b"g" * 150 + b"G" * 150 + hpc_seq(rng, 400))           # every k-mer across the run spans 256 or more
    seqs.append(hpc_seq(rng, 900, p_long=0.01))
    return seqs


def mix(key, mask):
    key = (~key + (key << 21)) & mask
    key ^= key >> 24
    key = (key + (key << 3) + (key << 8)) & mask
    key ^= key >> 14
    key = (key + (key << 2) + (key << 4)) & mask
    key ^= key >> 28
    key = (key + (key << 31)) & mask
    return key


def steps_by_position(seq, k, rid=0, stats=None):
    """The counted steps of the compressed sketch, each from the sequence alone: a list of (x, y, l).  A BOUNDARY is an ambiguous base, or a
    base that is the sequence's first or differs from the one before it; a run start's k-mer is the last k entries of the run-compacted
    bases (ambiguous ones removed), its position the base before the next boundary, its span that position minus the first base of the
    last min(k, m) runs plus one (m: runs since the last ambiguous base); it is not counted when the k-mer is its own reverse complement;
    l = counted run starts since the last ambiguous base; it has a value iff l >= k and span < 256.  stats (a dict) receives how many
    k-mers were their own reverse complement ("symmetric") and how many were left out for their span alone ("long")."""
    code = CODE[np.frombuffer(seq, np.uint8)]
    n = len(code)
    bnd = [i for i in range(n) if code[i] == 4 or i == 0 or code[i - 1] != code[i]]
    mask = (1 << 2 * k) - 1
    comp, starts, steps = [], [], []
    l = 0
    for b, i in enumerate(bnd):
        if code[i] == 4:
            starts, l = [], 0
            steps.append((NONE, NONE, 0))
            continue
        end = (bnd[b + 1] if b + 1 < len(bnd) else n) - 1
        comp.append(int(code[i]))
        starts.append(i)
        m = len(starts)
        span = end - starts[max(m - k, 0)] + 1
        fwd = rev = 0
        for d, c in enumerate(reversed(comp[-k:])):
            fwd |= c << 2 * d
            rev |= (3 ^ c) << (2 * (k - 1) - 2 * d)
        if fwd == rev:
            if stats is not None:
                stats["symmetric"] = stats.get("symmetric", 0) + 1
            continue
        strand = 0 if fwd < rev else 1
        l += 1
        if l >= k and span < 256:
            steps.append((mix(rev if strand else fwd, mask) << 8 | span, rid << 32 | end << 1 | strand, l))
        else:
            if stats is not None and l >= k:
                stats["long"] = stats.get("long", 0) + 1
            steps.append((NONE, NONE, l))
    return steps


def has_twins(steps, w):
    """Two steps of equal value inside one window."""
    xs = [x for x, _, _ in steps]
    return any(xs[i] != NONE and xs[i] in xs[i + 1:i + w] for i in range(len(xs)))


def ring(steps, w, k):
    """The window logic of sketch.c:110-142 over counted steps (x, y, l), as csrc/seeding.cpp restates it."""
    out = []
    buf = [(NONE, NONE)] * w
    best, best_slot, slot = (NONE, NONE), 0, 0
    for x, y, l in steps:
        cur = (x, y)
        buf[slot] = cur
        if l == w + k - 1 and best[0] != NONE:
            out += [q for q in buf[slot + 1:] + buf[:slot] if q[0] == best[0] and q[1] != best[1]]
        if cur[0] <= best[0]:
            if l >= w + k and best[0] != NONE:
                out.append(best)
            best, best_slot = cur, slot
        elif slot == best_slot:
            if l >= w + k - 1 and best[0] != NONE:
                out.append(best)
            best = (NONE, NONE)
            for j in list(range(slot + 1, w)) + list(range(0, slot + 1)):
                if buf[j][0] <= best[0]:
                    best, best_slot = buf[j], j
            if l >= w + k - 1 and best[0] != NONE:
                out += [q for q in buf[slot + 1:] + buf[:slot + 1] if q[0] == best[0] and q[1] != best[1]]
        slot = (slot + 1) % w
    if best[0] != NONE:
        out.append(best)
    return np.array(out, np.uint64).reshape(-1, 2)


def model_sketch(seq, w, k, rid=0):
    return ring(steps_by_position(seq, k, rid), w, k)


def load_sketch(k, w):
    z = np.load(os.path.join(HPC, f"sketch_k{k}_w{w}.npz"))
    flat, off, xy, xy_off = bytes(z["seqs"]), z["seq_off"], z["xy"], z["xy_off"]
    return [flat[off[r]:off[r + 1]] for r in range(len(off) - 1)], [xy[xy_off[r]:xy_off[r + 1]] for r in range(len(off) - 1)]


def seed_cases(prefix=""):
    return sorted(glob.glob(os.path.join(HPC, "seeds", prefix + "*.npz")))


def meta():
    return json.load(open(os.path.join(HPC, "meta.json")))
