#!/usr/bin/env python3
"""tests/golden/hpc/* from the REFERENCE, as data only (needs oracle/_ref, made by __graft_entry__.build() where the reference checkout
exists): what mm_sketch(..., is_hpc = 1) returns for the sequences of tests/hpc_cases.py, what mm_collect_matches handed on under
-H -k19 (through oracle/capture_hooks.c), and the PAF of `-x map-pb` at max-chain-skip = infinity.
    python tests/tools/gen_golden_hpc.py"""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, TESTS)
import golden_io      # noqa: E402
import hpc_cases      # noqa: E402
import orc            # noqa: E402
import sim_reads      # noqa: E402

DATA = os.path.join(golden_io.GOLD, "data")
OUT = hpc_cases.HPC
HPC_ARGS = ["-H", "-k19"]
PAIRS = {"mt": ("MT-human.fa", "MT-orang.fa"), "inv": ("t-inv.fa", "q-inv.fa")}


class Mm128V(C.Structure):
    _fields_ = [("n", C.c_size_t), ("m", C.c_size_t), ("a", C.c_void_p)]


def ref_sketch(lib, seq, w, k, rid=0, is_hpc=1):
    """mm_sketch (sketch.c:77) of the reference build: (n, 2) uint64."""
    v = Mm128V(0, 0, None)
    if len(seq) > 0:
        lib.mm_sketch(None, seq, len(seq), w, k, rid, is_hpc, C.byref(v))
    out = np.ctypeslib.as_array(C.cast(v.a, C.POINTER(C.c_uint64)), shape=(v.n * 2,)).reshape(-1, 2).copy() if v.n else np.zeros((0, 2), np.uint64)
    if v.a:
        lib.kfree(None, v.a)
    return out


def ref_lib():
    lib = C.CDLL(os.path.join(orc.REF_DIR, "libminimap2ref.so"))
    lib.mm_sketch.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_int, C.POINTER(Mm128V)]
    lib.mm_sketch.restype = None
    lib.kfree.argtypes = [C.c_void_p, C.c_void_p]
    lib.kfree.restype = None
    return lib


def capture(tgt, qry, extra):
    exe, hook = os.path.join(orc.REF_DIR, "minimap2_cpu"), os.path.join(orc.REF_DIR, "libcapture.so")
    with tempfile.TemporaryDirectory() as td:
        cap = os.path.join(td, "seeds.bin")
        subprocess.run([exe, "-t", "1"] + extra + [tgt, qry], env=dict(os.environ, LD_PRELOAD=hook, MM2GB_CAPTURE_SEEDS=cap), check=True, capture_output=True)
        return orc.read_seed_capture(cap) if os.path.exists(cap) else []


def paf(tgt, qry, to):
    r = subprocess.run([os.path.join(orc.REF_DIR, "minimap2_cpu"), "-t", "1", "-x", "map-pb", "--max-chain-skip=2147483647", tgt, qry], check=True, capture_output=True)
    open(to, "wb").write(r.stdout)
    return r.stdout.decode()


def save_seeds(name, k, r, source):
    meta = dict(flag=0, qlen=int(r["qlen"]), rep_len=int(r["rep_len"]), source=source, record=k)
    np.savez_compressed(os.path.join(OUT, "seeds", f"{name}_{k}.npz"), seeds=r["seeds"], hits=r["hits"], hit_off=r["hit_off"], a=r["a"], mini_pos=r["mini_pos"],
                        meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8))


if __name__ == "__main__":
    if not orc.ref_available():
        sys.exit("reference build missing (oracle/_ref)")
    os.makedirs(os.path.join(OUT, "seeds"), exist_ok=True)
    info = {}
    lib = ref_lib()
    seqs = hpc_cases.sequences(1)
    off = np.zeros(len(seqs) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    for k, w in hpc_cases.KW:
        sk = [ref_sketch(lib, s, w, k, rid=r) for r, s in enumerate(seqs)]
        xy_off = np.zeros(len(seqs) + 1, np.int64)
        xy_off[1:] = np.cumsum([len(x) for x in sk])
        np.savez_compressed(os.path.join(OUT, f"sketch_k{k}_w{w}.npz"), seqs=np.frombuffer(b"".join(seqs), np.uint8), seq_off=off, xy=np.concatenate(sk), xy_off=xy_off)
        print(f"sketch k={k} w={w}: {xy_off[-1]} pairs, {int(((np.concatenate(sk)[:, 0] & np.uint64(0xff)) > k).sum())} with span > k")
    for name, (tgt, qry) in PAIRS.items():
        recs = capture(os.path.join(DATA, tgt), os.path.join(DATA, qry), HPC_ARGS)
        for k, r in enumerate(recs):
            save_seeds(name, k, r, f"{tgt} x {qry} {' '.join(HPC_ARGS)}")
        text = paf(os.path.join(DATA, tgt), os.path.join(DATA, qry), os.path.join(OUT, f"real_{name}_map-pb.paf"))
        info[name] = dict(records=len(recs), paf_lines=len(text.splitlines()))
        print(f"{name}: {len(recs)} records, {len(text.splitlines())} PAF lines")
    with tempfile.TemporaryDirectory() as td:
        ref_fa, reads_fa = os.path.join(td, "ref.fa"), os.path.join(td, "reads.fa")
        sim_reads.simulate(ref_fa, reads_fa, seed=5, n_reads=150, len_lo=3_000, len_hi=20_000)         # as oracle/gen_golden_seeds.py
        recs = capture(ref_fa, reads_fa, HPC_ARGS)
        assert len(recs) == 150
        rep = [k for k, r in enumerate(recs) if r["rep_len"] > 0]
        pick = sorted(set([0, 1, 2, 3] + rep[:6]))
        for k in pick:
            save_seeds("sim", k, recs[k], "tests/sim_reads.py seed=5 n_reads=150 " + " ".join(HPC_ARGS))
        info["sim"] = dict(reads=pick, n_rep_len_positive=len(rep), rep_len=[int(recs[k]["rep_len"]) for k in pick])
        print("sim:", info["sim"])
        m = json.load(open(os.path.join(golden_io.GOLD, "sim160.json")))
        sim_reads.simulate(ref_fa, reads_fa, seed=m["seed"], n_reads=m["n_reads"], len_lo=m["len_lo"], len_hi=m["len_hi"], tandem=m["tandem"])
        assert hashlib.md5(open(ref_fa, "rb").read()).hexdigest() == m["ref_md5"] and hashlib.md5(open(reads_fa, "rb").read()).hexdigest() == m["reads_md5"]
        text = paf(ref_fa, reads_fa, os.path.join(OUT, "sim160_map-pb.paf"))
        info["sim160"] = dict(paf_lines=len(text.splitlines()), reads_mapped=len({ln.split("\t")[0] for ln in text.splitlines()}))
        print("sim160:", info["sim160"])
    info["made_by"] = "tests/tools/gen_golden_hpc.py: mm_sketch(is_hpc=1); minimap2_cpu -t 1 -H -k19 (seed recordings); -t 1 -x map-pb --max-chain-skip=2147483647 (PAF)"
    json.dump(info, open(os.path.join(OUT, "meta.json"), "w"), indent=1)
