"""The chaining DP with the skip limit kept (k_skip_fill) against the exhaustive kernel (k_score) on the same batch, in the same process,
alternating: score time (range + plan + DP, the engine's ms_score and ms_prep), the whole f/p call, and the reference's mg_lchain_dp
(oracle/_ref/libmm2ref.so, fill + backtrack + compaction, one read per call on the usable CPUs) at the same limit on a sample of the
same reads; the walk's own counters (rounds per target, the slowest chunk's share of the walk: MM2GB_SKIP_STATS) and range + score +
backtrace through mm2gb_chain_gpu.  Prints one JSON document.

    python profiles/skip_rate.py --anchors 500000000 --reps 2 --ref-reads 512    # BASELINE configs[3]: 100-300 kb reads
    python profiles/skip_rate.py --anchors 2000000 --reps 1 --ref-reads 8        # rehearsal size
"""
import argparse
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import bench  # noqa: E402
import mm2gb_amd as mm  # noqa: E402
import orc  # noqa: E402


def ref_seconds(a, off, n_reads, max_skip, threads):
    """Seconds of the reference's mg_lchain_dp over the first n_reads reads, one read per call on `threads` threads."""
    path = os.path.join(orc.REF_DIR, "libmm2ref.so")
    if not os.path.exists(path):
        return None
    ref = C.CDLL(path)
    ref.mg_lchain_dp.restype = C.c_void_p
    ref.mg_lchain_dp.argtypes = [C.c_int] * 7 + [C.c_float, C.c_float, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_void_p), C.c_void_p]
    libc = C.CDLL(None)
    libc.malloc.restype = C.c_void_p
    libc.malloc.argtypes = [C.c_size_t]
    libc.free.argtypes = [C.c_void_p]
    prm = orc.default_param()

    def one(r):
        x = a[off[r]:off[r + 1]]
        buf = libc.malloc(max(16, x.nbytes))
        C.memmove(buf, x.ctypes.data, x.nbytes)
        n_u, u = C.c_int(0), C.c_void_p(0)
        res = ref.mg_lchain_dp(prm.max_dist_x, prm.max_dist_y, prm.bw, max_skip, prm.max_iter, prm.min_cnt, prm.min_sc,
                               prm.pen_gap, prm.pen_skip, 0, 1, len(x), buf, C.byref(n_u), C.byref(u), None)
        if res:
            libc.free(res)
        if u.value:
            libc.free(u)

    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(one, range(n_reads)))
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--anchors", type=int, default=500_000_000)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--skips", default="25,0")
    ap.add_argument("--ref-reads", type=int, default=512, help="reads of the batch the reference's mg_lchain_dp is timed on (0: not timed)")
    args = ap.parse_args()
    os.environ["MM2GB_SKIP_STATS"] = "1"                   # read when the engine is made: the walk's rounds, targets and slowest chunk
    os.environ["MM2GB_SLICE_ANCHORS"] = os.environ["MM2GB_CHAIN_SLICE_ANCHORS"] = str(1 << 40)   # the batch in one launch, as bench.py times k_score
    threads = max(1, bench.cpu_quota() or 16)
    _, n_reads, a, off = bench.shard_for_rank(mm, 0, 1, 2024, args.anchors, 100_000, 300_000, threads=threads)
    n = len(a)
    skips = [int(s) for s in args.skips.split(",")]
    out = {"command": " ".join(["python", "profiles/skip_rate.py"] + sys.argv[1:]), "anchors": n, "reads": int(n_reads), "threads": threads, "runs": {}}
    forms = [("exhaustive", orc.INT32_MAX, False)] + [(f"skip{s}", s, True) for s in skips]
    with mm.Engine() as e:
        for rep in range(args.reps + 1):                   # rep 0 warms up
            for name, ms, keep in forms:
                e.set_chain_skip(keep)
                e.set_misc(mm.default_misc(max_skip=ms))
                t0 = time.perf_counter()
                f, p, st = e.score(a, off)
                wall = time.perf_counter() - t0
                if rep == 0:
                    continue
                r = out["runs"].setdefault(name, {"ms_score": [], "ms_prep": [], "wall_s": [], "form": e.last_score_form()})
                r["ms_score"].append(round(st["ms_score"], 3)); r["ms_prep"].append(round(st["ms_prep"], 3)); r["wall_s"].append(round(wall, 3))
                r["n_pairs"] = st["n_pairs"]
                if e.last_score_form() == 1:
                    k = e.skip_stats()
                    k["rounds_per_target"] = round(k["rounds"] / max(1, k["targets"]), 2)
                    k["candidates_met_at_most_per_target"] = round(64 * k["rounds"] / max(1, k["targets"]), 1)
                    k["window_per_target"] = round(st["n_pairs"] / max(1, k["targets"]), 1)
                    k["slowest_chunk_share_of_the_walk"] = round(k["slowest_chunk_ticks"] / max(1, k["span_ticks"]), 3)
                    k["slowest_chunk_ms"] = round(k["slowest_chunk_ticks"] / 1e5, 3)
                    k["span_ms"] = round(k["span_ticks"] / 1e5, 3)
                    r["walk"] = k
            del f, p
        # range + score + backtrace + compaction, all on the device (mm2gb_chain_gpu; its time includes no transfer)
        for name, ms, keep in forms:
            e.set_chain_skip(keep)
            e.set_misc(mm.default_misc(max_skip=ms))
            _, st = e.chain_gpu(a, off)
            out["runs"][name]["chain_gpu_ms"] = {"prep": round(st["ms_prep"], 3), "score": round(st["ms_score"], 3), "post": round(st["ms_post"], 3),
                                                 "range_score_backtrace": round(st["ms_prep"] + st["ms_score"] + st["ms_post"], 3)}
    base = min(out["runs"]["exhaustive"]["ms_score"])
    nr = min(int(n_reads), args.ref_reads)
    share = off[nr] / n
    for name, ms, keep in forms:
        r = out["runs"][name]
        r["score_vs_exhaustive"] = round(min(r["ms_score"]) / base, 3)
        s = ref_seconds(a, off, nr, ms, threads) if nr > 0 else None
        if s is not None:
            whole = s / share
            r["reference"] = {"reads": nr, "anchors": int(off[nr]), "seconds": round(s, 3), "threads": threads, "seconds_whole_batch_scaled": round(whole, 2),
                              "note": "mg_lchain_dp = fill + backtrack + compaction, one read per call"}
            dev = r["chain_gpu_ms"]["range_score_backtrace"] / 1e3
            r["speedup_vs_reference_range_score_backtrace"] = round(whole / dev, 1)
            r["speedup_vs_reference_range_score"] = round(whole / (min(r["ms_prep"]) / 1e3 + min(r["ms_score"]) / 1e3), 1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
