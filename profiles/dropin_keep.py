"""The wrapped reference host (oracle/_ref/minimap2_gpuhost_rmq) on bench.py's 1.05 Gbp read set at minimap2's default --max-chain-skip (25)
and at the reference README's `infinity` (= 0), with MM2GB_CHAIN_SKIP=keep: whole-program seconds, and the sampled reads (every 16th distinct
read) whose PAF differs from oracle/_ref/minimap2_cpu's at the same flag.  Uses bench.py's helpers; prints one JSON document.

    python profiles/dropin_keep.py                 # 1.05 Gbp, as bench.py's e2e.reference_host_at_scale
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=1_000_000_000)
    args = ap.parse_args()
    threads = max(1, min(32, bench.cpu_quota() or 16))
    cpu = os.path.join(ROOT, "oracle", "_ref", "minimap2_cpu")
    with tempfile.TemporaryDirectory() as td:
        ref, refs, uniq, reads, unique_bases, copies, bases = bench.scale_read_set(td, args.bases)
        sample = [(f"{n}_c0", s) for n, s in uniq[::16]]
        sp = os.path.join(td, "sample.fa")
        with open(sp, "wb") as fh:
            for n, sq in sample:
                fh.write(b">" + n.encode() + b"\n" + bytes(sq) + b"\n")
        want_by_flag = {}
        for name in ("default25", "readme_infinity"):
            flag = bench.SKIP_FLAGS[name]
            r = subprocess.run([cpu, "-t", str(threads)] + ([flag] if flag else []) + [ref, sp], capture_output=True, timeout=900)
            want_by_flag[name] = r.stdout.decode() if r.returncode == 0 else None
        out = bench.reference_host_at_scale(td, ref, reads, bases, uniq, None, threads, legs=("gpuhost_rmq@default25", "gpuhost_rmq@readme_infinity"),
                                            extra_env={"MM2GB_CHAIN_SKIP": "keep"}, want_by_flag=want_by_flag)
    out["env"] = {"MM2GB_CHAIN_SKIP": "keep"}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
