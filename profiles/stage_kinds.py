#!/usr/bin/env python3
"""The stages of the band pass (band_group) by the sweep form they take, and its last stages by their number of sources, for ONE
score_device call on the bench batch: needs the instrumented library (python profiles/experiments/make_stage_kinds_build.py ->
mm2-gb_amd/ab/libstages.so).  Prints JSON.   python profiles/stage_kinds.py [--anchors N]"""
import argparse, ctypes as C, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ["MM2GB_LIB_PATH"] = os.path.join(ROOT, "mm2-gb_amd", "ab", "libstages.so")
sys.path.insert(0, ROOT)
import numpy as np
import torch
import mm2gb_amd as mm
from bench import shard_for_rank

ap = argparse.ArgumentParser()
ap.add_argument("--anchors", type=int, default=500_000_000)
args = ap.parse_args()
first, n_reads, anchors, off = shard_for_rank(mm, 0, 1, 2024, args.anchors, 100_000, 300_000, 16)
n = int(off[-1])
dev = torch.device("cuda", 0)
d_a = torch.from_numpy(anchors.view(np.int64)).to(dev)
d_off = torch.from_numpy(off).to(dev)
d_f = torch.empty(n, dtype=torch.int32, device=dev)
d_p = torch.empty(n, dtype=torch.int32, device=dev)
torch.cuda.synchronize()
cnt = (C.c_ulonglong * 128)()
with mm.Engine() as e:
    mm.lib().mm2gb_debug_stage_counts(cnt, 1)
    e.score_device(n_reads, d_off.data_ptr(), d_a.data_ptr(), n, d_f.data_ptr(), d_p.data_ptr())
    e.sync()
    mm.lib().mm2gb_debug_stage_counts(cnt, 1)
    groups, chunks = e.band_groups(), e.sparse_chunks()
c = list(cnt)
kinds = ("far", "free", "no_check_only", "band_edge", "far_head", "free_head")
stages = sum(c[:6]) + sum(c[8:14])
last = {k: c[32 + k] for k in range(1, 64)}
n_last = sum(last.values())
swept_for_nothing = sum(v * (64 - k) for k, v in last.items())
swept_short = sum(v * (((k + 3) & ~3) - k) for k, v in last.items())
print(json.dumps({
    "anchors": n, "band_groups": list(groups), "sparse_chunks": chunks, "stages": stages,
    "full_stages_by_form": dict(zip(kinds, c[:6])), "last_stages_by_form": dict(zip(kinds, c[8:14])),
    "share_of_stages": {k: round((c[i] + c[8 + i]) / max(1, stages), 4) for i, k in enumerate(kinds)},
    "band_edge_left_of_every_target_but_beyond_the_free_span": c[16],
    "last_stages": n_last, "last_stage_mean_sources": round(sum(k * v for k, v in last.items()) / max(1, n_last), 2),
    "padded_sources_swept_in_last_stages_now": swept_for_nothing, "padded_sources_left_with_groups_of_4": swept_short,
    "last_stages_by_sources": last}))
