#!/usr/bin/env python3
"""Instrumented build of the score kernel for profiles/stage_kinds.py: a COPY of csrc/chain_kernels.hip that counts the stages of the band
pass (band_group) by the sweep form they take and the last stages by their number of sources, compiled with the other objects into
mm2-gb_amd/ab/libstages.so (git-ignored).  The tracked sources are not touched.   python profiles/experiments/make_stage_kinds_build.py"""
import os, subprocess
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.join(ROOT, "mm2-gb_amd")
src = open(os.path.join(PKG, "csrc", "chain_kernels.hip")).read()


def put(after, text):
    global src
    assert src.count(after) == 1, after
    src = src.replace(after, after + text, 1)


# [kind + 8 * (last stage)], kind: 0 FAR, 1 free, 2 no_check only, 3 band edge, 4 FAR with the window test (head), 5 free with the window test (head);
# [16] band-edge stages left of every target (gx_min > sx_max) that fail the free span; [32 + n]: last stages of n sources
put("struct BandIO { glb_i32_cptr raw, st, f, diag; glb_i32_ptr res; };\n",
    "__device__ unsigned long long g_stage_counts[128];\n"
    "__device__ __forceinline__ void count_stage(int lane, int at) { if (lane == 0) atomicAdd(&g_stage_counts[at], 1ull); }\n")
put("\t\t\t\tint idx = sidx, k_to = WAVE;\n", "\t\t\t\tbool last_ = false;\n")
put("\t\t\t\t\tif (n_st == 0) break;\n", "\t\t\t\t\tlast_ = true; count_stage(lane, 32 + n_st);\n")
put("\t\t\t\tstage_block_lut_at(lane, xs, ys, sf, sq, stage, far_block, d0);\n",
    "\t\t\t\tcount_stage(lane, (far_block ? (inside ? 0 : 4) : free_block ? (inside ? 1 : 5) : no_check ? 2 : 3) + (last_ ? 8 : 0));\n"
    "\t\t\t\tif (!free_block && !no_check && left) count_stage(lane, 16);\n")
src += '''
extern "C" void mm2gb_debug_stage_counts(unsigned long long *out, int reset)
{
	(void)hipDeviceSynchronize();
	(void)hipMemcpyFromSymbol(out, HIP_SYMBOL(mm2gb::g_stage_counts), 1024);
	if (reset) { unsigned long long z[128] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(mm2gb::g_stage_counts), z, 1024); }
}
'''
out_dir = os.path.join(PKG, "ab")
os.makedirs(out_dir, exist_ok=True)
tmp = os.path.join(PKG, "csrc", "chain_kernels_stages_tmp.hip")
open(tmp, "w").write(src)
try:
    subprocess.check_call(["make", "-s", "-C", PKG])
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include")]
    obj = os.path.join(out_dir, "chain_kernels_stages.o")
    subprocess.check_call(["/opt/rocm/bin/hipcc"] + flags + ["-c", tmp, "-o", obj])
    others = [os.path.join(PKG, "build", f) for f in os.listdir(os.path.join(PKG, "build")) if f.endswith(".o") and f != "chain_kernels.o"]
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", obj] + others + ["-o", os.path.join(out_dir, "libstages.so"), "-lpthread"])
finally:
    os.remove(tmp)
print(os.path.join(out_dir, "libstages.so"))
