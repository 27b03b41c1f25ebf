// wave_scan.h -- internal: scans over the 64 lanes of a wave that a skip-limited walk needs (gfx950).
// A walk meets 64 candidates per round, lane 0 first; the running best, the marks met inside the round and the skip counter of
// lchain.c:183-187 (mg_lchain_dp) or lchain.c:329-333 (mg_lchain_rmq) come from these scans.  Used by the RMQ fill's inner walk
// (post_kernels.hip, k_rmq_fill) and the chaining DP's walk (chain_kernels.hip, k_skip_fill).  Every lane must be active.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>

namespace mm2gb {

__device__ __forceinline__ int scan_lane() { return (int)(threadIdx.x & 63u); }

// The scans go by DPP inside the rows of 16 lanes (a shift is a vector instruction, not a trip through the LDS crossbar -- a round of
// the walk had ~30 of those behind each other) and by three scalar reads of the rows' last lanes across them.
template <int CTRL> __device__ __forceinline__ int dpp_or(int v, int otherwise) { return __builtin_amdgcn_update_dpp(otherwise, v, CTRL, 0xf, 0xf, false); }   // lanes without a source keep `otherwise`
constexpr int DPP_ROW_SHR = 0x110, DPP_WAVE_SHR1 = 0x138;
// largest value among the lanes BELOW this one (INT_MIN for lane 0)
__device__ __forceinline__ int wave_max_below(int v)
{
	v = max(v, dpp_or<DPP_ROW_SHR + 1>(v, INT_MIN)); v = max(v, dpp_or<DPP_ROW_SHR + 2>(v, INT_MIN));
	v = max(v, dpp_or<DPP_ROW_SHR + 4>(v, INT_MIN)); v = max(v, dpp_or<DPP_ROW_SHR + 8>(v, INT_MIN));
	const int t0 = __builtin_amdgcn_readlane(v, 15), t1 = max(t0, __builtin_amdgcn_readlane(v, 31)), t2 = max(t1, __builtin_amdgcn_readlane(v, 47));
	const int row = scan_lane() >> 4;
	v = max(v, row == 0 ? INT_MIN : row == 1 ? t0 : row == 2 ? t1 : t2);
	return dpp_or<DPP_WAVE_SHR1>(v, INT_MIN);
}
__device__ __forceinline__ unsigned wave_or_u32(unsigned x)
{
	int v = (int)x;
	v |= dpp_or<DPP_ROW_SHR + 1>(v, 0); v |= dpp_or<DPP_ROW_SHR + 2>(v, 0); v |= dpp_or<DPP_ROW_SHR + 4>(v, 0); v |= dpp_or<DPP_ROW_SHR + 8>(v, 0);
	return (unsigned)(__builtin_amdgcn_readlane(v, 15) | __builtin_amdgcn_readlane(v, 31) | __builtin_amdgcn_readlane(v, 47) | __builtin_amdgcn_readlane(v, 63));
}
__device__ __forceinline__ unsigned long long wave_or_u64(unsigned long long v) { return (unsigned long long)wave_or_u32((unsigned)(v >> 32)) << 32 | wave_or_u32((unsigned)v); }
// The skip counter is a chain of x -> max(x - 1, 0) (a better score was met), x -> x + 1 (a candidate whose chain had been offered) and
// x -> x: all of the form x -> max(x + a, b), closed under composition -- (a1, b1) then (a2, b2) is (a1 + a2, max(b1 + a2, b2)) --, so the
// counter after every lane comes from a prefix scan of the lanes' (a, b).  NONE stands for "no lower bound" (far below any count).
constexpr int SKIP_NONE = INT_MIN / 4;
__device__ __forceinline__ int wave_skip_counts(int a, int bnd, int before)
{
	// (the earlier lanes' step first, then this one's)
#define MM2GB_SKIP_STEP(N) { const int oa = dpp_or<DPP_ROW_SHR + N>(a, 0), ob = dpp_or<DPP_ROW_SHR + N>(bnd, SKIP_NONE); bnd = max(ob + a, bnd); a = oa + a; }
	MM2GB_SKIP_STEP(1) MM2GB_SKIP_STEP(2) MM2GB_SKIP_STEP(4) MM2GB_SKIP_STEP(8)
#undef MM2GB_SKIP_STEP
	// the rows before this lane's: their last lanes' (a, b), composed in order
	const int a0 = __builtin_amdgcn_readlane(a, 15), b0 = __builtin_amdgcn_readlane(bnd, 15);
	const int ra1 = __builtin_amdgcn_readlane(a, 31), rb1 = __builtin_amdgcn_readlane(bnd, 31);
	const int ra2 = __builtin_amdgcn_readlane(a, 47), rb2 = __builtin_amdgcn_readlane(bnd, 47);
	const int a1 = a0 + ra1, b1 = max(b0 + ra1, rb1);               // rows 0 and 1
	const int a2 = a1 + ra2, b2 = max(b1 + ra2, rb2);               // rows 0 .. 2
	const int row = scan_lane() >> 4;
	const int pa = row == 0 ? 0 : row == 1 ? a0 : row == 2 ? a1 : a2, pb = row == 0 ? SKIP_NONE : row == 1 ? b0 : row == 2 ? b1 : b2;
	bnd = max(pb + a, bnd); a = pa + a;
	return max(before + a, max(bnd, SKIP_NONE));
}

} // namespace mm2gb
