// est_err_kernels.hip -- the device form of mm_est_err's walk (esterr.c:30-61; mm2gb_est_err_gpu).  est_err.cpp is the definition.
// Two steps:
//   reads  (k_est_err_reads)  a wave per read: the sum of its minimizers' spans (esterr.c:37-38), whether their positions are strictly
//          ascending, and the read of every hit record (the walk's kernels are launched per hit, not per read).
//   walk   (k_est_err<G>)  a group of G lanes per hit: G = 64 (a wave) for hits of EE_LONG anchors or more, G = 16 below that; each
//          instantiation passes over the hits of the other.  A read has hundreds of hits and a chain tens of thousands of anchors, so
//          neither a lane per read nor a lane per hit would do.
// The walk of esterr.c:53-58 is a merge of two sequences: the chain's forward query positions x_1 .. x_{cnt-1} and the positions
// mini_pos[st+1 ..].  It advances k only when x_k is met at some j beyond the place of x_{k-1}.  Where mini_pos is STRICTLY ascending every
// value beyond that place exceeds x_{k-1}, so x_k is met there if and only if x_k > x_{k-1} and x_k is among the read's positions at all; and
// once some x_F is not met, j runs to n and the walk is over (the early end at j == n).  Hence
//     n_match = F = the first k >= 1 that is not strictly above its predecessor or absent from mini_pos (cnt if there is none),
//     en      = the place of x_{F-1},
// and every k can be tested on its own: a lane takes an anchor, searches its position, and the group takes the minimum of the failing k.
// The chain's own order plays no part in the argument (a chain of the reverse strand under homopolymer compression need not descend
// strictly in forward position: such an anchor simply ends the walk, as it does in the reference).  Where a read's mini_pos is NOT
// strictly ascending the argument does not hold and lane 0 of the group walks as esterr.c does (est_err_literal).
// No atomics, no LDS, no scratch; a hit's result is stored once.
#include <algorithm>
#include "engine.h"

namespace mm2gb {

namespace {

constexpr int EE_WG = 256;
constexpr int EE_LONG = 64;             // anchors from which a hit is a wave's

// esterr.c:7-14 on the anchor's two words as the kernels read them (x low, x high, y low, y high)
__device__ __forceinline__ int ee_for_qpos(int qlen, const uint4 a)
{
	const int x = (int)a.z, span = (int)(a.w & 0xffu);
	return a.y >> 31 ? qlen - 1 - (x + 1 - span) : x;
}

// esterr.c:16-28 on mp[lo .. hi]
__device__ __forceinline__ int ee_find(const unsigned long long *__restrict__ mp, int lo, int hi, int x)
{
	while (lo <= hi) {
		const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1), y = (int)(unsigned)mp[mid];
		if (y < x) lo = mid + 1;
		else if (y > x) hi = mid - 1;
		else return mid;
	}
	return -1;
}

// esterr.c:53-58 to the letter, one lane
__device__ int2 est_err_literal(const uint4 *__restrict__ a, int cnt, bool rev, int qlen, const unsigned long long *__restrict__ mp, int n, int st)
{
	int en = st, n_match = 1;
	for (int k = 1, j = st + 1; j < n && k < cnt; ++j)
		if (ee_for_qpos(qlen, a[rev ? cnt - 1 - k : k]) == (int)(unsigned)mp[j]) { ++k; en = j; ++n_match; }
	return make_int2(n_match, en);
}

} // namespace

__global__ __launch_bounds__(EE_WG) void k_est_err_reads(EstErrBatch b)
{
	const int l = threadIdx.x & 63;
	const int per = EE_WG / 64;
	for (int64_t r = (int64_t)blockIdx.x * per + (threadIdx.x >> 6); r < b.n_reads; r += (int64_t)gridDim.x * per) {
		const int64_t m0 = b.mini_off[r];
		const int n = (int)(b.mini_off[r + 1] - m0);
		const unsigned long long *mp = b.mini_pos + m0;
		unsigned long long sum = 0;
		int bad = 0;
		for (int i = l; i < n; i += 64) {
			const unsigned long long v = mp[i];
			sum += v >> 32 & 0xff;
			if (i > 0 && (int)(unsigned)mp[i - 1] >= (int)(unsigned)v) bad = 1;
		}
		for (int o = 32; o > 0; o >>= 1) { sum += __shfl_xor(sum, o); bad |= __shfl_xor(bad, o); }
		if (l == 0) { b.sum_k[r] = sum; b.read_literal[r] = bad; }
		const int64_t g0 = b.reg_off[r], g1 = b.reg_off[r + 1];
		for (int64_t j = g0 + l; j < g1; j += 64) b.reg_read[j] = (int32_t)r;
	}
}

template <int G>
__global__ __launch_bounds__(EE_WG) void k_est_err(EstErrBatch b)
{
	const int gl = threadIdx.x & (G - 1);
	const int64_t groups = (int64_t)gridDim.x * (EE_WG / G);
	for (int64_t h = (int64_t)blockIdx.x * (EE_WG / G) + threadIdx.x / G; h < b.n_regs; h += groups) {
		const RegRecord g = b.regs[h];
		const int cnt = g.cnt;
		if ((cnt >= EE_LONG) != (G == 64)) continue;                  // the other instantiation's
		const int r = b.reg_read[h];
		const int64_t m0 = b.mini_off[r];
		const int n = (int)(b.mini_off[r + 1] - m0);
		const unsigned long long *mp = b.mini_pos + m0;
		const int qlen = b.qlen[r];
		const bool rev = (g.flags >> 10) & 1;
		const uint4 *a = b.a + b.a_off[r] + g.as;
		int2 res = make_int2(0, -1);                                  // esterr.c:45-51: no anchors, or the first one's position is not a minimizer's
		int st = -1, x0 = 0;
		if (n > 0 && cnt > 0) { x0 = ee_for_qpos(qlen, a[rev ? cnt - 1 : 0]); st = ee_find(mp, 0, n - 1, x0); }
		if (st >= 0) {
			int n_match, en;
			if (b.read_literal[r]) {
				int2 w = make_int2(0, 0);
				if (gl == 0) w = est_err_literal(a, cnt, rev, qlen, mp, n, st);
				n_match = __shfl(w.x, 0, G); en = __shfl(w.y, 0, G);
			} else {
				int fail = cnt;                                           // the first k that ends the walk
				for (int base = 1; base < cnt; base += G) {
					const int k = base + gl;
					if (k < cnt) {
						const int xk = ee_for_qpos(qlen, a[rev ? cnt - 1 - k : k]), xp = ee_for_qpos(qlen, a[rev ? cnt - k : k - 1]);
						// positions ascend strictly from st on: x_k, if it is there, lies k .. x_k - x_0 places beyond it
						const int64_t hi = (int64_t)st + ((int64_t)xk - x0);
						if (xk <= xp || ee_find(mp, st + k < n ? st + k : n, (int)(hi < n - 1 ? hi : n - 1), xk) < 0) fail = k;
					}
					int f = fail;
					for (int o = G >> 1; o > 0; o >>= 1) { const int v = __shfl_xor(f, o, G); f = v < f ? v : f; }
					fail = f;
					if (fail < cnt) break;                                // (uniform in the group; later rounds hold larger k only)
				}
				n_match = fail;
				en = st;
				if (n_match > 1) {                                        // the place of the last anchor met (every lane the same search: one line)
					const int xl = ee_for_qpos(qlen, a[rev ? cnt - n_match : n_match - 1]);
					en = ee_find(mp, st + 1, n - 1, xl);
				}
			}
			// esterr.c:59-61
			const float avg_k = __fdiv_rn(__ull2float_rn(b.sum_k[r]), (float)n);
			int n_tot = en - st + 1;
			if ((float)g.qs > avg_k && (float)g.rs > avg_k) ++n_tot;
			if ((float)(qlen - g.qs) > avg_k && (float)(b.ref_len[g.rid] - g.re) > avg_k) ++n_tot;
			res = make_int2(n_match, n_tot);
		}
		if (gl == 0) b.out[h] = res;
	}
}

void launch_est_err(const EstErrBatch &b, hipStream_t s)
{
	if (b.n_reads <= 0) return;
	const int per = EE_WG / 64;
	const int64_t cap = ((int64_t)b.grid_waves + per - 1) / per;
	hipLaunchKernelGGL(k_est_err_reads, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((b.n_reads + per - 1) / per, cap))), dim3(EE_WG), 0, s, b);
	if (b.n_regs <= 0) return;
	hipLaunchKernelGGL(k_est_err<64>, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((b.n_regs + per - 1) / per, cap))), dim3(EE_WG), 0, s, b);
	hipLaunchKernelGGL(k_est_err<16>, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((b.n_regs + 15) / 16, cap))), dim3(EE_WG), 0, s, b);
}

} // namespace mm2gb
