// seed_heap_kernels.hip -- seed matches -> anchors in the order collect_seed_hits_heap leaves them (map.c:229-293; MM_F_HEAP_SORT, the short-read preset).
//
// The reference merges the seeds' sorted hit lists through a binary min-heap on cr: the hits come out in ascending cr, the forward-strand ones are
// appended, the reverse-strand ones filled from the back and reversed -- so the result is the forward anchors in pop order, then the reverse anchors in
// pop order.  Where every cr of a read is distinct the pop order IS the ascending order, whatever the heap does; among equal cr (one minimizer value at
// two places of the read: both seeds carry the same list) it is the heap's own, and ks_heapdown moves a child with an equal key up, so it is not the seed
// order.  Here a read's hits are sorted by (cr, seed, k) -- a hit's index in hits[] orders (seed, k) --, a read with two equal cr is flagged, and the
// caller does a flagged read again with the host form (seed_heap_host.cpp, the definition).
//
//   k_heap_sort_wave   per read of at most HEAP_WAVE_HITS hits: one wave sorts (cr, index) in LDS (a bitonic network: the pairs are distinct, so its order is total)
//   (rocprim)          the longer reads: segmented_radix_sort_pairs on cr with the index as value (stable, and the indices go in ascending)
//   k_heap_emit        per read: the sorted hits through skip_seed (map.c:205-227), the anchors of map.c:256-267 forward first, the tie flag
//   (rocprim) / k_heap_total / k_heap_pack   the reads back to back: their offsets by a device-wide exclusive scan of the kept counts
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <rocprim/device/device_segmented_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>
#include "seed_heap.h"

namespace mm2gb {

namespace {

constexpr int W = 64;
constexpr int HEAP_THREADS = 256;               // 4 waves, one read each

__device__ __forceinline__ int lane() { return threadIdx.x & (W - 1); }
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ void wave_sync()
{
	// LDS and global accesses of one wave are issued in order; the fence keeps the compiler from moving them across phases
	__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
	__builtin_amdgcn_wave_barrier();
}

struct alignas(16) HeapLds {
	unsigned long long key[HEAP_WAVE_HITS];
	uint32_t idx[HEAP_WAVE_HITS];
};
static_assert(sizeof(HeapLds) * (HEAP_THREADS / W) <= 48 * 1024, "three workgroups to a CU's 160 KiB of LDS");

} // namespace

__global__ __launch_bounds__(HEAP_THREADS) void k_heap_sort_wave(HeapBatch b)
{
	__shared__ HeapLds lds[HEAP_THREADS / W];
	HeapLds &L = lds[threadIdx.x / W];
	const int per = HEAP_THREADS / W, l = lane();
	for (int64_t r = (int64_t)blockIdx.x * per + uni(threadIdx.x / W); r < b.n_reads; r += (int64_t)gridDim.x * per) {
		const int64_t h0 = b.hit_off[b.seed_off[r]], h1 = b.hit_off[b.seed_off[r + 1]];
		if (h1 - h0 <= 0 || h1 - h0 > HEAP_WAVE_HITS) continue;
		const int n = (int)(h1 - h0);
		int P = W;
		while (P < n) P <<= 1;                                   // (P <= HEAP_WAVE_HITS, a power of two)
		// padding sorts last: no cr is larger, and where one is equal the padding's index is
		for (int i = l; i < P; i += W) { L.key[i] = i < n ? b.hits[h0 + i] : ~0ull; L.idx[i] = (uint32_t)i; }
		wave_sync();
		for (int k = 2; k <= P; k <<= 1)
			for (int j = k >> 1; j > 0; j >>= 1) {
				for (int t = l; t < P / 2; t += W) {
					const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), o = i | j;      // i < o < P
					const unsigned long long ki = L.key[i], ko = L.key[o];
					const uint32_t xi = L.idx[i], xo = L.idx[o];
					const bool gt = ki > ko || (ki == ko && xi > xo);
					if (((i & k) == 0) == gt) { L.key[i] = ko; L.key[o] = ki; L.idx[i] = xo; L.idx[o] = xi; }
				}
				wave_sync();
			}
		for (int i = l; i < n; i += W) b.ord[h0 + i] = (uint32_t)(h0 + L.idx[i]);
		wave_sync();
	}
}

__global__ __launch_bounds__(HEAP_THREADS) void k_heap_emit(HeapBatch b)
{
	constexpr long long F_NO_DIAG = 0x001, F_NO_DUAL = 0x002, F_FOR_ONLY = 0x100000, F_REV_ONLY = 0x200000;   // minimap.h:8-9,28-29
	const int per = HEAP_THREADS / W, l = lane();
	const unsigned long long below = (1ull << l) - 1;
	for (int64_t r = (int64_t)blockIdx.x * per + uni(threadIdx.x / W); r < b.n_reads; r += (int64_t)gridDim.x * per) {
		const int64_t s0 = b.seed_off[r], s1 = b.seed_off[r + 1];
		const int64_t h0 = b.hit_off[s0], n = b.hit_off[s1] - h0;
		const int qlen = b.qlen[r];
		const bool names = b.q_rank && (b.flag & (F_NO_DIAG | F_NO_DUAL));
		const int qr = names ? b.q_rank[r] : 0;
		bool tied = false;
		int64_t n_for = 0, n_rev = 0;
		for (int pass = 0; pass < 2; ++pass) {                   // 0: the forward anchors counted (the reverse ones begin behind them), 1: written
			int64_t f = 0, v = 0;
			for (int64_t base = 0; base < n; base += W) {
				const int64_t i = base + l;
				bool keep = false, fwd = false;
				ulonglong2 a = make_ulonglong2(0, 0);
				if (i < n) {
					const int64_t h = b.ord[h0 + i];
					const unsigned long long cr = b.hits[h];
					if (pass == 0 && i > 0 && b.hits[b.ord[h0 + i - 1]] == cr) tied = true;
					int64_t lo = s0, hi = s1;                    // invariant: hit_off[lo] <= h < hit_off[hi]  (seeds without hits are passed over)
					while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (b.hit_off[mid] <= h) lo = mid; else hi = mid; }
					const SeedRecord q = b.seeds[lo];
					const unsigned q_span = q.span_flt & 0x7fffffffu, seg_id = q.seg_tandem & 0x7fffffffu;
					const int rpos = (int)((unsigned)cr >> 1);
					fwd = (cr & 1) == (q.q_pos & 1);
					bool skip = false, is_self = false;
					if (names) {                                                                // map.c:208-219
						const int rid = (int)(cr >> 32), rr = b.ref_rank[rid];
						if ((b.flag & F_NO_DIAG) && qr == rr && b.ref_len[rid] == qlen) {
							if ((unsigned)cr >> 1 == (q.q_pos >> 1)) skip = true;
							else if (fwd) is_self = true;
						}
						if (!skip && (b.flag & F_NO_DUAL) && qr > rr) skip = true;
					}
					if (!skip && (b.flag & (F_FOR_ONLY | F_REV_ONLY))) skip = fwd ? (b.flag & F_REV_ONLY) != 0 : (b.flag & F_FOR_ONLY) != 0;   // map.c:220-226
					keep = !skip;
					if (fwd) {                                                                  // map.c:257-259
						a.x = (cr & 0xffffffff00000000ULL) | (unsigned)rpos;
						a.y = (unsigned long long)q_span << 32 | q.q_pos >> 1;
					} else {                                                                    // map.c:261-263
						a.x = 1ULL << 63 | (cr & 0xffffffff00000000ULL) | (unsigned)rpos;
						a.y = (unsigned long long)q_span << 32 | (unsigned)(qlen - (int)((q.q_pos >> 1) + 1 - q_span) - 1);
					}
					a.y |= (unsigned long long)seg_id << 48;                                    // MM_SEED_SEG_SHIFT
					if (q.seg_tandem >> 31) a.y |= 1ULL << 42;                                  // MM_SEED_TANDEM
					if (is_self) a.y |= 1ULL << 43;                                             // MM_SEED_SELF
				}
				const unsigned long long mf = __ballot(keep && fwd), mr = __ballot(keep && !fwd);
				if (pass == 1 && keep) b.tmp[h0 + (fwd ? f + __popcll(mf & below) : n_for + v + __popcll(mr & below))] = a;      // (below h0 + n: n_for + n_rev <= n)
				f += __popcll(mf); v += __popcll(mr);
			}
			if (pass == 0) { n_for = f; n_rev = v; }
		}
		const bool any_tied = __ballot(tied) != 0;
		if (l == 0) { b.n_kept[r] = (int32_t)(n_for + n_rev); b.tied[r] = any_tied ? 1 : 0; }
	}
}

// the reads' offsets are a device-wide exclusive scan of n_kept (rocprim: a batch is millions of short reads); this closes the array
__global__ void k_heap_total(HeapBatch b)
{
	if (blockIdx.x == 0 && threadIdx.x == 0) b.anchor_off[b.n_reads] = b.anchor_off[b.n_reads - 1] + b.n_kept[b.n_reads - 1];
}

__global__ __launch_bounds__(HEAP_THREADS) void k_heap_pack(HeapBatch b)
{
	const int per = HEAP_THREADS / W, l = lane();
	for (int64_t r = (int64_t)blockIdx.x * per + uni(threadIdx.x / W); r < b.n_reads; r += (int64_t)gridDim.x * per) {
		const int64_t h0 = b.hit_off[b.seed_off[r]], o0 = b.anchor_off[r];
		const int n = b.n_kept[r];
		for (int j = l; j < n; j += W) b.out[o0 + j] = b.tmp[h0 + j];
	}
}

namespace {
struct KeptAsOffset { __host__ __device__ long long operator()(int32_t v) const { return v; } };
inline hipError_t scan_offsets(void *tmp, size_t &bytes, const int32_t *n_kept, int64_t *anchor_off, int64_t n_reads, hipStream_t s)
{
	return rocprim::exclusive_scan(tmp, bytes, rocprim::make_transform_iterator(n_kept, KeptAsOffset()), (long long*)anchor_off, 0LL, (size_t)n_reads, rocprim::plus<long long>(), s);
}
}

// the library calls' scratch: the long reads' sort and the offsets' scan run one after the other on one stream and share it
size_t heap_sort_tmp_bytes(int64_t n_hits, int64_t n_long, int64_t n_reads)
{
	size_t bytes = 0, scan = 0;
	(void)scan_offsets(nullptr, scan, nullptr, nullptr, std::max<int64_t>(n_reads, 1), (hipStream_t)nullptr);
	scan = std::max<size_t>(scan, 16);
	if (n_long <= 0) return scan;
	(void)rocprim::segmented_radix_sort_pairs(nullptr, bytes, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, rocprim::make_counting_iterator<uint32_t>(0u), (uint32_t*)nullptr,
	                                          (unsigned)std::max<int64_t>(n_hits, 1), (unsigned)n_long, (const int64_t*)nullptr, (const int64_t*)nullptr, 0, 64, (hipStream_t)nullptr);
	return std::max(bytes, scan);
}

int launch_collect_seeds_heap(const HeapBatch &b, hipStream_t s)
{
	if (b.n_reads <= 0) return 0;
	const int per = HEAP_THREADS / W;
	const unsigned rgrid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((b.n_reads + per - 1) / per, ((int64_t)b.grid_waves + per - 1) / per));
	if (b.n_long > 0) {
		// the values are the hits' own indices (a counting iterator): a long read's range of ord[] receives them in (cr, index) order, nothing outside the ranges is written
		size_t tmp = b.sort_tmp_bytes;
		if (rocprim::segmented_radix_sort_pairs(b.sort_tmp, tmp, b.hits, b.keys, rocprim::make_counting_iterator<uint32_t>(0u), b.ord, (unsigned)b.n_hits, (unsigned)b.n_long,
		                                        b.long_begin, b.long_end, 0, 64, s) != hipSuccess) return -1;
	}
	hipLaunchKernelGGL(k_heap_sort_wave, dim3(rgrid), dim3(HEAP_THREADS), 0, s, b);
	hipLaunchKernelGGL(k_heap_emit, dim3(rgrid), dim3(HEAP_THREADS), 0, s, b);
	size_t tmp = b.sort_tmp_bytes;
	if (scan_offsets(b.sort_tmp, tmp, b.n_kept, b.anchor_off, b.n_reads, s) != hipSuccess) return -1;
	hipLaunchKernelGGL(k_heap_total, dim3(1), dim3(64), 0, s, b);
	hipLaunchKernelGGL(k_heap_pack, dim3(rgrid), dim3(HEAP_THREADS), 0, s, b);
	return 0;
}

} // namespace mm2gb
