// window_check.hip -- test entry point: the range pass (k_block_reads + k_window) alone on a caller's batch, and everything it wrote.
// Not used by the engine; tests/test_gpu_window.py checks st[], the per-block planner words and the input flags against their definitions.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "chain_dev.h"

using namespace mm2gb;

extern "C" int mm2gb_window_check(int64_t n, int64_t n_reads, const void *anchors /* n x 16 B */, const int64_t *offsets /* n_reads + 1 */,
                                  int max_dist_x, int max_iter, int32_t *st /* n */, int32_t *firstcut, int64_t *pairs, int32_t *clamped,
                                  int32_t *wmax /* 2 per block */, unsigned *flags /* 1 */)
{
	if (n <= 0 || n_reads <= 0) return -1;
	const int64_t nb = (n + PLAN_BLOCK - 1) / PLAN_BLOCK;
	DevBatch b;
	memset(&b, 0, sizeof b);
	DevParams P;
	memset(&P, 0, sizeof P);
	P.max_dist_x = max_dist_x;
	P.max_iter = max_iter;
	void *d_raw = nullptr, *d_off = nullptr, *d_st = nullptr, *d_fc = nullptr, *d_pairs = nullptr, *d_cl = nullptr, *d_rd = nullptr,
	     *d_wmax = nullptr, *d_flags = nullptr;
	int rc = -1;
	if (hipMalloc(&d_raw, n * 16) != hipSuccess || hipMalloc(&d_off, (n_reads + 1) * 8) != hipSuccess || hipMalloc(&d_st, n * 4) != hipSuccess ||
	    hipMalloc(&d_fc, nb * 4) != hipSuccess || hipMalloc(&d_pairs, nb * 8) != hipSuccess || hipMalloc(&d_cl, nb * 4) != hipSuccess ||
	    hipMalloc(&d_rd, nb * 4) != hipSuccess || hipMalloc(&d_wmax, nb * 8) != hipSuccess || hipMalloc(&d_flags, 16) != hipSuccess)
		goto done;
	if (hipMemcpy(d_raw, anchors, n * 16, hipMemcpyHostToDevice) != hipSuccess ||
	    hipMemcpy(d_off, offsets, (n_reads + 1) * 8, hipMemcpyHostToDevice) != hipSuccess || hipMemset(d_flags, 0, 16) != hipSuccess)
		goto done;
	b.raw = (const uint4*)d_raw; b.offsets = (const int64_t*)d_off; b.n = n; b.n_reads = n_reads;
	b.st = (int32_t*)d_st; b.blk_firstcut = (int32_t*)d_fc; b.blk_pairs = (int64_t*)d_pairs; b.blk_clamped = (int32_t*)d_cl;
	b.blk_read = (int32_t*)d_rd; b.blk_wmax = (int32_t*)d_wmax; b.n_blocks = nb; b.flags = (unsigned*)d_flags;
	launch_window(b, P, 0);
	if (hipDeviceSynchronize() != hipSuccess) goto done;
	if (hipMemcpy(st, d_st, n * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(firstcut, d_fc, nb * 4, hipMemcpyDeviceToHost) != hipSuccess ||
	    hipMemcpy(pairs, d_pairs, nb * 8, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(clamped, d_cl, nb * 4, hipMemcpyDeviceToHost) != hipSuccess ||
	    hipMemcpy(wmax, d_wmax, nb * 8, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(flags, d_flags, 4, hipMemcpyDeviceToHost) != hipSuccess)
		goto done;
	rc = 0;
done:
	for (void *p : {d_raw, d_off, d_st, d_fc, d_pairs, d_cl, d_rd, d_wmax, d_flags}) if (p) (void)hipFree(p);
	return rc;
}
