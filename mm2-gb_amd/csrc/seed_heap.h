// seed_heap.h -- internal: seed matches -> anchors in the order collect_seed_hits_heap leaves them (map.c:229-293; MM_F_HEAP_SORT, the short-read preset).
// The host form (seed_heap_host.cpp) is the definition; the device form (seed_heap_kernels.hip) sorts a read's hits by (cr, seed, k) and is exact for every
// read in which no two hits carry the same cr -- a read with such a pair is flagged and done again by the host form.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mm2gb_chain.h"
#include "post_dev.h"

namespace mm2gb {

// One read through collect_seed_hits_heap with ks_heapmake / ks_heapdown (ksort.h:43-59): seeds[0 .. n_seeds) with hits[hit_off[k] .. hit_off[k+1]) (hit_off: the
// batch's, n_seeds + 1 entries from the read's first seed on).  names: the name tests run with q_rank / ref_rank / ref_len (skip_seed, map.c:208-219).  out must hold
// the read's hits; returns the number of anchors.  *tied (may be null): two of the read's hits carry the same cr.
int64_t collect_seeds_heap_read(int64_t opt_flag, int64_t n_seeds, const mm2gb_seed_t *seeds, const int64_t *hit_off, const uint64_t *hits, int32_t qlen, bool names,
                                int32_t q_rank, const int32_t *ref_len, const int32_t *ref_rank, mm2gb_anchor_t *out, bool *tied);

// A read of at most this many hits is sorted by one wave in LDS: 1024 x (8-byte cr + 4-byte index) = 12 KiB a wave, 48 KiB a workgroup of four, so three
// workgroups -- twelve waves -- share a CU's 160 KiB.  A longer read goes through rocprim::segmented_radix_sort_pairs.
constexpr int HEAP_WAVE_HITS = 1024;

struct HeapBatch {
	const SeedRecord *seeds;           // as SeedBatch (post_dev.h)
	const int64_t *seed_off, *hit_off;
	const unsigned long long *hits;
	const int32_t *qlen, *q_rank, *ref_len, *ref_rank;
	int64_t        n_reads, n_seeds, n_hits;   // n_hits < 2^31
	long long      flag;               // MM_F_NO_DIAG | MM_F_NO_DUAL | MM_F_FOR_ONLY | MM_F_REV_ONLY
	uint32_t      *ord;                // scratch, n_hits: a read's hits (their indices in hits[]) in (cr, seed, k) order, at the read's hits' place
	unsigned long long *keys;          // scratch, n_hits: the long reads' sorted cr (unused otherwise)
	const int64_t *long_begin, *long_end;      // the long reads' ranges of hits[], n_long each
	int64_t        n_long;
	void          *sort_tmp;           // heap_sort_tmp_bytes(n_hits, n_long, n_reads)
	size_t         sort_tmp_bytes;
	ulonglong2    *tmp;                // scratch, n_hits: a read's anchors at its hits' place
	int32_t       *n_kept;             // scratch, n_reads
	int32_t       *tied;               // out, n_reads: 1 where two of the read's hits carry the same cr
	int64_t       *anchor_off;         // out, n_reads + 1
	ulonglong2    *out;                // out, n_hits: the reads' anchors back to back
	int            grid_waves;
};
size_t heap_sort_tmp_bytes(int64_t n_hits, int64_t n_long, int64_t n_reads);
int    launch_collect_seeds_heap(const HeapBatch &b, hipStream_t s);   // -1: the library sort refused

} // namespace mm2gb
