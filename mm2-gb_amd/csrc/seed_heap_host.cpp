// seed_heap_host.cpp -- seed matches -> anchors in the order collect_seed_hits_heap leaves them (map.c:229-293; MM_F_HEAP_SORT, the short-read preset): the host
// form, which is the definition of the device form (seed_heap_kernels.hip) and what that form's caller does a read with two equal cr again with.  Host code only:
// nothing of the HIP runtime is called, so the unit links into a stand-alone program (tests/tools/sr_replay.cpp).
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>
#include "host_threads.h"
#include "seed_heap.h"

namespace mm2gb { int fail(const std::string &msg); }

// collect_seed_hits_heap (map.c:229-293) for one read: a binary min-heap on cr (heap_lt, map.c:202) with the payload seed << 32 | k, made and sifted as
// ks_heapmake / ks_heapdown do (ksort.h:43-59: of two children the right one only where it is strictly smaller, and a child moves up unless it is strictly
// larger than the element sifted -- so among equal cr the order is the heap's own).  Forward hits are appended in pop order; reverse ones are filled from the
// back, reversed and closed up (map.c:282-291), which leaves them in pop order behind the forward ones.
namespace mm2gb {
int64_t collect_seeds_heap_read(int64_t opt_flag, int64_t n_seeds, const mm2gb_seed_t *seeds, const int64_t *hit_off, const uint64_t *hits, int32_t qlen, bool names,
                                int32_t q_rank, const int32_t *ref_len, const int32_t *ref_rank, mm2gb_anchor_t *out, bool *tied)
{
	constexpr int64_t F_NO_DIAG = 0x001, F_NO_DUAL = 0x002, F_FOR_ONLY = 0x100000, F_REV_ONLY = 0x200000;   // minimap.h:8-9,28-29
	struct Node { uint64_t x, y; };
	const int64_t n_a = n_seeds > 0 ? hit_off[n_seeds] - hit_off[0] : 0;
	if (tied) *tied = false;
	if (n_a == 0) return 0;
	std::vector<Node> heap;
	heap.reserve((size_t)n_seeds);
	for (int64_t i = 0; i < n_seeds; ++i) if (seeds[i].n > 0) heap.push_back({ hits[hit_off[i]], (uint64_t)i << 32 });
	size_t heap_size = heap.size();
	Node *l = heap.data();
	auto heapdown = [&](size_t i, size_t n) {                // ksort.h:43-53 with heap_lt(a, b) = a.x > b.x
		size_t k = i;
		const Node tmp = l[i];
		while ((k = (k << 1) + 1) < n) {
			if (k != n - 1 && l[k].x > l[k + 1].x) ++k;
			if (l[k].x > tmp.x) break;
			l[i] = l[k]; i = k;
		}
		l[i] = tmp;
	};
	for (size_t i = (heap_size >> 1) - 1; i != (size_t)-1; --i) heapdown(i, heap_size);     // ksort.h:54-59
	int64_t n_for = 0, n_rev = 0;
	uint64_t last = 0;
	bool any = false;
	while (heap_size > 0) {
		const mm2gb_seed_t &q = seeds[l[0].y >> 32];
		const uint64_t rr = l[0].x;
		if (any && rr == last && tied) *tied = true;          // (pops never descend: equal cr come out one after the other)
		last = rr; any = true;
		const int32_t rpos = (int32_t)((uint32_t)rr >> 1);
		const bool same_strand = (rr & 1) == (q.q_pos & 1);
		const uint32_t q_span = q.span_flt & 0x7fffffffu, seg_id = q.seg_tandem & 0x7fffffffu;
		bool skip = false, is_self = false;
		if (names) {                                                                      // map.c:208-219
			const int32_t rid = (int32_t)(rr >> 32);
			if ((opt_flag & F_NO_DIAG) && q_rank == ref_rank[rid] && ref_len[rid] == qlen) {
				if ((uint32_t)rr >> 1 == (q.q_pos >> 1)) skip = true;
				else if (same_strand) is_self = true;
			}
			if (!skip && (opt_flag & F_NO_DUAL) && q_rank > ref_rank[rid]) skip = true;
		}
		if (!skip && (opt_flag & (F_FOR_ONLY | F_REV_ONLY))) skip = same_strand ? (opt_flag & F_REV_ONLY) != 0 : (opt_flag & F_FOR_ONLY) != 0;   // map.c:220-226
		if (!skip) {
			mm2gb_anchor_t *p;
			if (same_strand) {                                                            // map.c:256-259
				p = &out[n_for++];
				p->x = (rr & 0xffffffff00000000ULL) | (uint32_t)rpos;
				p->y = (uint64_t)q_span << 32 | q.q_pos >> 1;
			} else {                                                                      // map.c:260-263
				p = &out[n_a - (++n_rev)];
				p->x = 1ULL << 63 | (rr & 0xffffffff00000000ULL) | (uint32_t)rpos;
				p->y = (uint64_t)q_span << 32 | (uint32_t)(qlen - (int32_t)((q.q_pos >> 1) + 1 - q_span) - 1);
			}
			p->y |= (uint64_t)seg_id << 48;                                                // MM_SEED_SEG_SHIFT
			if (q.seg_tandem >> 31) p->y |= 1ULL << 42;                                    // MM_SEED_TANDEM
			if (is_self) p->y |= 1ULL << 43;                                               // MM_SEED_SELF
		}
		if ((uint32_t)l[0].y < q.n - 1) {                                                 // map.c:270-277
			++l[0].y;
			l[0].x = hits[hit_off[l[0].y >> 32] + (uint32_t)l[0].y];
		} else {
			l[0] = l[heap_size - 1];
			--heap_size;
		}
		if (heap_size > 0) heapdown(0, heap_size);
	}
	std::reverse(out + (n_a - n_rev), out + n_a);                                          // map.c:283-287
	if (n_a > n_for + n_rev) memmove(out + n_for, out + (n_a - n_rev), (size_t)n_rev * sizeof(mm2gb_anchor_t));
	return n_for + n_rev;
}
} // namespace mm2gb

using namespace mm2gb;

extern "C" {

// collect_seed_hits_heap (map.c:229-293) on host threads: the definition of mm2gb_collect_seeds_heap_gpu
int mm2gb_collect_seeds_heap_host(int64_t opt_flag, int64_t n_reads, const int64_t *seed_off, const mm2gb_seed_t *seeds, const int64_t *hit_off,
                                  const uint64_t *hits, const int32_t *qlen, const int32_t *q_rank, int32_t n_ref, const int32_t *ref_len,
                                  const int32_t *ref_rank, int n_threads, int64_t *anchor_off, mm2gb_anchor_t *anchors, int64_t *n_tied_reads)
{
	constexpr int64_t F_NO_DIAG = 0x001, F_NO_DUAL = 0x002, F_QSTRAND = 0x100000000LL;
	if (n_tied_reads) *n_tied_reads = 0;
	if (opt_flag & F_QSTRAND) return fail("mm2gb_collect_seeds_heap_host: MM_F_QSTRAND is not supported (collect_seed_hits_heap has no such branch)");
	if (n_reads < 0 || !seed_off || !anchor_off || seed_off[0] != 0) return fail("mm2gb_collect_seeds_heap_host: seed_off[0] must be 0");
	anchor_off[0] = 0;
	if (n_reads == 0) return 0;
	for (int64_t r = 0; r < n_reads; ++r) if (seed_off[r + 1] < seed_off[r]) return fail("mm2gb_collect_seeds_heap_host: seed_off must be non-decreasing");
	const int64_t n_seeds = seed_off[n_reads];
	if (!qlen || !hit_off || (n_seeds > 0 && !seeds) || hit_off[0] != 0) return fail("mm2gb_collect_seeds_heap_host: null argument, or hit_off[0] is not 0");
	for (int64_t k = 0; k < n_seeds; ++k) if (hit_off[k + 1] - hit_off[k] != (int64_t)seeds[k].n) return fail("mm2gb_collect_seeds_heap_host: hit_off does not match the seeds' hit counts");
	const bool names = (opt_flag & (F_NO_DIAG | F_NO_DUAL)) != 0 && q_rank != nullptr;
	if (names && (!ref_rank || n_ref <= 0)) return fail("mm2gb_collect_seeds_heap_host: NO_DIAG / NO_DUAL need ref_rank");
	if (names && (opt_flag & F_NO_DIAG) && !ref_len) return fail("mm2gb_collect_seeds_heap_host: NO_DIAG needs ref_len");
	if (hit_off[n_seeds] > 0 && (!hits || !anchors)) return fail("mm2gb_collect_seeds_heap_host: null buffer");
	if (names)
		for (int64_t h = 0; h < hit_off[n_seeds]; ++h) if ((int64_t)(hits[h] >> 32) >= n_ref) return fail("mm2gb_collect_seeds_heap_host: a hit names a reference sequence >= n_ref");
	// every read writes at its hits' offset first (an upper bound of where it ends up) and is moved down afterwards
	std::vector<int64_t> kept((size_t)n_reads, 0);
	std::vector<unsigned char> tied((size_t)n_reads, 0);
	for_each_on_threads((size_t)n_reads, n_threads, 16, [&](size_t r) {
		bool t = false;
		kept[r] = collect_seeds_heap_read(opt_flag, seed_off[r + 1] - seed_off[r], seeds + seed_off[r], hit_off + seed_off[r], hits, qlen[r], names, names ? q_rank[r] : 0, ref_len, ref_rank,
		                                  anchors + hit_off[seed_off[r]], &t);
		tied[r] = t;
	});
	for (int64_t r = 0; r < n_reads; ++r) {
		anchor_off[r + 1] = anchor_off[r] + kept[(size_t)r];
		const int64_t from = hit_off[seed_off[r]];
		if (from != anchor_off[r] && kept[(size_t)r] > 0) memmove(anchors + anchor_off[r], anchors + from, (size_t)kept[(size_t)r] * sizeof(mm2gb_anchor_t));
		if (n_tied_reads) *n_tied_reads += tied[(size_t)r];
	}
	return 0;
}

} // extern "C"
