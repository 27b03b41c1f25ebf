// seeding.cpp -- from sequence to seed matches, written from scratch (the producer side of the path).
//
//   sketch            (w,k)-minimizers of a sequence, the reference's definition to the letter (sketch.c:77-143, plain and homopolymer-
//                     compressed): the hash of the canonical k-mer (sketch.c:29-39), ties inside a window kept, the special first window,
//                     ambiguous bases
//   Index             every minimizer of the reference sequences -> its occurrences  rid << 32 | last_pos << 1 | strand  in ascending
//                     order: what mm_idx_get hands out (index.c:81-98; the order is that of radix_sort_64 in index.c:251), and the
//                     occurrence threshold mid_occ of mm_mapopt_update (options.c:78-84 with index.c:186-211)
//   collect_matches   mm_collect_matches (seed.c:98-131) for one read: query minimizers, the over-represented ones dropped
//                     (mm_seed_mz_flt, seed.c:5-30), every minimizer the index knows (mm_seed_collect_all, seed.c:32-54), the high-occurrence
//                     ones thinned out (mm_seed_select, seed.c:58-96), repeat length and minimizer positions
// The output of collect_matches is the input of mm2gb_collect_seeds_gpu.  One query segment per read, or the two mates of a fragment as one list (collect_matches_frag_refs).
// Host code: an index look-up per minimizer is a pointer chase through a structure the size of the genome -- not a kernel.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>
#include "engine.h"
#include "host_threads.h"
#include "host_chain.h"
#include "index_dev.h"
#include "kmer.h"

namespace mm2gb {
namespace {

struct Mini { uint64_t x, y; };            // x = hash << 8 | span, y = rid << 32 | last_pos << 1 | strand   (sketch.c:66-71)

// sketch.c:77-143.  A ring of the last w k-mers (slot = k-mer number mod w); the current minimum and
// its slot; what is emitted when, in this order: the k-mers equal to the minimum of the FIRST full window; the old minimum when a
// k-mer at least as small arrives or when it leaves the window; after a rescan, the other k-mers equal to the new minimum.
// hpc (sketch.c:94-105): a step per homopolymer run -- i jumps to the run's last base, the words take one base per run, the span is the summed
// length of the last k runs (a queue of run lengths, emptied at an ambiguous base); a k-mer of 256 bases or more has no value but counts.
void sketch(const char *seq, int len, int w, int k, uint32_t rid, bool hpc, std::vector<Mini> &out)
{
	const uint64_t none = ~0ull, mask = (1ull << 2 * k) - 1, top_shift = 2 * (k - 1);
	uint64_t fwd = 0, rev = 0;
	std::vector<Mini> ring((size_t)w, Mini{ none, none });
	Mini best{ none, none };
	int run = 0, slot = 0, best_slot = 0;       // run: valid bases since the last ambiguous one (k-mers ending here: run - k + 1)
	int run_len[32], q_front = 0, q_count = 0, hpc_span = 0;     // hpc: the lengths of the last k runs (tiny_queue_t, sketch.c:41-58) and their sum
	for (int i = 0; i < len; ++i) {
		const int c = base_code((unsigned char)seq[i]);
		Mini cur{ none, none };
		if (c < 4) {
			int span;
			if (hpc) {
				int skip_len = 1;
				while (i + skip_len < len && base_code((unsigned char)seq[i + skip_len]) == c) ++skip_len;
				i += skip_len - 1;                      // at the run's last base
				run_len[(q_front + q_count++) & 31] = skip_len;
				hpc_span += skip_len;
				if (q_count > k) { hpc_span -= run_len[q_front]; q_front = (q_front + 1) & 31; --q_count; }
				span = hpc_span;
			} else span = run + 1 < k ? run + 1 : k;
			fwd = (fwd << 2 | (uint64_t)c) & mask;
			rev = rev >> 2 | (uint64_t)(3 ^ c) << top_shift;
			if (fwd == rev) continue;               // its own reverse complement: no strand, and it does not count as a base seen
			const int strand = fwd < rev ? 0 : 1;
			++run;
			if (run >= k && span < 256) {
				cur.x = mix(strand ? rev : fwd, mask) << 8 | (uint64_t)span;
				cur.y = (uint64_t)rid << 32 | (uint64_t)(uint32_t)i << 1 | (uint64_t)strand;
			}
		} else { run = 0; q_front = q_count = 0; hpc_span = 0; }
		ring[(size_t)slot] = cur;
		auto twins = [&](int from, int to) {     // k-mers in slots [from, to) with the minimum's value at another position
			for (int j = from; j < to; ++j)
				if (ring[(size_t)j].x == best.x && ring[(size_t)j].y != best.y) out.push_back(ring[(size_t)j]);
		};
		if (run == w + k - 1 && best.x != none) { twins(slot + 1, w); twins(0, slot); }     // the first full window
		if (cur.x <= best.x) {                     // at least as small: the old minimum is done
			if (run >= w + k && best.x != none) out.push_back(best);
			best = cur; best_slot = slot;
		} else if (slot == best_slot) {            // the minimum leaves the window
			if (run >= w + k - 1 && best.x != none) out.push_back(best);
			best.x = none;
			for (int j = slot + 1; j < w; ++j) if (ring[(size_t)j].x <= best.x) { best = ring[(size_t)j]; best_slot = j; }   // oldest first, later wins ties
			for (int j = 0; j <= slot; ++j) if (ring[(size_t)j].x <= best.x) { best = ring[(size_t)j]; best_slot = j; }
			if (run >= w + k - 1 && best.x != none) { twins(slot + 1, w); twins(0, slot + 1); }
		}
		if (++slot == w) slot = 0;
	}
	if (best.x != none) out.push_back(best);    // sketch.c:141-142
}

// (struct SeedIndex, the index itself, is in index_dev.h: index_kernels.hip fills the same structure on a device)

// max-heap of 64-bit values, sift-down as in ksort.h:43-59.  (Where an element sits does not decide the outcome: a replacement needs a strictly
// smaller n and evicts the largest (n, index), so a streak keeps its K smallest by (n, index) -- the form k_m_select computes on the device)
void sift_down(size_t i, size_t n, uint64_t *h)
{
	const uint64_t v = h[i];
	for (size_t c = 2 * i + 1; c < n; c = 2 * i + 1) {
		if (c + 1 < n && h[c] < h[c + 1]) ++c;
		if (h[c] < v) break;
		h[i] = h[c]; i = c;
	}
	h[i] = v;
}

struct Match { uint32_t n, q_pos, q_span, seg_id; bool flt, tandem; const uint64_t *cr; };

// seed.c:58-96: inside every streak of minimizers that occur more than max_occ times, keep the max_high_occ rarest -- one per
// `dist` bases of the streak -- and never one that occurs more than max_max_occ times
void thin_out(std::vector<Match> &m, int qlen, int max_occ, int max_max_occ, int dist)
{
	const int n = (int)m.size();
	if (n < 2) return;
	bool any = false;
	for (const Match &q : m) any |= q.n > (uint32_t)max_occ;
	if (!any) return;
	uint64_t heap[128];
	for (int i = 0, last_low = -1; i <= n; ++i) {
		if (i < n && m[(size_t)i].n > (uint32_t)max_occ) continue;
		if (i - last_low > 1) {                    // the streak (last_low, i)
			const int from = last_low + 1, to = i;
			const int ps = last_low < 0 ? 0 : (int)(m[(size_t)last_low].q_pos >> 1), pe = i == n ? qlen : (int)(m[(size_t)i].q_pos >> 1);
			int keep = (int)((double)(pe - ps) / dist + .499);
			if (keep > 0) {
				if (keep > 128) keep = 128;
				int j = from, filled = 0;
				for (; j < to && filled < keep; ++j, ++filled) heap[filled] = (uint64_t)m[(size_t)j].n << 32 | (uint32_t)j;
				for (size_t s = (size_t)filled / 2; s-- > 0;) sift_down(s, (size_t)filled, heap);
				for (; j < to; ++j)
					if ((int32_t)m[(size_t)j].n < (int32_t)(heap[0] >> 32)) { heap[0] = (uint64_t)m[(size_t)j].n << 32 | (uint32_t)j; sift_down(0, (size_t)filled, heap); }
				for (int s = 0; s < filled; ++s) m[(size_t)(uint32_t)heap[s]].flt = true;
			}
			for (int j = from; j < to; ++j) m[(size_t)j].flt = !m[(size_t)j].flt;
			for (int j = from; j < to; ++j) if (m[(size_t)j].n > (uint32_t)max_max_occ) m[(size_t)j].flt = true;
		}
		last_low = i;
	}
}

} // namespace
} // namespace mm2gb

using namespace mm2gb;

extern "C" {

int mm2gb_sketch(const char *seq, int32_t len, int w, int k, uint32_t rid, uint64_t **out_xy, int64_t *n_out)
{
	return mm2gb_sketch_flag(seq, len, w, k, rid, 0, out_xy, n_out);
}

int mm2gb_sketch_flag(const char *seq, int32_t len, int w, int k, uint32_t rid, int flag, uint64_t **out_xy, int64_t *n_out)
{
	if (!seq || !out_xy || !n_out || len < 0 || w < 1 || w > 255 || k < 1 || k > 28) return fail("mm2gb_sketch: bad arguments (0 < w < 256, 0 < k <= 28)");
	if (flag & ~MM2GB_I_HPC) return fail("mm2gb_sketch: unknown flag (MM2GB_I_HPC only)");
	std::vector<Mini> v;
	if (len > 0) sketch(seq, len, w, k, rid, (flag & MM2GB_I_HPC) != 0, v);
	*n_out = (int64_t)v.size();
	*out_xy = (uint64_t*)malloc((v.size() + 1) * 16);
	if (!*out_xy) return fail("mm2gb_sketch: out of memory");
	if (!v.empty()) memcpy(*out_xy, v.data(), v.size() * 16);
	return 0;
}

mm2gb_index_t *mm2gb_index_build(int k, int w, int32_t n_seq, const char *const *seqs, const int32_t *lens, int n_threads)
{
	return mm2gb_index_build_flag(k, w, 0, n_seq, seqs, lens, n_threads);
}

int mm2gb_index_flag(const mm2gb_index_t *ix_)
{
	const SeedIndex *ix = reinterpret_cast<const SeedIndex*>(ix_);
	return ix ? ix->flag : fail("mm2gb_index_flag: null argument");
}

mm2gb_index_t *mm2gb_index_build_flag(int k, int w, int flag, int32_t n_seq, const char *const *seqs, const int32_t *lens, int n_threads)
{
	if (n_seq < 0 || (n_seq > 0 && (!seqs || !lens)) || w < 1 || w > 255 || k < 1 || k > 28) { fail("mm2gb_index_build: bad arguments (0 < w < 256, 0 < k <= 28)"); return nullptr; }
	if (flag & ~MM2GB_I_HPC) { fail("mm2gb_index_build: unknown flag (MM2GB_I_HPC only)"); return nullptr; }
	SeedIndex *ix = new SeedIndex;
	ix->k = k; ix->w = w; ix->flag = flag;
	const bool hpc = (flag & MM2GB_I_HPC) != 0;
	ix->lens.assign(lens, lens + n_seq);
	std::vector<std::vector<Mini>> per((size_t)n_seq);
	for_each_on_threads((size_t)n_seq, n_threads, 1, [&](size_t s) { if (lens[s] > 0) sketch(seqs[s], lens[s], w, k, (uint32_t)s, hpc, per[s]); });
	size_t total = 0;
	for (auto &v : per) total += v.size();
	std::vector<Mini> all;
	all.reserve(total);
	for (auto &v : per) { all.insert(all.end(), v.begin(), v.end()); std::vector<Mini>().swap(v); }
	// by minimizer (span apart: x >> 8, index.c:229), then by occurrence (index.c:251)
	std::sort(all.begin(), all.end(), [](const Mini &a, const Mini &b) { return (a.x >> 8) != (b.x >> 8) ? (a.x >> 8) < (b.x >> 8) : a.y < b.y; });
	ix->where.resize(all.size());
	for (size_t i = 0; i < all.size(); ++i) {
		if (i == 0 || (all[i].x >> 8) != (all[i - 1].x >> 8)) { ix->keys.push_back(all[i].x >> 8); ix->first.push_back((int64_t)i); }
		ix->where[i] = all[i].y;
	}
	ix->first.push_back((int64_t)all.size());
	if (ix->keys.size() >= ((size_t)1 << 32)) { delete ix; fail("mm2gb_index_build: more than 2^32 distinct minimizers"); return nullptr; }
	ix->build_buckets();
	return reinterpret_cast<mm2gb_index_t*>(ix);
}

void mm2gb_index_destroy(mm2gb_index_t *ix_)
{
	SeedIndex *ix = reinterpret_cast<SeedIndex*>(ix_);
	if (!ix) return;
	// the device copies go the way of the engines' outgrown arenas: freed later, not under other engines' kernels (engine.hip)
	for (const SeedIndex::DevCopy &c : ix->dev) for (int a = 0; a < 4; ++a) retire_device_buffer(c.ptr[a], c.bytes[a]);
	delete ix;
}

int mm2gb_index_to_device(mm2gb_index_t *ix, int device)
{
	DevIndexView view;
	return index_on_device(ix, device, &view);
}

int64_t mm2gb_index_size(const mm2gb_index_t *ix_, int64_t *n_occurrences)
{
	const SeedIndex *ix = reinterpret_cast<const SeedIndex*>(ix_);
	if (!ix) return -1;
	if (n_occurrences) *n_occurrences = (int64_t)ix->where.size();
	return (int64_t)ix->keys.size();
}

// options.c:78-84 with index.c:186-211: one more than the (1 - frac) quantile of the occurrence counts, within [min_mid_occ, max_mid_occ]
int32_t mm2gb_index_mid_occ(const mm2gb_index_t *ix_, float frac, int32_t min_mid_occ, int32_t max_mid_occ)
{
	const SeedIndex *ix = reinterpret_cast<const SeedIndex*>(ix_);
	if (!ix) return -1;
	int32_t occ = INT32_MAX;
	if (frac > 0.f && !ix->keys.empty()) {
		const size_t n = ix->keys.size();
		std::vector<uint32_t> cnt(n);
		for (size_t i = 0; i < n; ++i) cnt[i] = (uint32_t)(ix->first[i + 1] - ix->first[i]);
		const size_t kth = (size_t)(uint32_t)((1. - frac) * n);
		std::nth_element(cnt.begin(), cnt.begin() + (ptrdiff_t)std::min(kth, n - 1), cnt.end());
		occ = (int32_t)(cnt[std::min(kth, n - 1)] + 1);
	}
	if (occ < min_mid_occ) occ = min_mid_occ;
	if (max_mid_occ > min_mid_occ && occ > max_mid_occ) occ = max_mid_occ;
	return occ;
}

int mm2gb_index_view(const mm2gb_index_t *ix_, mm2gb_index_view_t *out)
{
	const SeedIndex *ix = reinterpret_cast<const SeedIndex*>(ix_);
	if (!ix || !out) return fail("mm2gb_index_view: null argument");
	std::lock_guard<std::mutex> lock(ix->dev_mu);
	out->n_keys = (int64_t)ix->keys.size(); out->n_occ = (int64_t)ix->where.size(); out->n_bucket = (int64_t)ix->bucket.size();
	out->bucket_shift = ix->bucket_shift; out->k = ix->k; out->w = ix->w; out->built_on = ix->built_on; out->uploads = ix->uploads;
	out->keys = ix->keys.data(); out->first = ix->first.data(); out->where = ix->where.data(); out->bucket = ix->bucket.data();
	return 0;
}

// a device's resident arrays as they are, into the caller's buffers (sized by mm2gb_index_view); on a stream of its own
int mm2gb_index_fetch_device(const mm2gb_index_t *ix_, int device, uint64_t *keys, int64_t *first, uint64_t *where, uint32_t *bucket)
{
	const SeedIndex *ix = reinterpret_cast<const SeedIndex*>(ix_);
	if (!ix || !keys || !first || !where || !bucket) return fail("mm2gb_index_fetch_device: null argument");
	std::lock_guard<std::mutex> lock(ix->dev_mu);
	const SeedIndex::DevCopy *have = nullptr;
	for (const SeedIndex::DevCopy &c : ix->dev) if (c.device == device) have = &c;
	if (!have) return fail("mm2gb_index_fetch_device: the index is not resident on device " + std::to_string(device));
	MM2GB_HIP(hipSetDevice(device));
	hipStream_t s = nullptr;
	MM2GB_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
	void *dst[4] = { keys, first, where, bucket };
	const size_t bytes[4] = { ix->keys.size() * 8, ix->first.size() * 8, ix->where.size() * 8, ix->bucket.size() * 4 };
	hipError_t err = hipSuccess;
	for (int a = 0; a < 4 && err == hipSuccess; ++a) if (bytes[a]) err = hipMemcpyAsync(dst[a], have->ptr[a], bytes[a], hipMemcpyDeviceToHost, s);
	const hipError_t done = hipStreamSynchronize(s);
	(void)hipStreamDestroy(s);
	if (err == hipSuccess) err = done;
	if (err != hipSuccess) return fail(std::string("mm2gb_index_fetch_device: ") + hipGetErrorString(err));
	return 0;
}

int mm2gb_index_build_split(const mm2gb_index_t *ix_, double *ms)
{
	const SeedIndex *ix = reinterpret_cast<const SeedIndex*>(ix_);
	if (!ix || !ms) return fail("mm2gb_index_build_split: null argument");
	for (int a = 0; a < 5; ++a) ms[a] = ix->build_ms[a];
	return 0;
}

int mm2gb_collect_matches(const mm2gb_index_t *ix, const char *seq, int32_t len, const mm2gb_seed_opt_t *opt, mm2gb_matches_t *out)
{
	return collect_matches_refs(ix, seq, len, opt, out, nullptr);
}

int mm2gb_collect_matches_frag(const mm2gb_index_t *ix, int32_t n_segs, const char *const *seqs, const int32_t *lens, const mm2gb_seed_opt_t *opt, mm2gb_matches_t *out)
{
	if (n_segs < 1 || n_segs > 2) return fail("mm2gb_collect_matches_frag: a fragment has one or two segments (MM_MAX_SEG > 2 is not taken)");
	return collect_matches_frag_refs(ix, n_segs, seqs, lens, opt, opt ? opt->mid_occ : 0, out, nullptr);
}

} // extern "C"

// The index in a device's memory: keys, first, where, bucket copied as they are; the look-up there is SeedIndex::find as written (k_m_lookup).
int mm2gb::index_on_device(const mm2gb_index_t *ix_, int device, DevIndexView *out)
{
	const SeedIndex *ix = reinterpret_cast<const SeedIndex*>(ix_);
	if (!ix || !out) return fail("mm2gb_index_to_device: null argument");
	std::lock_guard<std::mutex> lock(ix->dev_mu);
	const SeedIndex::DevCopy *have = nullptr;
	for (const SeedIndex::DevCopy &c : ix->dev) if (c.device == device) have = &c;
	if (!have) {
		int n_dev = 0;
		if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) return fail("mm2gb_index_to_device: device " + std::to_string(device) + " not present");
		MM2GB_HIP(hipSetDevice(device));
		SeedIndex::DevCopy c;
		c.device = device;
		const void *src[4] = { ix->keys.data(), ix->first.data(), ix->where.data(), ix->bucket.data() };
		const size_t bytes[4] = { ix->keys.size() * 8, ix->first.size() * 8, ix->where.size() * 8, ix->bucket.size() * 4 };
		for (int a = 0; a < 4; ++a) { c.ptr[a] = nullptr; c.bytes[a] = std::max<size_t>(bytes[a], 8); }
		hipError_t err = hipSuccess;
		for (int a = 0; a < 4 && err == hipSuccess; ++a) {
			err = hipMalloc(&c.ptr[a], c.bytes[a]);
			if (err == hipSuccess && bytes[a]) err = hipMemcpy(c.ptr[a], src[a], bytes[a], hipMemcpyHostToDevice);
		}
		if (err != hipSuccess) {                        // an error of the call, never another way to the result
			for (int a = 0; a < 4; ++a) if (c.ptr[a]) (void)hipFree(c.ptr[a]);
			(void)hipGetLastError();
			return fail(std::string("mm2gb_index_to_device: the index does not fit the device: ") + hipGetErrorString(err));
		}
		ix->dev.push_back(c);
		++ix->uploads;
		have = &ix->dev.back();
	}
	out->keys = (const unsigned long long*)have->ptr[0]; out->first = (const long long*)have->ptr[1];
	out->where = (const unsigned long long*)have->ptr[2]; out->bucket = (const uint32_t*)have->ptr[3];
	out->n_bucket = ix->bucket.size(); out->bucket_shift = ix->bucket_shift; out->k = ix->k; out->w = ix->w; out->flag = ix->flag;
	return 0;
}

// refs == nullptr: out->hits is a copy of every kept seed's occurrences; otherwise out->hits stays null and refs[s] points at seed s's
// occurrences in the index (the mapper copies them straight into the batch's array: host_chain.h)
int mm2gb::collect_matches_refs(const mm2gb_index_t *ix, const char *seq, int32_t len, const mm2gb_seed_opt_t *opt, mm2gb_matches_t *out, std::vector<const uint64_t*> *refs)
{
	if (len < 0 || (len > 0 && !seq)) return fail("mm2gb_collect_matches: null argument");
	return collect_matches_frag_refs(ix, 1, &seq, &len, opt, opt ? opt->mid_occ : 0, out, refs);
}

// The same for a fragment of n_segs segments (map.c:186-200, 663-666): every segment sketched by itself, segment j's minimizers moved behind those of the segments before
// it (y += (lens[0] + .. + lens[j-1]) << 1) with j in y >> 32, and everything after that on ONE list of length qlen_sum -- the q-occurrence filter, the tandem test across
// the segments' boundary, the streaks and their length, the repeat length's state machine, mini_pos in concatenated coordinates.  flt_mid_occ: the threshold of the
// q-occurrence filter, which the reference runs once with mid_occ before either round of seed collection (map.c:664); opt->mid_occ is the round's (max_occ in the rescue)
int mm2gb::collect_matches_frag_refs(const mm2gb_index_t *ix_, int n_segs, const char *const *seqs, const int32_t *lens, const mm2gb_seed_opt_t *opt, int32_t flt_mid_occ, mm2gb_matches_t *out,
                                     std::vector<const uint64_t*> *refs)
{
	const SeedIndex *ix = reinterpret_cast<const SeedIndex*>(ix_);
	if (!ix || !opt || !out || n_segs < 1 || !seqs || !lens) return fail("mm2gb_collect_matches: null argument");
	int32_t len = 0;                                       // qlen_sum
	for (int j = 0; j < n_segs; ++j) { if (lens[j] < 0 || (lens[j] > 0 && !seqs[j])) return fail("mm2gb_collect_matches: null argument"); len += lens[j]; }
	memset(out, 0, sizeof(*out));
	std::vector<Mini> mv;
	for (int j = 0, sum = 0; j < n_segs; sum += lens[j++]) {
		const size_t from = mv.size();
		if (lens[j] > 0) sketch(seqs[j], lens[j], ix->w, ix->k, (uint32_t)j, (ix->flag & MM2GB_I_HPC) != 0, mv);
		for (size_t i = from; i < mv.size(); ++i) mv[i].y += (uint64_t)sum << 1;
	}
	// seed.c:5-30: a minimizer that makes up more than q_occ_frac of the read's minimizers (and more than mid_occ of them) goes
	if (opt->q_occ_frac > 0.0f && flt_mid_occ > 0 && (int64_t)mv.size() > flt_mid_occ) {
		// occurrences of every minimizer value in the read, counted in an open-addressed table (the reference sorts a copy, seed.c:12-16; what
		// is dropped depends on the counts only)
		size_t cap = 64;
		while (cap < 2 * mv.size()) cap <<= 1;
		std::vector<uint64_t> key(cap, ~0ull);
		std::vector<int32_t> cnt(cap, 0);
		auto slot_of = [&](uint64_t x) { size_t h = (size_t)((x * 0x9E3779B97F4A7C15ull) >> 20) & (cap - 1); while (key[h] != ~0ull && key[h] != x) h = (h + 1) & (cap - 1); return h; };
		bool any = false;
		for (const Mini &q : mv) { const size_t h = slot_of(q.x); key[h] = q.x; any |= ++cnt[h] > flt_mid_occ; }
		if (any) {
			size_t kept = 0;
			for (size_t i = 0; i < mv.size(); ++i) {
				const int32_t c = cnt[slot_of(mv[i].x)];
				if (!(c > flt_mid_occ && c > mv.size() * opt->q_occ_frac)) mv[kept++] = mv[i];
			}
			mv.resize(kept);
		}
	}
	// seed.c:32-54
	std::vector<Match> m;
	m.reserve(mv.size());
	for (size_t i = 0; i < mv.size(); ++i) {
		int n = 0;
		const uint64_t *cr = ix->find(mv[i].x >> 8, &n);
		if (n == 0) continue;
		Match q;
		q.n = (uint32_t)n; q.q_pos = (uint32_t)mv[i].y; q.q_span = (uint32_t)(mv[i].x & 0xff); q.seg_id = (uint32_t)(mv[i].y >> 32); q.cr = cr;
		q.flt = false;
		q.tandem = (i > 0 && (mv[i].x >> 8) == (mv[i - 1].x >> 8)) || (i + 1 < mv.size() && (mv[i].x >> 8) == (mv[i + 1].x >> 8));
		m.push_back(q);
	}
	// seed.c:105-111
	if (opt->occ_dist > 0 && opt->max_max_occ > opt->mid_occ) thin_out(m, len, opt->mid_occ, opt->max_max_occ, opt->occ_dist);
	else for (Match &q : m) if (q.n > (uint32_t)opt->mid_occ) q.flt = true;
	// seed.c:112-130: repeat length = bases covered by dropped minimizers; the kept ones, their hits and positions
	int64_t n_hits = 0;
	size_t n_keep = 0;
	for (const Match &q : m) if (!q.flt) { n_hits += q.n; ++n_keep; }
	out->seeds = (mm2gb_seed_t*)malloc((n_keep + 1) * sizeof(mm2gb_seed_t));
	out->hits = refs ? nullptr : (uint64_t*)malloc(((size_t)n_hits + 1) * 8);
	out->mini_pos = (uint64_t*)malloc((n_keep + 1) * 8);
	if (refs) { refs->clear(); refs->reserve(n_keep); }
	if (!out->seeds || (!refs && !out->hits) || !out->mini_pos) { mm2gb_matches_free(out); return fail("mm2gb_collect_matches: out of memory"); }
	int rep_st = 0, rep_en = 0, rep_len = 0;
	int64_t at = 0;
	for (const Match &q : m) {
		if (q.flt) {
			const int en = (int)(q.q_pos >> 1) + 1, st = en - (int)q.q_span;
			if (st > rep_en) { rep_len += rep_en - rep_st; rep_st = st; rep_en = en; }
			else rep_en = en;
		} else {
			mm2gb_seed_t &s = out->seeds[out->n_seeds];
			s.n = q.n; s.q_pos = q.q_pos; s.span_flt = q.q_span; s.seg_tandem = q.seg_id | (q.tandem ? 1u << 31 : 0u);
			if (refs) refs->push_back(q.cr);
			else memcpy(out->hits + at, q.cr, (size_t)q.n * 8);
			at += q.n;
			out->mini_pos[out->n_seeds++] = (uint64_t)q.q_span << 32 | q.q_pos >> 1;
		}
	}
	out->rep_len = rep_len + (rep_en - rep_st);
	out->n_hits = n_hits;
	out->n_mini_pos = out->n_seeds;
	return 0;
}

extern "C" {

// collect_seed_hits (map.c:295-331) with skip_seed (map.c:205-227) on host threads: the same function as mm2gb_collect_seeds_gpu, for
// batches small enough that the trip over the link and one wave sorting the largest read cost more than they save
int mm2gb_collect_seeds_host(int64_t opt_flag, int64_t n_reads, const int64_t *seed_off, const mm2gb_seed_t *seeds, const int64_t *hit_off,
                             const uint64_t *hits, const int32_t *qlen, const int32_t *q_rank, int32_t n_ref, const int32_t *ref_len,
                             const int32_t *ref_rank, int n_threads, int64_t *anchor_off, mm2gb_anchor_t *anchors)
{
	constexpr int64_t F_NO_DIAG = 0x001, F_NO_DUAL = 0x002, F_FOR_ONLY = 0x100000, F_REV_ONLY = 0x200000, F_QSTRAND = 0x100000000LL;   // minimap.h:8-9,28-29,40
	if (n_reads < 0 || !seed_off || !anchor_off || seed_off[0] != 0) return fail("mm2gb_collect_seeds_host: seed_off[0] must be 0");
	anchor_off[0] = 0;
	if (n_reads == 0) return 0;
	const int64_t n_seeds = seed_off[n_reads];
	if (!qlen || !hit_off || (n_seeds > 0 && !seeds) || hit_off[0] != 0) return fail("mm2gb_collect_seeds_host: null argument, or hit_off[0] is not 0");
	const bool names = (opt_flag & (F_NO_DIAG | F_NO_DUAL)) != 0 && q_rank != nullptr;
	if (names && (!ref_rank || n_ref <= 0)) return fail("mm2gb_collect_seeds_host: NO_DIAG / NO_DUAL need ref_rank");
	if (((opt_flag & F_QSTRAND) || (names && (opt_flag & F_NO_DIAG))) && (!ref_len || n_ref <= 0)) return fail("mm2gb_collect_seeds_host: QSTRAND / NO_DIAG need ref_len");
	if (hit_off[n_seeds] > 0 && (!hits || !anchors)) return fail("mm2gb_collect_seeds_host: null buffer");
	// every read writes at its hits' offset first (an upper bound of where it ends up), sorts there, and is moved down afterwards
	std::vector<int64_t> kept((size_t)n_reads, 0);
	for_each_on_threads((size_t)n_reads, n_threads, 1, [&](size_t r) {
		mm2gb_anchor_t *out = anchors + hit_off[seed_off[r]];
		int64_t n_a = 0;
		for (int64_t k = seed_off[r]; k < seed_off[r + 1]; ++k) {
			const mm2gb_seed_t &q = seeds[k];
			const uint32_t q_span = q.span_flt & 0x7fffffffu, seg_id = q.seg_tandem & 0x7fffffffu;
			for (int64_t h = hit_off[k]; h < hit_off[k + 1]; ++h) {
				const uint64_t rr = hits[h];
				const int32_t rpos = (int32_t)((uint32_t)rr >> 1);
				const bool same_strand = (rr & 1) == (q.q_pos & 1);
				bool skip = false, is_self = false;
				if (names) {                                                                      // map.c:208-219
					const int32_t rid = (int32_t)(rr >> 32);
					if ((opt_flag & F_NO_DIAG) && q_rank[r] == ref_rank[rid] && ref_len[rid] == qlen[r]) {
						if ((uint32_t)rr >> 1 == (q.q_pos >> 1)) skip = true;
						else if (same_strand) is_self = true;
					}
					if (!skip && (opt_flag & F_NO_DUAL) && q_rank[r] > ref_rank[rid]) skip = true;
				}
				if (!skip && (opt_flag & (F_FOR_ONLY | F_REV_ONLY))) skip = same_strand ? (opt_flag & F_REV_ONLY) != 0 : (opt_flag & F_FOR_ONLY) != 0;   // map.c:220-226
				if (skip) continue;
				mm2gb_anchor_t &p = out[n_a++];
				if (same_strand) {                                                                // map.c:311-313
					p.x = (rr & 0xffffffff00000000ULL) | (uint32_t)rpos;
					p.y = (uint64_t)q_span << 32 | q.q_pos >> 1;
				} else if (!(opt_flag & F_QSTRAND)) {                                             // map.c:314-316
					p.x = 1ULL << 63 | (rr & 0xffffffff00000000ULL) | (uint32_t)rpos;
					p.y = (uint64_t)q_span << 32 | (uint32_t)(qlen[r] - (int32_t)((q.q_pos >> 1) + 1 - q_span) - 1);
				} else {                                                                          // map.c:317-321
					p.x = 1ULL << 63 | (rr & 0xffffffff00000000ULL) | (uint32_t)(ref_len[rr >> 32] - (rpos + 1 - (int32_t)q_span) - 1);
					p.y = (uint64_t)q_span << 32 | q.q_pos >> 1;
				}
				p.y |= (uint64_t)seg_id << 48;                                                     // MM_SEED_SEG_SHIFT
				if (q.seg_tandem >> 31) p.y |= 1ULL << 42;                                         // MM_SEED_TANDEM
				if (is_self) p.y |= 1ULL << 43;                                                    // MM_SEED_SELF
			}
		}
		sort_by_x_like_host(out, out + n_a);                                                       // map.c:329
		kept[(size_t)r] = n_a;
	});
	for (int64_t r = 0; r < n_reads; ++r) {
		anchor_off[r + 1] = anchor_off[r] + kept[(size_t)r];
		const int64_t from = hit_off[seed_off[r]];
		if (from != anchor_off[r] && kept[(size_t)r] > 0) memmove(anchors + anchor_off[r], anchors + from, (size_t)kept[(size_t)r] * sizeof(mm2gb_anchor_t));
	}
	return 0;
}

void mm2gb_matches_free(mm2gb_matches_t *m)
{
	if (!m) return;
	free(m->seeds); free(m->hits); free(m->mini_pos);
	memset(m, 0, sizeof(*m));
}

} // extern "C"
