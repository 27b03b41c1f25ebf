// index_kernels.hip -- the minimizer index built on the device (gfx950): mm2gb_index_build_gpu, mm2gb_index_mid_occ_gpu.
// Every array is byte-identical to what seeding.cpp's mm2gb_index_build / mm2gb_index_mid_occ make, which stay the definition.
//
//   sketch   the sequences in chunks of whole sequences through launch_sketch_* (seed_kernels.hip), rid = sequence index; the H2D copy of
//            chunk c + 1 runs on the engine's input stream while chunk c is sketched; each chunk's pairs are split into the sort's key
//            (x >> 8) and value (y) and appended to two device arrays that grow geometrically and keep their contents;
//   sort     by (x >> 8, y), the host's comparator: a stable LIBRARY radix sort (rocPRIM) over bits [0, 2k) of the key.  Equal keys keep
//            their order of arrival, and they arrive in ascending y: chunks are appended in sequence order and a sequence's sketch
//            emits its pairs in ascending position (tests/test_index_api_cpu.py asserts it).  The values are sorted straight into `where`;
//   tables   ours: heads (key[i] != key[i-1]), their exclusive scan (library), then one thread per head writes its key, where its
//            occurrences begin, and the bucket entries between its predecessor's prefix and its own (a long gap by its whole wave);
//   mid_occ  ours: the k-th smallest count by radix select, four histogram passes of 8 bits over first[], the digit picked on the device.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>
#include <rocprim/functional.hpp>
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "engine.h"
#include "index_dev.h"

namespace mm2gb {
namespace {

__global__ __launch_bounds__(TB) void k_ix_split(const ulonglong2 *mini, int64_t n, unsigned long long *key, unsigned long long *val)
{
	const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
	if (i >= n) return;
	const ulonglong2 q = mini[i];
	key[i] = q.x >> 8;                                                            // the span apart (seeding.cpp:227, index.c:229)
	val[i] = q.y;
}

__global__ __launch_bounds__(TB) void k_ix_heads(const unsigned long long *key, int64_t n, unsigned char *head)
{
	const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
	if (i > n) return;
	head[i] = (i < n && (i == 0 || key[i] != key[i - 1])) ? 1 : 0;
}

// keys / first as mm2gb_index_build's loop writes them, bucket as SeedIndex::build_buckets defines it: bucket[b] = first key with
// (key >> shift) >= b.  Head number j, with prefix p, is that key for every b in (prefix of head j - 1, p]; thread n closes both tables
// (the buckets above the last key's prefix hold n_keys; without keys that is every bucket, and n_keys is 0).
// The gaps are NOT all short: a minimizer is the smallest hash of its window, so the keys crowd the low prefixes and thin out towards the
// top -- of 187 M minimizers at w = 10 a few dozen lie in the top fifth of the key space, and the last gap alone is millions of buckets.
// A thread fills a gap of fewer than GAP_WAVE entries itself; a longer one is filled by its whole wave, 64 entries a step.
constexpr int GAP_WAVE = 32;
__global__ __launch_bounds__(TB) void k_ix_tables(const unsigned long long *key, const unsigned char *head, const long long *pos, int64_t n, int64_t n_keys, int bits,
                                                   int shift, unsigned long long *keys_out, long long *first_out, uint32_t *bucket_out)
{
	const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
	long long from = 0, to = -1, j = 0;                                           // this thread's bucket entries: [from, to] hold j
	if (i == n) {
		first_out[n_keys] = n;
		from = n > 0 ? (long long)(key[n - 1] >> shift) + 1 : 0; to = 1ll << bits; j = n_keys;
	} else if (i < n && head[i]) {
		j = pos[i];
		const unsigned long long x = key[i];
		keys_out[j] = x;
		first_out[j] = i;
		from = i > 0 ? (long long)(key[i - 1] >> shift) + 1 : 0; to = (long long)(x >> shift);
	}
	const bool wide = to - from >= GAP_WAVE;
	if (!wide) for (long long b = from; b <= to; ++b) bucket_out[b] = (uint32_t)j;
	const int lane = threadIdx.x & 63;
	for (unsigned long long m = __ballot(wide); m; m &= m - 1) {                  // (every lane of the wave gets here: no thread has returned)
		const int src = __ffsll((long long)m) - 1;
		const long long f = __shfl(from, src), t = __shfl(to, src);
		const uint32_t v = (uint32_t)__shfl(j, src);
		for (long long b = f + lane; b <= t; b += 64) bucket_out[b] = v;
	}
}

// ---- radix select: work[0] the value's bits found so far, work[1] the rank among the counts that share them, work[2 ..] the histogram
__global__ void k_ix_select_init(unsigned long long *work, unsigned long long rank)
{
	const int t = threadIdx.x;
	if (t == 0) { work[0] = 0; work[1] = rank; }
	work[2 + t] = 0;
}

// counts that share the bits above shift + 8 with the value so far, by their next 8 bits.  Most keys occur once: a thread adds a run of
// equal digits with one atomic
__global__ __launch_bounds__(TB) void k_ix_hist(const long long *first, int64_t n_keys, unsigned long long *work, int shift)
{
	__shared__ unsigned s_hist[256];
	s_hist[threadIdx.x] = 0;
	__syncthreads();
	const uint32_t prefix = (uint32_t)work[0];
	int run_digit = -1;
	unsigned run = 0;
	for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < n_keys; i += (int64_t)gridDim.x * TB) {
		const uint32_t cnt = (uint32_t)(first[i + 1] - first[i]);                 // as mm2gb_index_mid_occ counts
		if (shift < 24 && (cnt >> (shift + 8)) != (prefix >> (shift + 8))) continue;
		const int d = (int)((cnt >> shift) & 255u);
		if (d != run_digit) { if (run) atomicAdd(&s_hist[run_digit], run); run_digit = d; run = 0; }
		++run;
	}
	if (run) atomicAdd(&s_hist[run_digit], run);
	__syncthreads();
	if (s_hist[threadIdx.x]) atomicAdd(&work[2 + threadIdx.x], (unsigned long long)s_hist[threadIdx.x]);
}

// the digit that holds the rank, in ascending order of digits; the histogram is cleared for the next pass
__global__ void k_ix_pick(unsigned long long *work, int shift)
{
	__shared__ unsigned long long s_hist[256];
	const int t = threadIdx.x;
	s_hist[t] = work[2 + t];
	work[2 + t] = 0;
	__syncthreads();
	if (t != 0) return;
	unsigned long long want = work[1];
	int d = 0;
	for (; d < 255; ++d) { if (want < s_hist[d]) break; want -= s_hist[d]; }
	work[0] |= (unsigned long long)d << shift;
	work[1] = want;
}

struct HeadOf { __host__ __device__ long long operator()(unsigned char h) const { return (long long)h; } };

} // namespace

void launch_ix_split(const ulonglong2 *mini, int64_t n, unsigned long long *key_out, unsigned long long *val_out, hipStream_t s)
{
	if (n > 0) hipLaunchKernelGGL(k_ix_split, dim3(blocks(n)), dim3(TB), 0, s, mini, n, key_out, val_out);
}

int ix_sort_pairs(void *tmp, size_t &tmp_bytes, const unsigned long long *key_in, unsigned long long *key_out, const unsigned long long *val_in,
                  unsigned long long *val_out, int64_t n, int k, hipStream_t s)
{
	return rocprim::radix_sort_pairs(tmp, tmp_bytes, key_in, key_out, val_in, val_out, (size_t)n, 0u, (unsigned)(2 * k), s) == hipSuccess ? 0 : -1;
}

int ix_heads_scan(void *tmp, size_t &tmp_bytes, const unsigned long long *key, int64_t n, unsigned char *head, long long *pos, hipStream_t s)
{
	if (tmp) hipLaunchKernelGGL(k_ix_heads, dim3(blocks(n + 1)), dim3(TB), 0, s, key, n, head);
	return rocprim::exclusive_scan(tmp, tmp_bytes, rocprim::make_transform_iterator((const unsigned char*)head, HeadOf()), pos, 0ll, (size_t)n + 1, rocprim::plus<long long>(), s) == hipSuccess ? 0 : -1;
}

void launch_ix_tables(const unsigned long long *key, const unsigned char *head, const long long *pos, int64_t n, int64_t n_keys, int bits, int bucket_shift,
                      unsigned long long *keys_out, long long *first_out, uint32_t *bucket_out, hipStream_t s)
{
	hipLaunchKernelGGL(k_ix_tables, dim3(blocks(n + 1)), dim3(TB), 0, s, key, head, pos, n, n_keys, bits, bucket_shift, keys_out, first_out, bucket_out);
}

void launch_ix_select(const long long *first, int64_t n_keys, unsigned long long rank, unsigned long long *work, int n_cu, hipStream_t s)
{
	hipLaunchKernelGGL(k_ix_select_init, dim3(1), dim3(256), 0, s, work, rank);
	const unsigned grid = (unsigned)std::min<int64_t>(blocks(n_keys), (int64_t)std::max(n_cu, 1) * 8);
	for (int shift = 24; shift >= 0; shift -= 8) {
		hipLaunchKernelGGL(k_ix_hist, dim3(grid), dim3(TB), 0, s, first, n_keys, work, shift);
		hipLaunchKernelGGL(k_ix_pick, dim3(1), dim3(256), 0, s, work, shift);
	}
}

// ---------------------------------------------------------------------------------------------------------------- the build
namespace {

constexpr size_t PIECE = (size_t)16 << 20;                 // bytes per copy of the way back (two page-locked pieces alternate)

// a device array that keeps its contents when it grows: by a quarter, as the engines' arenas do (engine.hip), the outgrown buffer retired
struct KeptBuf {
	void *ptr = nullptr; size_t bytes = 0;
	int ensure(size_t need, size_t used, hipStream_t s)
	{
		if (need <= bytes) return 0;
		size_t want = bytes ? std::max(need, bytes + bytes / 4) : need;
		void *fresh = nullptr;
		if (hipMalloc(&fresh, want) != hipSuccess) {
			(void)hipGetLastError();
			flush_retired_buffers();
			want = need;
			if (hipMalloc(&fresh, want) != hipSuccess) { (void)hipGetLastError(); return fail("no room on the device for " + std::to_string(want) + " bytes of the index"); }
		}
		if (used > 0) { const hipError_t err = hipMemcpyAsync(fresh, ptr, used, hipMemcpyDeviceToDevice, s); if (err != hipSuccess) { retire_device_buffer(fresh, want); return fail(std::string("hipMemcpyAsync: ") + hipGetErrorString(err)); } }
		retire_device_buffer(ptr, bytes);
		ptr = fresh; bytes = want;
		return 0;
	}
};

int device_alloc(void **out, size_t bytes)
{
	if (hipMalloc(out, bytes) == hipSuccess) return 0;
	(void)hipGetLastError();
	flush_retired_buffers();
	if (hipMalloc(out, bytes) == hipSuccess) return 0;
	(void)hipGetLastError();
	*out = nullptr;
	return fail("no room on the device for " + std::to_string(bytes) + " bytes of the index");
}

struct Chunk { int32_t s0, s1; int64_t bases; };

// everything a build holds besides its result; whatever is left when it ends, either way, is given up here
struct Build {
	Engine &e;
	PinnedBuf h_in[2];                                     // staging of a chunk (offsets, ids, bases), then the pieces of the way back
	DevBuf d_in[2];
	hipEvent_t in_done[2] = { nullptr, nullptr }, sk_done[2] = { nullptr, nullptr }, out_done[2] = { nullptr, nullptr };
	bool in_used[2] = { false, false }, sk_used[2] = { false, false };
	std::vector<hipEvent_t> marks[4];                      // pairs (start, end) of the timed spans: H2D, sketch, sort, tables
	KeptBuf key_in, val_in;
	void *key_sorted = nullptr; size_t key_sorted_bytes = 0;
	void *final_ptr[4] = { nullptr, nullptr, nullptr, nullptr }; size_t final_bytes[4] = { 0, 0, 0, 0 };   // keys, first, where, bucket until the index owns them
	explicit Build(Engine &e_) : e(e_) {}
	int init()
	{
		for (int s = 0; s < 2; ++s) { MM2GB_HIP(hipEventCreateWithFlags(&in_done[s], hipEventDisableTiming)); MM2GB_HIP(hipEventCreateWithFlags(&sk_done[s], hipEventDisableTiming)); MM2GB_HIP(hipEventCreateWithFlags(&out_done[s], hipEventDisableTiming)); }
		return 0;
	}
	int mark(int what, hipStream_t s) { hipEvent_t ev = nullptr; MM2GB_HIP(hipEventCreate(&ev)); marks[what].push_back(ev); MM2GB_HIP(hipEventRecord(ev, s)); return 0; }
	double spans_ms(int what) const
	{
		double sum = 0;
		for (size_t m = 0; m + 1 < marks[what].size(); m += 2) { float t = 0; if (hipEventElapsedTime(&t, marks[what][m], marks[what][m + 1]) == hipSuccess) sum += t; }
		return sum;
	}
	~Build()
	{
		(void)hipStreamSynchronize(e.stream); (void)hipStreamSynchronize(e.s_in); (void)hipStreamSynchronize(e.s_out);
		(void)hipGetLastError();
		for (int s = 0; s < 2; ++s) {
			h_in[s].release();
			retire_device_buffer(d_in[s].ptr, d_in[s].bytes); d_in[s].ptr = nullptr; d_in[s].bytes = 0;
			if (in_done[s]) (void)hipEventDestroy(in_done[s]);
			if (sk_done[s]) (void)hipEventDestroy(sk_done[s]);
			if (out_done[s]) (void)hipEventDestroy(out_done[s]);
		}
		for (auto &v : marks) for (hipEvent_t ev : v) (void)hipEventDestroy(ev);
		retire_device_buffer(key_in.ptr, key_in.bytes); retire_device_buffer(val_in.ptr, val_in.bytes); retire_device_buffer(key_sorted, key_sorted_bytes);
		for (int a = 0; a < 4; ++a) retire_device_buffer(final_ptr[a], final_bytes[a]);
	}
};

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// chunk c into page-locked memory and from there to the device, on the input stream: offsets, ids, bases and the closing 'N' in one copy
int stage_chunk(Build &B, const Chunk &c, int set, const char *const *seqs, const int32_t *lens)
{
	Engine &e = B.e;
	const size_t ns = (size_t)(c.s1 - c.s0), o_rid = (ns + 1) * 8, o_seq = align256(o_rid + ns * 4), total = o_seq + (size_t)c.bases + 1;
	if (B.in_used[set]) MM2GB_HIP(hipEventSynchronize(B.in_done[set]));          // the copy two chunks back has left the page-locked block
	if (B.h_in[set].ensure(total)) return -1;
	char *h = (char*)B.h_in[set].ptr;
	int64_t *off = (int64_t*)h;
	uint32_t *rid = (uint32_t*)(h + o_rid);
	char *bases = h + o_seq;
	off[0] = 0;
	for (int32_t s = c.s0; s < c.s1; ++s) {
		const size_t j = (size_t)(s - c.s0);
		if (lens[s] > 0) memcpy(bases + off[j], seqs[s], (size_t)lens[s]);
		off[j + 1] = off[j] + lens[s];
		rid[j] = (uint32_t)s;
	}
	bases[c.bases] = 'N';
	if (B.sk_used[set]) MM2GB_HIP(hipStreamWaitEvent(e.s_in, B.sk_done[set], 0));  // the sketch two chunks back has read the device block
	if (B.d_in[set].ensure(total)) return -1;
	if (B.mark(0, e.s_in)) return -1;
	MM2GB_HIP(hipMemcpyAsync(B.d_in[set].ptr, h, total, hipMemcpyHostToDevice, e.s_in));
	if (B.mark(0, e.s_in)) return -1;
	MM2GB_HIP(hipEventRecord(B.in_done[set], e.s_in));
	B.in_used[set] = true;
	return 0;
}

// the arrays of a finished index from the device into the host's vectors: async copies into two page-locked pieces on the output stream,
// piece p + 1 on its way while piece p is moved into the vector
int copy_back(Build &B, const std::vector<std::pair<char*, const char*>> &arrays, const std::vector<size_t> &sizes)
{
	Engine &e = B.e;
	struct Piece { char *dst; const char *src; size_t bytes; };
	std::vector<Piece> pieces;
	for (size_t a = 0; a < arrays.size(); ++a)
		for (size_t at = 0; at < sizes[a]; at += PIECE) pieces.push_back({ arrays[a].first + at, arrays[a].second + at, std::min(PIECE, sizes[a] - at) });
	if (pieces.empty()) return 0;
	size_t largest = 0;
	for (const Piece &p : pieces) largest = std::max(largest, p.bytes);
	for (int s = 0; s < 2; ++s) if (B.h_in[s].ensure(largest)) return -1;
	auto land = [&](size_t p) -> int {
		MM2GB_HIP(hipEventSynchronize(B.out_done[p & 1]));
		memcpy(pieces[p].dst, B.h_in[p & 1].ptr, pieces[p].bytes);
		return 0;
	};
	for (size_t p = 0; p < pieces.size(); ++p) {
		MM2GB_HIP(hipMemcpyAsync(B.h_in[p & 1].ptr, pieces[p].src, pieces[p].bytes, hipMemcpyDeviceToHost, e.s_out));
		MM2GB_HIP(hipEventRecord(B.out_done[p & 1], e.s_out));
		if (p > 0 && land(p - 1)) return -1;
	}
	return land(pieces.size() - 1);
}

int build_on_device(Engine &e, SeedIndex *ix, int k, int w, int flag, int32_t n_seq, const char *const *seqs, const int32_t *lens)
{
	// chunks of whole sequences
	int64_t limit = (int64_t)256 << 20;
	if (const char *v = getenv("MM2GB_INDEX_CHUNK_BASES")) { const long long q = atoll(v); if (q > 0) limit = q; }
	limit = std::min<int64_t>(limit, ((int64_t)1 << 31) - 2);                     // positions of a batch are 32-bit on the device
	std::vector<Chunk> chunks;
	int64_t total_bases = 0;
	for (int32_t s = 0; s < n_seq; ++s) {
		if (lens[s] < 0 || (lens[s] > 0 && !seqs[s])) return fail("mm2gb_index_build_gpu: bad arguments (a sequence without bases)");
		if ((int64_t)lens[s] >= ((int64_t)1 << 31) - 1) return fail("mm2gb_index_build_gpu: a sequence is limited to 2^31 - 2 bases");
		if (chunks.empty() || (chunks.back().s1 > chunks.back().s0 && chunks.back().bases + lens[s] > limit)) chunks.push_back({ s, s, 0 });
		chunks.back().s1 = s + 1; chunks.back().bases += lens[s];
		total_bases += lens[s];
	}
	{ std::vector<Chunk> keep; for (const Chunk &c : chunks) if (c.bases > 0) keep.push_back(c); chunks.swap(keep); }     // (a chunk of empty sequences has no minimizers)

	MM2GB_HIP(hipSetDevice(e.device));
	MM2GB_HIP(hipStreamSynchronize(e.stream));
	Build B(e);
	if (B.init()) return -1;
	const hipStream_t st = e.stream;
	int64_t n_occ = 0;
	// room for the pairs a random sequence yields (2 / (w + 1) per base) and a tenth more; what repeats add makes the arrays grow
	const size_t guess = (size_t)((double)total_bases * 2.2 / (w + 1)) + 1024;
	if (B.key_in.ensure(guess * 8, 0, st) || B.val_in.ensure(guess * 8, 0, st)) return -1;
	const size_t n_chunks = chunks.size();
	if (n_chunks > 0 && stage_chunk(B, chunks[0], 0, seqs, lens)) return -1;
	for (size_t c = 0; c < n_chunks; ++c) {
		const int set = (int)(c & 1);
		const Chunk &ch = chunks[c];
		const size_t ns = (size_t)(ch.s1 - ch.s0), o_rid = (ns + 1) * 8, o_seq = align256(o_rid + ns * 4);
		const char *d = (const char*)B.d_in[set].ptr;
		SketchBatch b;
		memset(&b, 0, sizeof b);
		b.seq_off = (const int64_t*)d; b.rid = (const uint32_t*)(d + o_rid); b.seqs = (const unsigned char*)(d + o_seq);
		b.n_seqs = (int64_t)ns; b.n = ch.bases; b.w = w; b.k = k; b.hpc = (flag & MM2GB_I_HPC) != 0;
		if (e.sk_work.ensure(sketch_layout(b, nullptr)) || e.sk_mini_off.ensure((ns + 1) * 8)) return -1;
		sketch_layout(b, e.sk_work.ptr);
		b.mini_off = (int64_t*)e.sk_mini_off.ptr;
		MM2GB_HIP(hipStreamWaitEvent(st, B.in_done[set], 0));
		if (B.mark(1, st)) return -1;
		if (launch_sketch_count(b, st)) return fail("mm2gb_index_build_gpu: a library scan of the sketch refused to run");
		MM2GB_HIP(hipGetLastError());
		int64_t total = 0;
		MM2GB_HIP(hipMemcpyAsync(&total, b.mini_off + b.n_seqs, 8, hipMemcpyDeviceToHost, st));
		if (c + 1 < n_chunks && stage_chunk(B, chunks[c + 1], set ^ 1, seqs, lens)) return -1;     // the next chunk travels while this one is counted
		MM2GB_HIP(hipStreamSynchronize(st));
		if (total < 0 || total >= ((int64_t)1 << 31)) return fail("mm2gb_index_build_gpu: a chunk is limited to 2^31 minimizers");
		if (e.sk_mini.ensure(std::max<size_t>((size_t)total, 1) * 16) || e.sk_mini_read.ensure(std::max<size_t>((size_t)total, 1) * 4)) return -1;
		b.mini = (ulonglong2*)e.sk_mini.ptr; b.mini_read = (int32_t*)e.sk_mini_read.ptr;
		if (total > 0) {
			launch_sketch_write(b, st);
			if (B.key_in.ensure((size_t)(n_occ + total + 1) * 8, (size_t)n_occ * 8, st) || B.val_in.ensure((size_t)(n_occ + total + 1) * 8, (size_t)n_occ * 8, st)) return -1;
			launch_ix_split(b.mini, total, (unsigned long long*)B.key_in.ptr + n_occ, (unsigned long long*)B.val_in.ptr + n_occ, st);
			MM2GB_HIP(hipGetLastError());
		}
		if (B.mark(1, st)) return -1;
		MM2GB_HIP(hipEventRecord(B.sk_done[set], st));
		B.sk_used[set] = true;
		n_occ += total;
	}

	// sort: keys into a buffer of their own, values straight into `where`
	const size_t no = (size_t)n_occ;
	if (B.key_in.ensure((no + 1) * 8, no * 8, st) || B.val_in.ensure((no + 1) * 8, no * 8, st)) return -1;
	B.key_sorted_bytes = (no + 1) * 8;
	if (device_alloc(&B.key_sorted, B.key_sorted_bytes)) return -1;
	B.final_bytes[2] = std::max<size_t>(no * 8, 8);
	if (device_alloc(&B.final_ptr[2], B.final_bytes[2])) return -1;
	size_t tmp_sort = 0, tmp_scan = 0;
	if (no > 0 && ix_sort_pairs(nullptr, tmp_sort, (const unsigned long long*)B.key_in.ptr, (unsigned long long*)B.key_sorted, (const unsigned long long*)B.val_in.ptr,
	                            (unsigned long long*)B.final_ptr[2], n_occ, k, st)) return fail("mm2gb_index_build_gpu: the library sort refused to run");
	if (ix_heads_scan(nullptr, tmp_scan, (const unsigned long long*)B.key_sorted, n_occ, (unsigned char*)B.val_in.ptr, (long long*)B.key_in.ptr, st))
		return fail("mm2gb_index_build_gpu: a library scan of the tables refused to run");
	size_t tmp_bytes = std::max(tmp_sort, tmp_scan) + 256;
	if (e.sk_work.ensure(tmp_bytes)) return -1;                 // (the sketch's arena is done with)
	if (B.mark(2, st)) return -1;
	if (no > 0) {
		size_t q = tmp_bytes;
		if (ix_sort_pairs(e.sk_work.ptr, q, (const unsigned long long*)B.key_in.ptr, (unsigned long long*)B.key_sorted, (const unsigned long long*)B.val_in.ptr,
		                  (unsigned long long*)B.final_ptr[2], n_occ, k, st)) return fail("mm2gb_index_build_gpu: the library sort refused to run");
	}
	if (B.mark(2, st)) return -1;
	// tables: the sort's inputs are free now: the heads go where the values were, their scan where the keys were
	if (B.mark(3, st)) return -1;
	unsigned char *head = (unsigned char*)B.val_in.ptr;
	long long *pos = (long long*)B.key_in.ptr;
	{
		size_t q = tmp_bytes;
		if (ix_heads_scan(e.sk_work.ptr, q, (const unsigned long long*)B.key_sorted, n_occ, head, pos, st)) return fail("mm2gb_index_build_gpu: a library scan of the tables refused to run");
	}
	MM2GB_HIP(hipGetLastError());
	int64_t n_keys = 0;
	MM2GB_HIP(hipMemcpyAsync(&n_keys, pos + n_occ, 8, hipMemcpyDeviceToHost, st));
	MM2GB_HIP(hipStreamSynchronize(st));
	if (n_keys < 0 || n_keys >= ((int64_t)1 << 32)) return fail("mm2gb_index_build_gpu: more than 2^32 distinct minimizers");
	const int bits = SeedIndex::bucket_bits(k, (size_t)n_keys), shift = 2 * k - bits;
	const size_t nk = (size_t)n_keys, nb = ((size_t)1 << bits) + 1;
	B.final_bytes[0] = std::max<size_t>(nk * 8, 8); B.final_bytes[1] = (nk + 1) * 8; B.final_bytes[3] = nb * 4;
	if (device_alloc(&B.final_ptr[0], B.final_bytes[0]) || device_alloc(&B.final_ptr[1], B.final_bytes[1]) || device_alloc(&B.final_ptr[3], B.final_bytes[3])) return -1;
	launch_ix_tables((const unsigned long long*)B.key_sorted, head, pos, n_occ, n_keys, bits, shift, (unsigned long long*)B.final_ptr[0], (long long*)B.final_ptr[1],
	                 (uint32_t*)B.final_ptr[3], st);
	MM2GB_HIP(hipGetLastError());
	if (B.mark(3, st)) return -1;
	MM2GB_HIP(hipEventRecord(B.sk_done[0], st));
	MM2GB_HIP(hipStreamWaitEvent(e.s_out, B.sk_done[0], 0));

	// the way back: into the vectors every host function reads
	const auto t0 = std::chrono::steady_clock::now();
	ix->keys.resize(nk); ix->first.resize(nk + 1); ix->where.resize(no); ix->bucket.resize(nb);
	ix->bucket_shift = shift;
	if (copy_back(B, { { (char*)ix->keys.data(), (const char*)B.final_ptr[0] }, { (char*)ix->first.data(), (const char*)B.final_ptr[1] },
	                   { (char*)ix->where.data(), (const char*)B.final_ptr[2] }, { (char*)ix->bucket.data(), (const char*)B.final_ptr[3] } },
	              { nk * 8, (nk + 1) * 8, no * 8, nb * 4 })) return -1;
	MM2GB_HIP(hipStreamSynchronize(st));
	ix->build_ms[4] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	for (int what = 0; what < 4; ++what) ix->build_ms[what] = B.spans_ms(what);            // (a chunk's copy runs beside the sketch before it)
	// the resident arrays are the index's copy on this device
	SeedIndex::DevCopy copy;
	copy.device = e.device;
	for (int a = 0; a < 4; ++a) { copy.ptr[a] = B.final_ptr[a]; copy.bytes[a] = B.final_bytes[a]; B.final_ptr[a] = nullptr; B.final_bytes[a] = 0; }
	ix->dev.push_back(copy);
	ix->built_on = e.device;
	return 0;
}

} // namespace
} // namespace mm2gb

using namespace mm2gb;

extern "C" {

mm2gb_index_t *mm2gb_index_build_gpu(mm2gb_engine_t *eng, int k, int w, int32_t n_seq, const char *const *seqs, const int32_t *lens)
{
	return mm2gb_index_build_gpu_flag(eng, k, w, 0, n_seq, seqs, lens);
}

mm2gb_index_t *mm2gb_index_build_gpu_flag(mm2gb_engine_t *eng, int k, int w, int flag, int32_t n_seq, const char *const *seqs, const int32_t *lens)
{
	if (!eng) { fail("mm2gb_index_build_gpu: null engine"); return nullptr; }
	if (n_seq < 0 || (n_seq > 0 && (!seqs || !lens)) || w < 1 || w > 255 || k < 1 || k > 28) { fail("mm2gb_index_build_gpu: bad arguments (0 < w < 256, 0 < k <= 28)"); return nullptr; }
	if (flag & ~MM2GB_I_HPC) { fail("mm2gb_index_build_gpu: unknown flag (MM2GB_I_HPC only)"); return nullptr; }
	SeedIndex *ix = new SeedIndex;
	ix->k = k; ix->w = w; ix->flag = flag;
	if (n_seq > 0) ix->lens.assign(lens, lens + n_seq);
	if (build_on_device(eng->e, ix, k, w, flag, n_seq, seqs, lens)) {                   // an error of the call: never the host build instead
		const std::string why = mm2gb_last_error();
		if (why.rfind("mm2gb_index_build_gpu", 0) != 0) fail("mm2gb_index_build_gpu: " + why);
		mm2gb_index_destroy(reinterpret_cast<mm2gb_index_t*>(ix));
		return nullptr;
	}
	return reinterpret_cast<mm2gb_index_t*>(ix);
}

int32_t mm2gb_index_mid_occ_gpu(mm2gb_engine_t *eng, const mm2gb_index_t *ix_, float frac, int32_t min_mid_occ, int32_t max_mid_occ)
{
	const SeedIndex *ix = reinterpret_cast<const SeedIndex*>(ix_);
	if (!eng || !ix) return (int32_t)fail("mm2gb_index_mid_occ_gpu: null argument");
	Engine &e = eng->e;
	int32_t occ = INT32_MAX;
	if (frac > 0.f && !ix->keys.empty()) {
		const size_t n = ix->keys.size();
		const size_t kth = (size_t)(uint32_t)((1. - frac) * n);                   // the host's expression: no floating point on the device
		DevIndexView view;
		if (index_on_device(ix_, e.device, &view)) return -1;
		unsigned long long value = 0;
		hipError_t err = hipSetDevice(e.device);
		if (err == hipSuccess && e.sk_work.ensure((size_t)IX_SELECT_WORDS * 8)) return -1;
		if (err == hipSuccess) {
			launch_ix_select(view.first, (int64_t)n, (unsigned long long)std::min(kth, n - 1), (unsigned long long*)e.sk_work.ptr, e.n_cu, e.stream);
			err = hipGetLastError();
		}
		if (err == hipSuccess) err = hipMemcpyAsync(&value, e.sk_work.ptr, 8, hipMemcpyDeviceToHost, e.stream);
		const hipError_t done = hipStreamSynchronize(e.stream);
		if (err == hipSuccess) err = done;
		if (err != hipSuccess) return (int32_t)fail(std::string("mm2gb_index_mid_occ_gpu: ") + hipGetErrorString(err));
		occ = (int32_t)((uint32_t)value + 1);
	}
	if (occ < min_mid_occ) occ = min_mid_occ;
	if (max_mid_occ > min_mid_occ && occ > max_mid_occ) occ = max_mid_occ;
	return occ;
}

} // extern "C"
