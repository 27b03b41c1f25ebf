// seed_kernels.hip -- from sequence bytes to seed matches on the device (gfx950): the stage in front of k_seed_* (post_kernels.hip).
// Every result is byte-identical to seeding.cpp's host functions (sketch, collect_matches_refs), which stay the definition.
//
// The sketch by POSITION.  seeding.cpp's loop carries state (ring, best, run, slot), but every quantity of a step is a function
// of the input alone:
//   * the words fwd / rev at a step are the last k entries of the sequence's COMPACTED form (an N does not clear them);
//   * a step whose words are equal is SKIPPED (the loop's `continue`); the others are COUNTED, t = 0, 1, ... (slot = t mod w);
//   * run = counted valid steps since the last N: a difference of two prefix sums;
//   * best after step t = the RIGHTMOST minimum of the values of steps [t - w + 1, t]; what step t emits follows from that of t - 1 and t.
// So: prefix sums (library scans), one thread per position for the words, one thread per counted position for what it emits, a scan of
// the counts, the same threads again to write.  A thread reads its w predecessors' values from memory: neighbours read the same lines.
//
// ONE pipeline (sketch_steps) in two FORMS, a template parameter of the kernels that differ (k_sk_words, k_sk_values; the compaction is a
// kernel per form, k_sk_compact / k_hp_compact: they share four lines):
//   plain   a step is a position; the compacted form leaves out the ambiguous bases; the span is k;
//   HPC     homopolymer-compressed (sketch.c:94-105): a step is a BOUNDARY -- a run's first base, an ambiguous base --, every other position
//           counts as skipped; the compacted form has a base per run; a step's position is its run's last base: the next boundary's
//           position (or the sequence's end) minus one; between two ambiguous bases the runs are contiguous, so the span of the last
//           min(k, m) runs is a difference of two positions.  No thread walks along a run.  The boundaries and their scans (k_hp_bound,
//           n_valid over run starts, n_bnd) are this form's own prologue.
//
// Matches: q-occurrence filter by a segmented sort of the reads' values, look-up as SeedIndex::find, streak thinning by RANK -- in a streak
// of matches above mid_occ the survivors are the K smallest by (n, index): a radix select per streak, by a workgroup --, repeat length by a
// wave per read, offsets by scans, hits gathered 64 seeds per wave.
//
// Both pipelines are written once, against a Pass: the layout functions run them to MEASURE the library calls' work space, the launch
// functions to launch.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>
#include <rocprim/functional.hpp>
#include <algorithm>
#include "seed_dev.h"
#include "kmer.h"

namespace mm2gb {
namespace {

constexpr unsigned long long NONE = ~0ull;

// What a pipeline's list of steps runs against.  MEASURING (tmp == nullptr): every library step is asked for its work space and the largest
// answer is kept; nothing is launched.  LAUNCHING: the library steps get tmp, the kernels are launched; after a refusal nothing more is.
struct Pass {
	void *tmp; size_t tmp_bytes; hipStream_t s;
	size_t need = 0; bool refused = false;
	bool launching() const { return tmp && !refused; }
	template <class Call> void lib(Call call)                                  // call(tmp, bytes): a rocPRIM call
	{
		if (refused) return;
		size_t q = tmp_bytes;
		refused = call(tmp, q) != hipSuccess;
		if (!tmp) need = std::max(need, q);
	}
	template <class Kernel, class... Args> void run(Kernel kernel, unsigned grid, unsigned block, const Args &...args)
	{
		if (launching()) hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, s, args...);
	}
};
// the library steps but one: out[i] = in[0] + ... + in[i - 1], and out[i] = op(in[0], ..., in[i])
template <class In, class Out, class T> void sums(Pass &p, In in, Out out, T zero, size_t n)
{
	p.lib([&](void *t, size_t &q) { return rocprim::exclusive_scan(t, q, in, out, zero, n, rocprim::plus<T>(), p.s); });
}
template <class In, class Out, class Op> void running(Pass &p, In in, Out out, size_t n, Op op)
{
	p.lib([&](void *t, size_t &q) { return rocprim::inclusive_scan(t, q, in, out, n, op, p.s); });
}

template <class In, class F> auto via(In in, F f) { return rocprim::make_transform_iterator(in, f); }
inline auto positions() { return rocprim::make_counting_iterator<uint32_t>(0u); }

// largest r < n_seg with off[r] <= i (off[0] <= i < off[n_seg]); empty segments are passed over
__device__ inline int64_t seg_of(const int64_t *off, int64_t n_seg, int64_t i)
{
	int64_t lo = 0, hi = n_seg;
	while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (off[mid] <= i) lo = mid; else hi = mid; }
	return lo;
}
// the same for the threads of a workgroup that look at consecutive i: one bisection for the first, the others walk on from there
__device__ inline int64_t seg_of_block(const int64_t *off, int64_t n_seg, int64_t i_first, int64_t i, bool in)
{
	__shared__ int64_t s_first;
	if (threadIdx.x == 0) s_first = seg_of(off, n_seg, i_first);
	__syncthreads();
	int64_t r = s_first;
	if (in) while (r + 1 < n_seg && off[r + 1] <= i) ++r;
	return r;
}

struct ValidOf { __host__ __device__ uint32_t operator()(unsigned char c) const { return base_code(c) < 4 ? 1u : 0u; } };
struct RunOf   { __host__ __device__ uint32_t operator()(unsigned char f) const { return f & 1u; } };
struct BndOf   { __host__ __device__ uint32_t operator()(unsigned char f) const { return f ? 1u : 0u; } };
struct SkipOf  { __host__ __device__ uint32_t operator()(unsigned char f) const { return (f >> 1) & 1u; } };
struct LastN   { const unsigned char *seqs; __host__ __device__ uint32_t operator()(uint32_t i) const { return base_code(seqs[i]) >= 4 ? i + 1 : 0u; } };
struct ToI64   { __host__ __device__ long long operator()(uint32_t v) const { return (long long)v; } };

// HPC, before the words: flags = 1 the first base of a run (a run does not continue from the sequence before), 2 an ambiguous base,
// 0 inside a run.  Position n is a boundary: every run ends before it
__global__ __launch_bounds__(TB) void k_hp_bound(SketchBatch b)
{
	const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
	const bool in = i < b.n;
	const int64_t r = seg_of_block(b.seq_off, b.n_seqs, (int64_t)blockIdx.x * TB, i, in);
	if (i == b.n) b.flags[i] = 2;
	if (!in) return;
	const int c = base_code(b.seqs[i]);
	b.flags[i] = (unsigned char)(c >= 4 ? 2 : (i == b.seq_off[r] || base_code(b.seqs[i - 1]) != c) ? 1 : 0);
}

// where the run that begins at boundary i ends: before the next boundary, or with its sequence
__device__ inline int64_t run_end(const SketchBatch &b, int64_t i, int64_t r)
{
	return std::min<int64_t>((int64_t)b.bnd_pos[b.n_bnd[i] + 1], b.seq_off[r + 1]) - 1;
}

// the compacted sequences, each from its own offset on.  Plain: the sequences without their ambiguous bases
__global__ __launch_bounds__(TB) void k_sk_compact(SketchBatch b)
{
	const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
	const bool in = i < b.n;
	const int64_t r = seg_of_block(b.seq_off, b.n_seqs, (int64_t)blockIdx.x * TB, i, in);
	if (!in) return;
	const int c = base_code(b.seqs[i]);
	if (c >= 4) return;
	const int64_t s0 = b.seq_off[r];
	b.comp[s0 + (b.n_valid[i] - b.n_valid[s0])] = (unsigned char)c;
}
// HPC: a base per run, and the boundaries' positions
__global__ __launch_bounds__(TB) void k_hp_compact(SketchBatch b)
{
	const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
	const bool in = i < b.n;
	const int64_t r = seg_of_block(b.seq_off, b.n_seqs, (int64_t)blockIdx.x * TB, i, in);
	if (i > b.n) return;
	const unsigned fl = b.flags[i];
	if (fl == 0) return;
	b.bnd_pos[b.n_bnd[i]] = (uint32_t)i;
	if (fl != 1 || !in) return;
	const int64_t s0 = b.seq_off[r];
	b.comp[s0 + (b.n_valid[i] - b.n_valid[s0])] = (unsigned char)base_code(b.seqs[i]);
}

// the words of every step with a base (seeding.cpp:65-70), from the last k bases of its sequence's compacted form.  HPC: the span from the
// first of the last min(k, m) runs' positions (m: runs since the last ambiguous base, this one included) to this run's end; the flags of
// k_hp_bound become what the plain form leaves, inside a run: skipped
template <bool HPC>
__global__ __launch_bounds__(TB) void k_sk_words(SketchBatch b)
{
	const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
	const bool in = i < b.n;
	const int64_t r = seg_of_block(b.seq_off, b.n_seqs, (int64_t)blockIdx.x * TB, i, in);
	if (i == b.n) b.flags[i] = 0;
	if (!in) return;
	if (HPC) {
		const unsigned bnd = b.flags[i];
		if (bnd != 1) { b.flags[i] = (unsigned char)(bnd == 0 ? 2 : 0); return; }
	} else if (base_code(b.seqs[i]) >= 4) { b.flags[i] = 0; return; }
	const int64_t s0 = b.seq_off[r];
	const int64_t o = (int64_t)(b.n_valid[i] - b.n_valid[s0]);
	const unsigned char *at = b.comp + s0 + o;
	const int top = 2 * (b.k - 1);
	const int have = (int)(o + 1 < b.k ? o + 1 : b.k);
	unsigned long long f = 0, rv = 0;
	for (int d = 0; d < have; ++d) {
		const unsigned long long c = at[-d];
		f |= c << (2 * d);
		rv |= (3 ^ c) << (top - 2 * d);
	}
	const unsigned long long mask = (1ull << (2 * b.k)) - 1;
	const bool skip = f == rv;
	const unsigned strand = f < rv ? 0u : 1u;
	int64_t span = b.k;
	if (HPC) {
		const int64_t j = std::max<int64_t>((int64_t)b.last_n[i], s0);
		const uint32_t m = b.n_valid[i] + 1 - b.n_valid[j];
		const int64_t from = (int64_t)b.bnd_pos[b.n_bnd[i] + 1 - std::min<uint32_t>(m, (uint32_t)b.k)];
		span = run_end(b, i, r) - from + 1;
	}
	b.hx[i] = (!HPC || span < 256) ? mix(strand ? rv : f, mask) << 8 | (unsigned long long)span : NONE;
	b.flags[i] = (unsigned char)(1u | (skip ? 2u : 0u) | strand << 2);
}

__global__ __launch_bounds__(TB) void k_sk_cstart(SketchBatch b)
{
	const int64_t r = (int64_t)blockIdx.x * TB + threadIdx.x;
	if (r <= b.n_seqs) b.cstart[r] = b.seq_off[r] - (int64_t)b.n_skip[b.seq_off[r]];
}

// every counted step's value, position (HPC: its run's last base) and run, at its counted index
template <bool HPC>
__global__ __launch_bounds__(TB) void k_sk_values(SketchBatch b)
{
	const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
	const bool in = i < b.n;
	const int64_t r = seg_of_block(b.seq_off, b.n_seqs, (int64_t)blockIdx.x * TB, i, in);
	if (!in) return;
	const unsigned fl = b.flags[i];
	if (fl & 2u) return;
	const int64_t g = i - (int64_t)b.n_skip[i];
	const int64_t s0 = b.seq_off[r];
	uint32_t run = 0;
	int64_t pos = i;
	if (fl & 1u) {
		const int64_t j = std::max<int64_t>((int64_t)b.last_n[i], s0);          // first position after the last N (or the sequence's first)
		run = (uint32_t)(i + 1 - j) - (b.n_skip[i + 1] - b.n_skip[j]);          // every position of [j, i] is a valid base
		if (HPC) pos = run_end(b, i, r);
	}
	b.vx[g] = ((fl & 1u) && run >= (uint32_t)b.k) ? b.hx[i] : NONE;
	b.vy[g] = (uint32_t)(pos - s0) << 1 | ((fl >> 2) & 1u);
	b.vrun[g] = std::min<uint32_t>(run, (uint32_t)(b.w + b.k));
}

// what step t of its sequence emits (seeding.cpp:82-95), from the values of steps t - w .. t
template <bool WRITE>
__global__ __launch_bounds__(TB) void k_sk_emit(SketchBatch b)
{
	const int64_t g = (int64_t)blockIdx.x * TB + threadIdx.x;
	const int64_t n_counted = b.cstart[b.n_seqs];
	const bool in = g < n_counted;
	const int64_t r = seg_of_block(b.cstart, b.n_seqs, (int64_t)blockIdx.x * TB, g, in && (int64_t)blockIdx.x * TB < n_counted);
	if (!in) { if (!WRITE && g <= b.n) b.emit_cnt[g] = 0; return; }
	const int64_t c0 = b.cstart[r];
	const int w = b.w, k = b.k;
	const int64_t t = g - c0, T = b.cstart[r + 1] - c0;
	const unsigned long long *vx = b.vx + c0;
	auto val = [&](int64_t j) { return j < 0 ? NONE : vx[j]; };
	const int run = (int)b.vrun[g];
	const unsigned long long cur = vx[t];
	uint32_t cnt = 0;
	int64_t out_at = WRITE ? b.emit_off[g] : 0;
	const unsigned long long y_hi = (unsigned long long)(b.rid ? b.rid[r] : 0u) << 32;
	auto emit = [&](int64_t j) {
		if (WRITE) { b.mini[out_at] = make_ulonglong2(vx[j], y_hi | b.vy[c0 + j]); b.mini_read[out_at] = (int32_t)r; ++out_at; }
		else ++cnt;
	};
	// the minimum before this step: the rightmost one of steps [t - w, t - 1]
	int64_t pb = t - w;
	unsigned long long px = NONE;
	if (t > 0) { px = val(pb); for (int64_t j = t - w + 1; j <= t - 1; ++j) { const unsigned long long x = val(j); if (x <= px) { px = x; pb = j; } } }
	if (run == w + k - 1 && px != NONE)                                        // the first full window: the minimum's twins
		for (int64_t j = std::max<int64_t>(t - w + 1, 0); j <= t - 1; ++j) if (vx[j] == px && j != pb) emit(j);
	int64_t nb = -1;                                                           // the minimum after this step, where it was needed
	if (cur <= px) {
		if (run >= w + k && px != NONE) emit(pb);
	} else if (pb == t - w) {                                                  // the minimum's slot is the one overwritten (t > 0: cur <= NONE otherwise)
		if (run >= w + k - 1 && px != NONE) emit(pb);
		nb = t - w + 1;
		unsigned long long qx = val(nb);
		for (int64_t j = t - w + 2; j <= t; ++j) { const unsigned long long x = val(j); if (x <= qx) { qx = x; nb = j; } }
		if (run >= w + k - 1 && qx != NONE)
			for (int64_t j = std::max<int64_t>(t - w + 1, 0); j <= t; ++j) if (vx[j] == qx && j != nb) emit(j);
	}
	if (t == T - 1) {                                                          // seeding.cpp:95
		if (nb < 0) nb = cur <= px ? t : pb;
		if (val(nb) != NONE) emit(nb);
	}
	if (!WRITE) b.emit_cnt[g] = cnt;
}

__global__ __launch_bounds__(TB) void k_sk_mini_off(SketchBatch b)
{
	const int64_t r = (int64_t)blockIdx.x * TB + threadIdx.x;
	if (r <= b.n_seqs) b.mini_off[r] = b.emit_off[b.cstart[r]];
}

// the sketch through mini_off, in either form.  (The scan of last_n reads the sequences alone: it can stand before the words in both)
template <bool HPC>
void sketch_steps(const SketchBatch &b, Pass &p)
{
	const unsigned gp = blocks(b.n + 1), gs = blocks(b.n_seqs + 1);
	const size_t n1 = (size_t)b.n + 1;
	const unsigned char *flags = b.flags;
	if (HPC) {
		p.run(k_hp_bound, gp, TB, b);
		sums(p, via(flags, RunOf()), b.n_valid, 0u, n1);
		sums(p, via(flags, BndOf()), b.n_bnd, 0u, n1);
	} else sums(p, via(b.seqs, ValidOf()), b.n_valid, 0u, n1);
	running(p, via(positions(), LastN{ b.seqs }), b.last_n, n1, rocprim::maximum<uint32_t>());
	p.run(HPC ? k_hp_compact : k_sk_compact, gp, TB, b);
	p.run(k_sk_words<HPC>, gp, TB, b);
	sums(p, via(flags, SkipOf()), b.n_skip, 0u, n1);
	p.run(k_sk_cstart, gs, TB, b);
	p.run(k_sk_values<HPC>, gp, TB, b);
	p.run(k_sk_emit<false>, gp, TB, b);
	sums(p, via((const uint32_t*)b.emit_cnt, ToI64()), (long long*)b.emit_off, 0ll, n1);
	p.run(k_sk_mini_off, gs, TB, b);
}
void sketch_steps(const SketchBatch &b, Pass &p) { if (b.hpc) sketch_steps<true>(b, p); else sketch_steps<false>(b, p); }

} // namespace

size_t sketch_layout(SketchBatch &b, void *base)
{
	Carver c(base);
	const size_t n1 = (size_t)b.n + 1, s1 = (size_t)b.n_seqs + 1;
	b.n_valid = c.take<uint32_t>(n1); b.n_skip = c.take<uint32_t>(n1); b.last_n = c.take<uint32_t>(n1);
	b.comp = c.take<unsigned char>(n1); b.flags = c.take<unsigned char>(n1);
	b.hx = c.take<unsigned long long>(n1); b.vx = c.take<unsigned long long>(n1);
	b.vy = c.take<uint32_t>(n1); b.vrun = c.take<uint32_t>(n1);
	b.cstart = c.take<int64_t>(s1);
	b.emit_cnt = c.take<uint32_t>(n1); b.emit_off = c.take<int64_t>(n1);
	b.n_bnd = b.hpc ? c.take<uint32_t>(n1) : nullptr; b.bnd_pos = b.hpc ? c.take<uint32_t>(n1 + 1) : nullptr;
	Pass measure{ nullptr, 0, 0 };
	sketch_steps(b, measure);
	b.tmp_bytes = measure.need + 256;
	b.tmp = c.take<unsigned char>(b.tmp_bytes);
	return c.at + 256;
}

int launch_sketch_count(const SketchBatch &b, hipStream_t s)
{
	Pass p{ b.tmp, b.tmp_bytes, s };
	sketch_steps(b, p);
	return p.refused ? -1 : 0;
}

void launch_sketch_write(const SketchBatch &b, hipStream_t s)
{
	hipLaunchKernelGGL(k_sk_emit<true>, dim3(blocks(b.n + 1)), dim3(TB), 0, s, b);
}

// ---------------------------------------------------------------------------------------------------------------- fragments
namespace {

// a thread per minimizer and per fragment boundary: the minimizer's sequence is found among frag_off by bisection (a fragment holds one or two sequences)
__global__ __launch_bounds__(TB) void k_f_view(FragView v)
{
	const int64_t t = (int64_t)blockIdx.x * TB + threadIdx.x;
	if (t <= v.n_frag) {
		const int64_t r0 = v.frag_off[t];
		v.f_seq_off[t] = v.seq_off[r0]; v.f_mini_off[t] = v.mini_off[r0];
		if (t < v.n_frag) v.len0[t] = v.frag_off[t + 1] - r0 > 1 ? (int32_t)(v.seq_off[r0 + 1] - v.seq_off[r0]) : INT32_MAX;
	}
	if (t >= v.n_mini) return;
	const int64_t r = v.mini_read[t];
	int64_t lo = 0, hi = v.n_frag;                                                // frag_off[lo] <= r < frag_off[hi]
	while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (v.frag_off[mid] <= r) lo = mid; else hi = mid; }
	const int64_t r0 = v.frag_off[lo];
	if (r > r0) {
		ulonglong2 q = v.mini[t];
		q.y += (unsigned long long)(v.seq_off[r] - v.seq_off[r0]) << 1 | (unsigned long long)(r - r0) << 32;     // (a sequence's own id is 0: sketch_device's rid is null here)
		v.mini[t] = q;
	}
	v.mini_read[t] = (int32_t)lo;
}

} // namespace

void launch_frag_view(const FragView &v, hipStream_t s)
{
	hipLaunchKernelGGL(k_f_view, dim3(blocks(std::max(v.n_mini, v.n_frag + 1))), dim3(TB), 0, s, v);
}

// ---------------------------------------------------------------------------------------------------------------- matches
namespace {

struct KeepQ   { __host__ __device__ uint32_t operator()(unsigned char v) const { return v ? 1u : 0u; } };
struct HasOcc  { __host__ __device__ uint32_t operator()(uint32_t n) const { return n ? 1u : 0u; } };
struct LowFwd  { const uint32_t *m_n; const int64_t *tot; uint32_t mid;
                 __device__ uint32_t operator()(uint32_t i) const { return ((int64_t)i >= tot[1] || m_n[i] <= mid) ? i + 1 : 0u; } };
struct LowRev  { const uint32_t *m_n; const int64_t *tot; uint32_t mid, last;     // position j stands for match last - j
                 __device__ uint32_t operator()(uint32_t j) const { const uint32_t i = last - j; return ((int64_t)i >= tot[1] || m_n[i] <= mid) ? i : 0xffffffffu; } };
struct KeptOf  { const unsigned char *flt; const int64_t *tot;
                 __device__ uint32_t operator()(uint32_t i) const { return ((int64_t)i < tot[1] && !flt[i]) ? 1u : 0u; } };
struct HitsOf  { const unsigned char *flt; const uint32_t *m_n; const int64_t *tot;
                 __device__ long long operator()(uint32_t i) const { return ((int64_t)i < tot[1] && !flt[i]) ? (long long)m_n[i] : 0ll; } };

__global__ __launch_bounds__(TB) void k_m_copy_x(MatchBatch b)
{
	const int64_t m = (int64_t)blockIdx.x * TB + threadIdx.x;
	if (m < b.n_mini) b.skey_in[m] = b.mini[m].x;
}

// seed.c:5-30 (seeding.cpp: the q-occurrence filter): a value that occurs c times among a read's n minimizers goes if c > mid_occ and c > n * q_occ_frac
__global__ __launch_bounds__(TB) void k_m_qflt(MatchBatch b, int active)
{
	const int64_t m = (int64_t)blockIdx.x * TB + threadIdx.x;
	if (m > b.n_mini) return;
	if (m == b.n_mini) { b.keepq[m] = 0; return; }
	unsigned char keep = 1;
	if (active) {
		const int r = b.mini_read[m];
		const int64_t s = b.mini_off[r], e = b.mini_off[r + 1], n = e - s;
		if (n > (int64_t)b.mid_occ) {
			const unsigned long long x = b.mini[m].x;
			int64_t lo = s, hi = e;                                               // first position with skey >= x
			while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (b.skey[mid] < x) lo = mid + 1; else hi = mid; }
			if (lo + b.mid_occ < e && b.skey[lo + b.mid_occ] == x) {              // more than mid_occ of them: count
				int64_t ul = lo + b.mid_occ, uh = e;                              // first position with skey > x
				while (ul < uh) { const int64_t mid = (ul + uh) >> 1; if (b.skey[mid] <= x) ul = mid + 1; else uh = mid; }
				const int32_t c = (int32_t)(ul - lo);
				if (c > b.mid_occ && (float)c > (float)(unsigned long long)n * b.q_occ_frac) keep = 0;
			}
		}
	}
	b.keepq[m] = keep;
}

__global__ __launch_bounds__(TB) void k_m_filtered(MatchBatch b)
{
	const int64_t m = (int64_t)blockIdx.x * TB + threadIdx.x;
	if (m == 0) b.tot[0] = b.fpos[b.n_mini];
	if (m >= b.n_mini || !b.keepq[m]) return;
	const uint32_t f = b.fpos[m];
	const ulonglong2 q = b.mini[m];
	b.fx[f] = q.x; b.fy[f] = (uint32_t)q.y; b.fread[f] = b.mini_read[m];
}

// seed.c:32-54: SeedIndex::find for every minimizer of the filtered list, and whether a neighbour in that list has the same value
__global__ __launch_bounds__(TB) void k_m_lookup(MatchBatch b)
{
	const int64_t f = (int64_t)blockIdx.x * TB + threadIdx.x;
	if (f > b.n_mini) return;
	const int64_t F = b.fpos[b.n_mini];
	if (f >= F) { b.l_n[f] = 0; return; }
	const unsigned long long key = b.fx[f] >> 8;
	const int rd = b.fread[f];
	uint32_t n = 0; long long first = 0;
	const unsigned long long bk = key >> b.ix.bucket_shift;
	if (bk + 1 < b.ix.n_bucket) {
		uint32_t lo = b.ix.bucket[bk];
		const uint32_t hi = b.ix.bucket[bk + 1];
		while (lo < hi && b.ix.keys[lo] < key) ++lo;                              // a prefix holds a key or two
		if (lo < hi && b.ix.keys[lo] == key) { first = b.ix.first[lo]; n = (uint32_t)(b.ix.first[lo + 1] - first); }
	}
	b.l_n[f] = n; b.l_first[f] = first;
	b.l_tan[f] = (f > 0 && b.fread[f - 1] == rd && (b.fx[f - 1] >> 8) == key) || (f + 1 < F && b.fread[f + 1] == rd && (b.fx[f + 1] >> 8) == key);
}

__global__ __launch_bounds__(TB) void k_m_matches(MatchBatch b)
{
	const int64_t f = (int64_t)blockIdx.x * TB + threadIdx.x;
	if (f == 0) b.tot[1] = b.mpos[b.n_mini];
	if (f >= b.n_mini || b.l_n[f] == 0) return;
	const uint32_t i = b.mpos[f];
	b.m_n[i] = b.l_n[f]; b.m_q[i] = b.fy[f]; b.m_span[i] = (uint32_t)(b.fx[f] & 0xff) | (b.l_tan[f] ? 1u << 31 : 0u);
	b.m_first[i] = b.l_first[f]; b.m_read[i] = b.fread[f];
}

__global__ __launch_bounds__(TB) void k_m_read_off(MatchBatch b)
{
	const int64_t r = (int64_t)blockIdx.x * TB + threadIdx.x;
	if (r > b.n_reads) return;
	b.moff[r] = b.mpos[b.fpos[b.mini_off[r]]];
	if (r < b.n_reads) b.qlen[r] = (int32_t)(b.seq_off[r + 1] - b.seq_off[r]);
}

// the streak of matches above mid_occ that match i lies in, and how many of it survive (seeding.cpp: thin_out)
struct Streak { int64_t from, to; int keep; bool alone; };
__device__ inline Streak streak_of(const MatchBatch &b, int64_t i)
{
	Streak s;
	const int r = b.m_read[i];
	const int64_t rs = b.moff[r], re = b.moff[r + 1];
	s.alone = re - rs < 2;
	s.from = std::max<int64_t>((int64_t)b.low_before[i], rs);
	s.to = std::min<int64_t>((int64_t)b.low_after[(b.n_mini - 1) - i], re);
	const int ps = s.from > rs ? (int)(b.m_q[s.from - 1] >> 1) : 0, pe = s.to < re ? (int)(b.m_q[s.to] >> 1) : b.qlen[r];
	int keep = (int)((double)(pe - ps) / b.occ_dist + .499);
	s.keep = keep > 128 ? 128 : keep;
	return s;
}

__global__ __launch_bounds__(TB) void k_m_streaks(MatchBatch b)
{
	const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
	if (i >= b.tot[1] || !(b.m_n[i] > (uint32_t)b.mid_occ)) return;
	const Streak s = streak_of(b, i);
	if (s.alone || i != s.from || s.keep <= 0 || (int64_t)s.keep >= s.to - s.from) return;
	b.streaks[atomicAdd(b.n_streaks, 1)] = make_int4((int)s.from, (int)(s.to - s.from), s.keep, 0);
}

// the K-th smallest of a streak's (n << 32 | index in the streak), bit by bit from the top: a workgroup per streak
__global__ __launch_bounds__(TB) void k_m_select(MatchBatch b)
{
	__shared__ unsigned s_cnt;
	const int n_streaks = *b.n_streaks;
	for (int q = blockIdx.x; q < n_streaks; q += gridDim.x) {
		const int4 st = b.streaks[q];
		const uint32_t *n = b.m_n + st.x;
		const int len = st.y;
		int idx_bits = 1;
		while ((1 << idx_bits) < len) ++idx_bits;
		unsigned long long prefix = 0;
		int want = st.z;                                                          // 1-based rank among the keys that share the prefix so far
		for (int bit = 63; bit >= 0; --bit) {
			if (bit < 32 && bit >= idx_bits) continue;                            // no index has these bits
			unsigned c = 0;
			for (int j = threadIdx.x; j < len; j += TB) {
				const unsigned long long key = (unsigned long long)n[j] << 32 | (unsigned)j;
				if (((key ^ prefix) >> bit >> 1) == 0 && !((key >> bit) & 1)) ++c;
			}
			for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
			if (threadIdx.x == 0) s_cnt = 0;
			__syncthreads();
			if ((threadIdx.x & 63) == 0) atomicAdd(&s_cnt, c);
			__syncthreads();
			const unsigned zeros = s_cnt;
			__syncthreads();
			if ((int)zeros < want) { prefix |= 1ull << bit; want -= (int)zeros; }
		}
		if (threadIdx.x == 0) b.thr[st.x] = prefix;
	}
}

__global__ __launch_bounds__(TB) void k_m_flt(MatchBatch b, int thin)
{
	const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
	if (i >= b.tot[1]) return;
	const uint32_t n = b.m_n[i];
	bool flt = false;
	if (n > (uint32_t)b.mid_occ) {
		if (!thin) flt = true;                                                    // seed.c:110-111
		else {
			const Streak s = streak_of(b, i);
			if (!s.alone) {                                                       // (a read with fewer than two matches is left alone)
				if (s.keep <= 0) flt = true;
				else if ((int64_t)s.keep < s.to - s.from) flt = ((unsigned long long)n << 32 | (unsigned)(i - s.from)) > b.thr[s.from];
				if (n > (uint32_t)b.max_max_occ) flt = true;
			}
		}
	}
	b.flt[i] = flt;
}

// seeding.cpp:323-339: the bases covered by a read's dropped minimizers, the state machine as written; a wave per read, the dropped ones of 64
// matches at a time
__global__ __launch_bounds__(64) void k_m_rep_len(MatchBatch b)
{
	const int l = threadIdx.x;
	for (int64_t r = blockIdx.x; r < b.n_reads; r += gridDim.x) {
		const int64_t rs = b.moff[r], re = b.moff[r + 1];
		int rep_st = 0, rep_en = 0, rep_len = 0;
		for (int64_t base = rs; base < re; base += 64) {
			const int64_t i = base + l;
			const bool dropped = i < re && b.flt[i];
			const int en = dropped ? (int)(b.m_q[i] >> 1) + 1 : 0, st = dropped ? en - (int)(b.m_span[i] & 0xff) : 0;
			unsigned long long m = __ballot(dropped);
			while (m) {
				const int src = __ffsll((long long)m) - 1;
				m &= m - 1;
				const int e = __shfl(en, src), s = __shfl(st, src);
				if (s > rep_en) { rep_len += rep_en - rep_st; rep_st = s; rep_en = e; }
				else rep_en = e;
			}
		}
		if (l == 0) b.rep_len[r] = rep_len + (rep_en - rep_st);
	}
}

__global__ __launch_bounds__(TB) void k_m_seeds(MatchBatch b)
{
	const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
	const int64_t M = b.tot[1];
	if (i == 0) { b.tot[2] = b.spos[M]; b.tot[3] = b.hpos[M]; b.hit_off[b.spos[M]] = b.hpos[M]; }
	if (i <= b.n_reads) b.seed_off[i] = b.spos[b.moff[i]];
	if (i >= M || b.flt[i]) return;
	const uint32_t s = b.spos[i], span = b.m_span[i] & 0xff, q = b.m_q[i];
	SeedRecord rec;
	const uint32_t seg = b.len0 && (int32_t)(q >> 1) >= b.len0[b.m_read[i]] ? 1u : 0u;                   // single reads: seg_id 0; a fragment's second mate lies past the first
	rec.n = b.m_n[i]; rec.q_pos = q; rec.span_flt = span; rec.seg_tandem = (b.m_span[i] & (1u << 31)) | seg;
	b.seeds[s] = rec;
	b.mini_pos[s] = (unsigned long long)span << 32 | q >> 1;
	b.hit_off[s] = b.hpos[i];
	b.src_first[s] = b.m_first[i];
}

// without minimizers: offsets and counts of nothing
__global__ __launch_bounds__(TB) void k_m_empty(MatchBatch b)
{
	const int64_t r = (int64_t)blockIdx.x * TB + threadIdx.x;
	if (r == 0) { b.tot[0] = b.tot[1] = b.tot[2] = b.tot[3] = 0; b.hit_off[0] = 0; }
	if (r <= b.n_reads) b.seed_off[r] = 0;
	if (r < b.n_reads) { b.rep_len[r] = 0; b.qlen[r] = (int32_t)(b.seq_off[r + 1] - b.seq_off[r]); }
}

// every kept seed's occurrences, copied from the index: a wave takes 64 seeds, whose hits are one run of the output; a lane finds its hit's seed
// among the 64 offsets (long runs are split over the lanes, short ones packed into them)
__global__ __launch_bounds__(64) void k_m_gather(MatchBatch b, int64_t n_groups)
{
	__shared__ int64_t s_off[65];
	__shared__ long long s_src[64];
	const int l = threadIdx.x;
	const int64_t S = b.tot[2];
	for (int64_t grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
		const int64_t s0 = grp * 64;
		if (s0 >= S) break;
		__syncthreads();
		s_off[l] = b.hit_off[std::min<int64_t>(s0 + l, S)];
		if (l == 0) s_off[64] = b.hit_off[std::min<int64_t>(s0 + 64, S)];
		s_src[l] = s0 + l < S ? b.src_first[s0 + l] : 0;
		__syncthreads();
		const int64_t h0 = s_off[0], h1 = s_off[64];
		for (int64_t h = h0 + l; h < h1; h += 64) {
			int lo = 0, hi = 64;                                                  // s_off[lo] <= h < s_off[hi]
			while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (s_off[mid] <= h) lo = mid; else hi = mid; }
			b.hits[h] = b.ix.where[s_src[lo] + (h - s_off[lo])];
		}
	}
}

// the match selection: everything but the hits.  The steps under a condition are sized under it: the options are set before match_layout
void match_steps(const MatchBatch &b, Pass &p)
{
	const unsigned gr = blocks(b.n_reads + 1), gm = blocks(b.n_mini + 1);
	if (b.n_mini <= 0) { p.run(k_m_empty, gr, TB, b); return; }
	const size_t n = (size_t)b.n_mini, n1 = n + 1;
	const int qflt = b.q_occ_frac > 0.0f && b.mid_occ > 0;
	if (qflt) {
		p.run(k_m_copy_x, gm, TB, b);
		p.lib([&](void *t, size_t &q) { return rocprim::segmented_radix_sort_keys(t, q, b.skey_in, b.skey, (unsigned)b.n_mini, (unsigned)std::max<int64_t>(b.n_reads, 1), b.mini_off, b.mini_off + 1, 0, 64, p.s); });
	}
	p.run(k_m_qflt, gm, TB, b, qflt);
	sums(p, via((const unsigned char*)b.keepq, KeepQ()), b.fpos, 0u, n1);
	p.run(k_m_filtered, gm, TB, b);
	p.run(k_m_lookup, gm, TB, b);
	sums(p, via((const uint32_t*)b.l_n, HasOcc()), b.mpos, 0u, n1);
	p.run(k_m_matches, gm, TB, b);
	p.run(k_m_read_off, gr, TB, b);
	const int thin = b.occ_dist > 0 && b.max_max_occ > b.mid_occ;                 // seed.c:105-111
	if (thin) {
		running(p, via(positions(), LowFwd{ b.m_n, b.tot, (uint32_t)b.mid_occ }), b.low_before, n, rocprim::maximum<uint32_t>());
		running(p, via(positions(), LowRev{ b.m_n, b.tot, (uint32_t)b.mid_occ, (uint32_t)(b.n_mini - 1) }), b.low_after, n, rocprim::minimum<uint32_t>());
		if (p.launching()) (void)hipMemsetAsync(b.n_streaks, 0, sizeof(int32_t), p.s);
		p.run(k_m_streaks, gm, TB, b);
		p.run(k_m_select, (unsigned)std::min<int64_t>(b.n_mini / 2 + 1, 8192), TB, b);
	}
	p.run(k_m_flt, gm, TB, b, thin);
	p.run(k_m_rep_len, (unsigned)std::min<int64_t>(std::max<int64_t>(b.n_reads, 1), 16384), 64, b);
	sums(p, via(positions(), KeptOf{ b.flt, b.tot }), b.spos, 0u, n1);
	sums(p, via(positions(), HitsOf{ b.flt, b.m_n, b.tot }), (long long*)b.hpos, 0ll, n1);
	p.run(k_m_seeds, blocks(std::max(b.n_mini, b.n_reads) + 1), TB, b);
}

} // namespace

size_t match_layout(MatchBatch &b, void *base)
{
	Carver c(base);
	const size_t n1 = (size_t)b.n_mini + 1, r1 = (size_t)b.n_reads + 1;
	b.skey_in = c.take<unsigned long long>(n1); b.skey = c.take<unsigned long long>(n1);
	b.keepq = c.take<unsigned char>(n1); b.fpos = c.take<uint32_t>(n1);
	b.fx = c.take<unsigned long long>(n1); b.fy = c.take<uint32_t>(n1); b.fread = c.take<int32_t>(n1);
	b.l_n = c.take<uint32_t>(n1); b.l_first = c.take<long long>(n1); b.l_tan = c.take<unsigned char>(n1);
	b.mpos = c.take<uint32_t>(n1);
	b.m_n = c.take<uint32_t>(n1); b.m_q = c.take<uint32_t>(n1); b.m_span = c.take<uint32_t>(n1); b.m_first = c.take<long long>(n1); b.m_read = c.take<int32_t>(n1);
	b.moff = c.take<int64_t>(r1);
	b.low_before = c.take<uint32_t>(n1); b.low_after = c.take<uint32_t>(n1);
	b.streaks = c.take<int4>(n1 / 2 + 1); b.n_streaks = c.take<int32_t>(4);
	b.thr = c.take<unsigned long long>(n1);
	b.flt = c.take<unsigned char>(n1);
	b.spos = c.take<uint32_t>(n1); b.hpos = c.take<int64_t>(n1);
	b.tot = c.take<int64_t>(4);
	Pass measure{ nullptr, 0, 0 };
	match_steps(b, measure);
	b.tmp_bytes = measure.need + 256;
	b.tmp = c.take<unsigned char>(b.tmp_bytes);
	return c.at + 256;
}

int launch_matches_select(const MatchBatch &b, hipStream_t s)
{
	Pass p{ b.tmp, b.tmp_bytes, s };
	match_steps(b, p);
	return p.refused ? -1 : 0;
}

void launch_matches_gather(const MatchBatch &b, hipStream_t s)
{
	const int64_t n_groups = (b.n_mini + 63) / 64;                                // (an upper bound: the kernel stops at the seeds there are)
	if (n_groups <= 0) return;
	hipLaunchKernelGGL(k_m_gather, dim3((unsigned)std::min<int64_t>(n_groups, 65536)), dim3(64), 0, s, b, n_groups);
}

} // namespace mm2gb
