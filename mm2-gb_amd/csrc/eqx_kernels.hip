// eqx_kernels.hip -- the device form of the = / X rewrite (mm2gb_cigar_eqx_gpu).  The call is checked and laid out by tx_prepare, the
// text kernels' plan (aln_text_host.cpp): every record is cut into slices of EQ_SLICE columns, a cut may fall inside a word, and a workgroup takes
// one slice whatever record it is from.  Whether a column is a START (eqx.h) depends on the column and the one before it in its word alone, never
// on where the cuts fall; what crosses a cut is only how far the next start lies.  Three steps:
//   count  (k_eqx_count)  a column per thread and round: the column's word by a search of the slice's word starts in LDS, its residues and those of
//          the column before it from the resident bytes, hence start and equality.  A ballot per wave gives 64 columns' starts and equalities as
//          two words, which are KEPT (the write step reads no residue again); their popcounts give the slice's number of starts, the lowest bit
//          of the first non-empty one its number of columns before the first start.
//   carry  (k_eqx_carry)  a thread per record walks its slices backwards: how many columns after a slice's end the next start lies (a run may
//          cross several cuts without a start; the record's end closes the last).  A scan of the counts gives every slice's destination.
//   write  (k_eqx_write)  every start column stores its word once at its final place: its slot from the popcounts below it, the length of an
//          = / X run from the next start at or above it -- in its wave's word, else in the slice's later words, else beyond the cut.
// No atomics, no scratch, every word stored once.  An N word is ONE column (tx_prepare counts it so), so a cut never falls inside it.
#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "engine.h"
#include "align_host.h"
#include "eqx.h"
#include "host_chain.h"

namespace mm2gb {

constexpr int EQ_GROUPS = EQ_SLICE / 64;     // wave-sized groups of columns in a slice: a start word and an equality word each

// what the count step leaves per slice: its starts, the columns before the first one (all of them where it has none), whether it has one
struct EqCnt { int32_t n, lead, any, pad; };

__global__ __launch_bounds__(EQ_WG) void k_eqx_count(int n_slices, const TxRec *__restrict__ recs, const TxSlice *__restrict__ slices, const TxWord *__restrict__ words,
                                                     const uint8_t *__restrict__ refs, const uint8_t *__restrict__ reads, uint64_t *__restrict__ mask, EqCnt *__restrict__ cnt)
{
	__shared__ int32_t s_col[EQ_SLICE];                              // where the slice's words start
	__shared__ int32_t s_n[EQ_GROUPS], s_first[EQ_GROUPS];           // per group: its starts, the column of its first one (-1: none)
	if ((int)blockIdx.x >= n_slices) return;
	const TxSlice sl = slices[blockIdx.x];
	const TxRec rc = recs[sl.rec];
	const TxWord *W = words + rc.w_off;
	const int tid = (int)threadIdx.x, lane = tid & 63;
	uint64_t *M = mask + (size_t)blockIdx.x * 2 * EQ_GROUPS;
	for (int i = tid; i < sl.n_w; i += EQ_WG) s_col[i] = W[sl.w_first + i].col;
	__syncthreads();
	int n_groups = 0;
	for (int base = 0; base < sl.n; base += EQ_WG) {
		const int k = base + tid, g = k >> 6;
		bool start = false, eq = false;
		if (k < sl.n) {
			const int c = sl.start + k;
			int lo = 0, hi = sl.n_w - 1;                             // the last word that starts at or before c
			while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (s_col[mid] <= c) lo = mid; else hi = mid - 1; }
			const TxWord w = W[sl.w_first + lo];
			const int j = c - w.col;
			start = j == 0;
			if ((w.w & 0xf) == 0) {
				eq = refs[rc.t_at + w.t + j] == tx_query(reads, rc.q_at, rc.rev, w.q + j);
				if (j > 0) start = eq != (refs[rc.t_at + w.t + j - 1] == tx_query(reads, rc.q_at, rc.rev, w.q + j - 1));
			}
		}
		const uint64_t ms = __ballot(start), me = __ballot(eq);
		if (lane == 0) { M[g] = ms; M[EQ_GROUPS + g] = me; s_n[g] = __popcll(ms); s_first[g] = ms ? g * 64 + (int)__builtin_ctzll(ms) : -1; }
		n_groups += EQ_WG / 64;
	}
	__syncthreads();
	if (tid == 0) {
		int n = 0, lead = -1;
		for (int g = 0; g < n_groups; ++g) { n += s_n[g]; if (lead < 0) lead = s_first[g]; }
		cnt[blockIdx.x] = { n, lead < 0 ? sl.n : lead, lead >= 0 ? 1 : 0, 0 };
	}
}

// a thread per record: how far beyond every slice's end the next start lies, the slices' word counts (count[n_slices] = 0 for the scan's total)
__global__ __launch_bounds__(64) void k_eqx_carry(int n_recs, int n_slices, const TxRec *__restrict__ recs, const EqCnt *__restrict__ cnt, int32_t *__restrict__ tail,
                                                  int64_t *__restrict__ count)
{
	const int i = blockIdx.x * 64 + threadIdx.x;
	if (i == 0) count[n_slices] = 0;
	if (i >= n_recs) return;
	const TxRec rc = recs[i];
	const int s0 = rc.s_first + rc.n_cg_slices;
	int beyond = 0;
	for (int x = rc.n_tag_slices - 1; x >= 0; --x) {
		const EqCnt c = cnt[s0 + x];
		tail[s0 + x] = beyond; count[s0 + x] = c.n;
		beyond = c.any ? c.lead : beyond + c.lead;
	}
	for (int x = 0; x < rc.n_cg_slices; ++x) { tail[rc.s_first + x] = 0; count[rc.s_first + x] = 0; }
}

__global__ __launch_bounds__(EQ_WG) void k_eqx_write(int n_slices, const TxRec *__restrict__ recs, const TxSlice *__restrict__ slices, const TxWord *__restrict__ words,
                                                     const uint64_t *__restrict__ mask, const int32_t *__restrict__ tail, const int64_t *__restrict__ dest, uint32_t *__restrict__ out)
{
	__shared__ int32_t s_col[EQ_SLICE];
	__shared__ int32_t s_pre[EQ_GROUPS], s_next[EQ_GROUPS];          // per group: the slice's starts before it, the column of the first start after it
	if ((int)blockIdx.x >= n_slices) return;
	const TxSlice sl = slices[blockIdx.x];
	if (sl.kind == 0) return;
	const TxRec rc = recs[sl.rec];
	const TxWord *W = words + rc.w_off;
	const int tid = (int)threadIdx.x, lane = tid & 63;
	const uint64_t *M = mask + (size_t)blockIdx.x * 2 * EQ_GROUPS;
	const int64_t pos = dest[blockIdx.x], lim = dest[blockIdx.x + 1];
	const int n_groups = (sl.n + EQ_WG - 1) / EQ_WG * (EQ_WG / 64);
	for (int i = tid; i < sl.n_w; i += EQ_WG) s_col[i] = W[sl.w_first + i].col;
	if (tid < n_groups) {
		int pre = 0, next = sl.n + tail[blockIdx.x];
		for (int x = 0; x < tid; ++x) pre += __popcll(M[x]);
		for (int x = n_groups - 1; x > tid; --x) if (M[x]) next = x * 64 + (int)__builtin_ctzll(M[x]);
		s_pre[tid] = pre; s_next[tid] = next;
	}
	__syncthreads();
	for (int base = 0; base < sl.n; base += EQ_WG) {
		const int k = base + tid, g = k >> 6;
		const uint64_t ms = M[g], me = M[EQ_GROUPS + g];
		if (k >= sl.n || !(ms >> lane & 1)) continue;
		const uint64_t above = lane == 63 ? 0 : ms >> (lane + 1) << (lane + 1);
		const int next = above ? g * 64 + (int)__builtin_ctzll(above) : s_next[g];
		const int64_t slot = pos + s_pre[g] + __popcll(ms & (((uint64_t)1 << lane) - 1));
		const int c = sl.start + k;
		int lo = 0, hi = sl.n_w - 1;
		while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (s_col[mid] <= c) lo = mid; else hi = mid - 1; }
		const uint32_t w = W[sl.w_first + lo].w;
		if (slot < lim) out[slot] = (w & 0xf) == 0 ? (uint32_t)(next - k) << 4 | (me >> lane & 1 ? 7u : 8u) : w;
	}
}

namespace {
// of this thread's last call, as Engine::tx_s: residues up, the host's pass over the words, words up + kernels, the new words back
thread_local double eq_s[4] = { 0, 0, 0, 0 };
using clk = std::chrono::steady_clock;
inline double since(clk::time_point t0) { return std::chrono::duration<double>(clk::now() - t0).count(); }
}

int cigar_eqx_resident(Engine &e, const char *who_, int32_t n_ref, const int32_t *ref_lens, const int64_t *ref_at, int64_t n_reads, const int32_t *read_lens, const int64_t *read_at,
                       int64_t n_regs, const mm2gb_reg_t *regs, const int32_t *read_of_reg, const mm2gb_aln_t *aln, const uint32_t *cigar, mm2gb_aln_t **aln_out, uint32_t **cigar_out)
{
	const std::string who = who_;
	if (!aln_out || !cigar_out) return fail(who + ": null argument");
	*aln_out = nullptr; *cigar_out = nullptr;
	TxPlan p;
	auto t0 = clk::now();
	// The call runs on the text call's plan and buffers (tx_cnt: its counts, tx_run: the distance to the next start beyond a slice, tx_text: the new words); the
	// slices' start and equality bits lie in al_list, the alignment call's scratch, which every alignment call writes anew.
	eq_s[0] = eq_s[1] = eq_s[2] = eq_s[3] = 0;
	if (eqx_prepare(who, n_ref, ref_lens, ref_at, n_reads, read_lens, read_at, n_regs, regs, read_of_reg, aln, cigar, EQ_SLICE, p)) return -1;
	eq_s[1] = since(t0);
	t0 = clk::now();
	const size_t n_recs = p.recs.size(), n_sl = p.slices.size();
	std::vector<int64_t> dest(n_sl + 1, 0);
	if (n_sl > 0) {
		MM2GB_HIP(hipSetDevice(e.device));
		size_t tmp = 0;
		MM2GB_HIP(rocprim::exclusive_scan(nullptr, tmp, (int64_t*)nullptr, (int64_t*)nullptr, (int64_t)0, n_sl + 1, rocprim::plus<int64_t>(), e.stream));
		if (e.tx_recs.ensure(n_recs * sizeof(TxRec)) || e.tx_words.ensure(std::max<size_t>(p.words.size(), 1) * sizeof(TxWord)) || e.tx_slices.ensure(n_sl * sizeof(TxSlice)) ||
		    e.tx_cnt.ensure(n_sl * sizeof(EqCnt)) || e.tx_run.ensure(n_sl * 4) || e.tx_bytes.ensure((n_sl + 1) * 8) || e.tx_dest.ensure((n_sl + 1) * 8) || e.tx_tmp.ensure(std::max<size_t>(tmp, 16)) ||
		    e.al_list.ensure(n_sl * 2 * EQ_GROUPS * sizeof(uint64_t))) return -1;
		MM2GB_HIP(hipMemcpyAsync(e.tx_recs.ptr, p.recs.data(), n_recs * sizeof(TxRec), hipMemcpyHostToDevice, e.stream));
		if (!p.words.empty()) MM2GB_HIP(hipMemcpyAsync(e.tx_words.ptr, p.words.data(), p.words.size() * sizeof(TxWord), hipMemcpyHostToDevice, e.stream));
		MM2GB_HIP(hipMemcpyAsync(e.tx_slices.ptr, p.slices.data(), n_sl * sizeof(TxSlice), hipMemcpyHostToDevice, e.stream));
		hipLaunchKernelGGL(k_eqx_count, dim3((unsigned)n_sl), dim3(EQ_WG), 0, e.stream, (int)n_sl, (const TxRec*)e.tx_recs.ptr, (const TxSlice*)e.tx_slices.ptr, (const TxWord*)e.tx_words.ptr,
		                   (const uint8_t*)e.al_refs.ptr, (const uint8_t*)e.al_reads.ptr, (uint64_t*)e.al_list.ptr, (EqCnt*)e.tx_cnt.ptr);
		MM2GB_HIP(hipGetLastError());
		hipLaunchKernelGGL(k_eqx_carry, dim3((unsigned)((n_recs + 63) / 64)), dim3(64), 0, e.stream, (int)n_recs, (int)n_sl, (const TxRec*)e.tx_recs.ptr, (const EqCnt*)e.tx_cnt.ptr,
		                   (int32_t*)e.tx_run.ptr, (int64_t*)e.tx_bytes.ptr);
		MM2GB_HIP(hipGetLastError());
		MM2GB_HIP(rocprim::exclusive_scan(e.tx_tmp.ptr, tmp, (int64_t*)e.tx_bytes.ptr, (int64_t*)e.tx_dest.ptr, (int64_t)0, n_sl + 1, rocprim::plus<int64_t>(), e.stream));
		MM2GB_HIP(hipMemcpyAsync(dest.data(), e.tx_dest.ptr, (n_sl + 1) * 8, hipMemcpyDeviceToHost, e.stream));
		MM2GB_HIP(hipStreamSynchronize(e.stream));
	}
	const int64_t total = dest[n_sl];
	std::vector<int64_t> n_words(n_recs);
	for (size_t k = 0; k < n_recs; ++k) n_words[k] = dest[(size_t)p.recs[k].s_first + (size_t)p.recs[k].n_tag_slices] - dest[(size_t)p.recs[k].s_first];
	if (eqx_results(who, p, n_regs, aln, n_words.data(), aln_out, cigar_out)) return -1;
	struct Free { mm2gb_aln_t **a; uint32_t **w; bool keep = false; ~Free() { if (!keep) { free(*a); free(*w); *a = nullptr; *w = nullptr; } } } guard{ aln_out, cigar_out };
	if (total > 0) {
		if (e.tx_text.ensure((size_t)total * sizeof(uint32_t))) return -1;
		hipLaunchKernelGGL(k_eqx_write, dim3((unsigned)n_sl), dim3(EQ_WG), 0, e.stream, (int)n_sl, (const TxRec*)e.tx_recs.ptr, (const TxSlice*)e.tx_slices.ptr, (const TxWord*)e.tx_words.ptr,
		                   (const uint64_t*)e.al_list.ptr, (const int32_t*)e.tx_run.ptr, (const int64_t*)e.tx_dest.ptr, (uint32_t*)e.tx_text.ptr);
		MM2GB_HIP(hipGetLastError());
		MM2GB_HIP(hipStreamSynchronize(e.stream));
		eq_s[2] = since(t0);
		t0 = clk::now();
		MM2GB_HIP(hipMemcpy(*cigar_out, e.tx_text.ptr, (size_t)total * sizeof(uint32_t), hipMemcpyDeviceToHost));
		eq_s[3] = since(t0);
	} else eq_s[2] = since(t0);
	guard.keep = true;
	return 0;
}

} // namespace mm2gb

using namespace mm2gb;

int mm2gb_cigar_eqx_gpu(mm2gb_engine_t *eng, int32_t n_ref, const char *const *ref_seqs, const int32_t *ref_lens, int64_t n_reads, const char *const *read_seqs, const int32_t *read_lens,
                        int64_t n_regs, const mm2gb_reg_t *regs, const int32_t *read_of_reg, const mm2gb_aln_t *aln, const uint32_t *cigar, mm2gb_aln_t **aln_out, uint32_t **cigar_out)
{
	const std::string who = "mm2gb_cigar_eqx_gpu";
	if (!eng) return fail("mm2gb: null engine");
	if (!aln_out || !cigar_out || n_ref < 0 || n_reads < 0 || (n_ref > 0 && (!ref_seqs || !ref_lens)) || (n_reads > 0 && (!read_seqs || !read_lens))) return fail(who + ": null argument");
	*aln_out = nullptr; *cigar_out = nullptr;
	Engine &e = eng->e;
	for (int32_t i = 0; i < n_ref; ++i) if (ref_lens[i] < 0) return fail(who + ": a negative length");
	for (int64_t i = 0; i < n_reads; ++i) if (read_lens[i] < 0) return fail(who + ": a negative length");
	// the residues, one byte per base, as the alignment call keeps them
	const auto t0 = clk::now();
	std::vector<int64_t> ref_at, read_at;
	std::vector<uint8_t> refs, reads;
	pack_residues(n_ref, ref_seqs, ref_lens, n_reads, read_seqs, read_lens, std::min(usable_cpus(), 16), ref_at, read_at, refs, reads);
	MM2GB_HIP(hipSetDevice(e.device));
	if (e.al_refs.ensure(std::max<size_t>(refs.size(), 16)) || e.al_reads.ensure(std::max<size_t>(reads.size(), 16))) return -1;
	if (!refs.empty()) MM2GB_HIP(hipMemcpyAsync(e.al_refs.ptr, refs.data(), refs.size(), hipMemcpyHostToDevice, e.stream));
	if (!reads.empty()) MM2GB_HIP(hipMemcpyAsync(e.al_reads.ptr, reads.data(), reads.size(), hipMemcpyHostToDevice, e.stream));
	MM2GB_HIP(hipStreamSynchronize(e.stream));
	e.al_resident[0] = (int64_t)refs.size(); e.al_resident[1] = (int64_t)reads.size();
	const double s_up = since(t0);
	const int rc = cigar_eqx_resident(e, who.c_str(), n_ref, ref_lens, ref_at.data(), n_reads, read_lens, read_at.data(), n_regs, regs, read_of_reg, aln, cigar, aln_out, cigar_out);
	eq_s[0] = s_up;
	return rc;
}

int mm2gb_cigar_eqx_gpu_info(mm2gb_engine_t *eng, int64_t *consts2, double *s4)
{
	if (!eng || !consts2) return fail("mm2gb_cigar_eqx_gpu_info: null argument");
	consts2[0] = EQ_SLICE; consts2[1] = EQ_WG;
	if (s4) for (int i = 0; i < 4; ++i) s4[i] = eq_s[i];
	return 0;
}
