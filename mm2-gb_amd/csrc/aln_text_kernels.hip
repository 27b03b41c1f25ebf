// aln_text_kernels.hip -- the device form of the alignment tags' text (mm2gb_aln_text_gpu).  The call is checked and laid out by
// aln_text_host.cpp (tx_prepare): every record is cut into slices of TX_SLICE columns (CIGAR words, for cg:Z), a cut may fall inside a word,
// and a workgroup takes one slice whatever record it is from, so the work is balanced by columns.  Three steps:
//   count  (k_tx_pass<false>)  a column per thread and round: the column's word by a search of the slice's word starts in LDS, its residues from
//          the resident bytes (neighbouring threads read neighbouring bytes, downwards on the reverse strand), the rule of aln_text_cell.h, the
//          run length before every event from scans over the wave (DPP) and the workgroup (LDS).  Leaves the slice's byte count WITHOUT the
//          length its first event prints, and its carry: the matches before its first event, after its last one, whether it had one.
//   carry  (k_tx_carry)  a thread per record walks its slices' carries: the run open at every cut (it may cross several slices without an
//          event), hence the digits of the first length of every slice and of the record's last; then a scan gives every slice's destination.
//   write  (k_tx_pass<true>)  the same computation with the open run at the cut known; every column stores its bytes at their final place, the
//          event that closes a run the whole number.
// No atomics, no scratch, every byte stored once.
// The spliced calls (SPLICE): an N word is ONE column (tx_prepare counts it so, and its target position moves on by the word's length), so a cut
// falls before or after it, never inside; the column is an event in cs:Z with own bytes of its own length (tx_intron_*), nothing in MD:Z.
// The carry step sees events and counts only and is the same.  A batch of the spliced calls without an N word runs the plain instantiation.
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
#include "aln_text_host.h"
#include "host_chain.h"
#include "wave_scan.h"

namespace mm2gb {

constexpr int TX_SLICE = 2048;          // columns (words) of a slice
constexpr int TX_WG = 256;              // threads of a workgroup: a round takes TX_WG columns
constexpr int TX_WAVES = TX_WG / 64;

// what the count step leaves per slice
struct TxCnt { int32_t bytes, lead, trail, any; };

// v summed over this lane and the lanes below it (the pattern of wave_scan.h)
__device__ __forceinline__ int wave_sum_incl(int v)
{
	v += dpp_or<DPP_ROW_SHR + 1>(v, 0); v += dpp_or<DPP_ROW_SHR + 2>(v, 0); v += dpp_or<DPP_ROW_SHR + 4>(v, 0); v += dpp_or<DPP_ROW_SHR + 8>(v, 0);
	const int t0 = __builtin_amdgcn_readlane(v, 15), t1 = t0 + __builtin_amdgcn_readlane(v, 31), t2 = t1 + __builtin_amdgcn_readlane(v, 47);
	const int row = scan_lane() >> 4;
	return v + (row == 0 ? 0 : row == 1 ? t0 : row == 2 ? t1 : t2);
}

template <bool WRITE, bool SPLICE>
__global__ __launch_bounds__(TX_WG) void k_tx_pass(int mode, int n_slices, const TxRec *__restrict__ recs, const TxSlice *__restrict__ slices, const TxWord *__restrict__ words,
                                                   const uint8_t *__restrict__ refs, const uint8_t *__restrict__ reads, TxCnt *__restrict__ cnt,
                                                   const int32_t *__restrict__ run_in, const int64_t *__restrict__ dest, char *__restrict__ text)
{
	__shared__ int32_t s_col[TX_SLICE];                              // where the slice's words start
	__shared__ int32_t s_m[2][TX_WAVES], s_ev[2][TX_WAVES], s_tr[2][TX_WAVES], s_by[2][TX_WAVES];      // per wave of a round: matches, had an event, matches after its last event, bytes
	__shared__ int32_t s_lead;
	if ((int)blockIdx.x >= n_slices) return;
	const TxSlice sl = slices[blockIdx.x];
	const TxRec rc = recs[sl.rec];
	const TxWord *W = words + rc.w_off;
	const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
	int64_t pos = WRITE ? dest[blockIdx.x] : 0;
	const int64_t lim = WRITE ? dest[blockIdx.x + 1] : 0;
	auto put = [&](int64_t p, char ch) { if (WRITE && p < lim) text[p] = ch; };
	int total = 0;
	if (sl.start == 0) {                                             // the record's first slice of its kind writes the tag's name
		const char *name = sl.kind == 0 ? "\tcg:Z:" : mode == TX_MD ? "\tMD:Z:" : "\tcs:Z:";
		if (tid < 6) put(pos + tid, name[tid]);
		pos += 6; total = 6;
	}
	if (sl.kind == 0) {
		for (int base = 0, it = 0; base < sl.n; base += TX_WG, ++it) {
			const int k = base + tid, p = it & 1;
			const uint32_t w = k < sl.n ? W[sl.start + k].w : 0;
			const int b = k < sl.n ? tx_word_bytes(w) : 0, upto = wave_sum_incl(b);
			if (lane == 63) s_by[p][wv] = upto;
			__syncthreads();
			int off = 0, all = 0;
			for (int x = 0; x < TX_WAVES; ++x) { if (x < wv) off += s_by[p][x]; all += s_by[p][x]; }
			if (k < sl.n) tx_put_word(w, pos + off + upto - b, put);
			pos += all; total += all;
		}
		if (!WRITE && tid == 0) cnt[blockIdx.x] = { total, 0, 0, 0 };
		return;
	}
	for (int i = tid; i < sl.n_w; i += TX_WG) s_col[i] = W[sl.w_first + i].col;
	if (tid == 0) s_lead = 0;
	__syncthreads();
	int run = WRITE ? run_in[blockIdx.x] : 0;                        // the run open before the round's first column (the same in every thread)
	bool any = false;                                                // an event so far
	for (int base = 0, it = 0; base < sl.n; base += TX_WG, ++it) {
		const int k = base + tid, p = it & 1;
		TxCol col;
		col.ev = col.m = col.n_own = 0; col.own[0] = col.own[1] = col.own[2] = 0;
		uint32_t intron = 0;                                     // SPLICE: the length of the N word this column is, and its first and last two target residues
		int i0 = 0, i1 = 0, i2 = 0, i3 = 0;
		if (k < sl.n) {
			const int c = sl.start + k;
			int lo = 0, hi = sl.n_w - 1;                             // the last word that starts at or before c
			while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (s_col[mid] <= c) lo = mid; else hi = mid - 1; }
			const TxWord w = W[sl.w_first + lo];
			const int op = (int)(w.w & 0xf), j = c - w.col;
			if (SPLICE && op == 3) {
				if (mode != TX_MD) {
					const int64_t at = rc.t_at + w.t;
					intron = w.w >> 4; col.ev = mode == TX_CS;
					i0 = refs[at]; i1 = refs[at + 1]; i2 = refs[at + intron - 2]; i3 = refs[at + intron - 1];
				}
			} else {
				const int t = op != 1 ? refs[rc.t_at + w.t + j] : 0, q = op != 2 ? tx_query(reads, rc.q_at, rc.rev, w.q + j) : 0;
				bool prev = false;
				if (mode == TX_CS_LONG && op == 0 && j > 0) prev = refs[rc.t_at + w.t + j - 1] == tx_query(reads, rc.q_at, rc.rev, w.q + j - 1);
				col = tx_col(mode, op, j == 0, t, q, prev);
			}
		}
		// the run before this column: the matches since the last event below it in the wave, or else since the wave began plus what was open there
		const int m = col.m, upto_m = wave_sum_incl(m), before_m = upto_m - m;
		const int mark = col.ev ? before_m : -1, below = wave_max_below(mark), last = max(below, mark);
		const int wave_m = __builtin_amdgcn_readlane(upto_m, 63), wave_last = __builtin_amdgcn_readlane(last, 63);
		if (lane == 63) { s_m[p][wv] = wave_m; s_ev[p][wv] = wave_last >= 0; s_tr[p][wv] = wave_last >= 0 ? wave_m - wave_last : wave_m; }
		__syncthreads();
		int open = run, run_next = run;
		bool any_here = any, any_next = any;
		for (int x = 0; x < TX_WAVES; ++x) {
			if (x == wv) { open = run_next; any_here = any_next; }
			run_next = s_ev[p][x] ? s_tr[p][x] : run_next + s_tr[p][x];
			any_next = any_next || s_ev[p][x];
		}
		const int len = below >= 0 ? before_m - below : open + before_m;
		// count step: the slice's first event prints a length that the cut's open run is part of; it is left to the carry step
		const bool first_ev = !WRITE && col.ev && below < 0 && !any_here;
		if (first_ev) s_lead = len;
		const int nb = col.ev && !first_ev ? tx_len_bytes(mode, false, len) : 0;
		const int b = nb + col.n_own + (SPLICE && intron ? tx_intron_bytes(intron) : 0), upto = wave_sum_incl(b);
		if (lane == 63) s_by[p][wv] = upto;
		__syncthreads();
		int off = 0, all = 0;
		for (int x = 0; x < TX_WAVES; ++x) { if (x < wv) off += s_by[p][x]; all += s_by[p][x]; }
		if (WRITE) {
			int64_t at = pos + off + upto - b;
			if (col.ev) tx_put_len(mode, false, len, at, put);
			at += nb;
			if (col.n_own > 0) put(at, col.own[0]);
			if (col.n_own > 1) put(at + 1, col.own[1]);
			if (col.n_own > 2) put(at + 2, col.own[2]);
			if (SPLICE && intron) tx_put_intron(intron, i0, i1, i2, i3, at, put);
		}
		pos += all; total += all; run = run_next; any = any_next;
	}
	if (WRITE) {
		if (sl.start + sl.n == rc.n_cols && tid == 0) tx_put_len(mode, true, run, pos, put);       // the record's end closes its last run
	} else {
		__syncthreads();
		if (tid == 0) cnt[blockIdx.x] = { total, any ? s_lead : run, run, any ? 1 : 0 };
	}
}

// a thread per record: the run open at every cut, the slices' final byte counts (bytes[n_slices] = 0 for the scan's total)
__global__ __launch_bounds__(64) void k_tx_carry(int mode, int n_recs, int n_slices, const TxRec *__restrict__ recs, const TxCnt *__restrict__ cnt, int32_t *__restrict__ run_in,
                                                 int64_t *__restrict__ bytes)
{
	const int i = blockIdx.x * 64 + threadIdx.x;
	if (i == 0) bytes[n_slices] = 0;
	if (i >= n_recs) return;
	const TxRec rc = recs[i];
	int s = rc.s_first, run = 0;
	for (int x = 0; x < rc.n_cg_slices; ++x, ++s) { bytes[s] = cnt[s].bytes; run_in[s] = 0; }
	for (int x = 0; x < rc.n_tag_slices; ++x, ++s) {
		const TxCnt c = cnt[s];
		run_in[s] = run;
		int b = c.bytes + (c.any ? tx_len_bytes(mode, false, run + c.lead) : 0);
		run = c.any ? c.trail : run + c.trail;
		if (x == rc.n_tag_slices - 1) b += tx_len_bytes(mode, true, run);
		bytes[s] = b;
	}
}

namespace {
using clk = std::chrono::steady_clock;
inline double since(clk::time_point t0) { return std::chrono::duration<double>(clk::now() - t0).count(); }
}

int aln_text_resident(Engine &e, bool splice, const char *who_, int what, int32_t n_ref, const int32_t *ref_lens, const int64_t *ref_at, int64_t n_reads, const int32_t *read_lens,
                      const int64_t *read_at, int64_t n_regs, const mm2gb_reg_t *regs, const int32_t *read_of_reg, const mm2gb_aln_t *aln, const uint32_t *cigar,
                      int64_t **text_off, char **text)
{
	const std::string who = who_;
	if (!text_off || !text) return fail(who + ": null argument");
	*text_off = nullptr; *text = nullptr;
	TxPlan p;
	auto t0 = clk::now();
	e.tx_s[0] = e.tx_s[1] = e.tx_s[2] = e.tx_s[3] = 0;
	if (tx_prepare(splice, who, what, n_ref, ref_lens, ref_at, n_reads, read_lens, read_at, n_regs, regs, read_of_reg, aln, cigar, TX_SLICE, p)) return -1;
	e.tx_s[1] = since(t0);
	t0 = clk::now();
	const size_t n_recs = p.recs.size(), n_sl = p.slices.size();
	int64_t *off = (int64_t*)malloc(((size_t)n_regs + 1) * sizeof(int64_t));
	if (!off) return fail(who + ": out of memory");
	struct Free { void *a = nullptr, *b = nullptr; ~Free() { free(a); free(b); } } guard;
	guard.a = off;
	std::vector<int64_t> dest(n_sl + 1, 0);
	if (n_sl > 0) {
		MM2GB_HIP(hipSetDevice(e.device));
		size_t tmp = 0;
		MM2GB_HIP(rocprim::exclusive_scan(nullptr, tmp, (int64_t*)nullptr, (int64_t*)nullptr, (int64_t)0, n_sl + 1, rocprim::plus<int64_t>(), e.stream));
		if (e.tx_recs.ensure(n_recs * sizeof(TxRec)) || e.tx_words.ensure(std::max<size_t>(p.words.size(), 1) * sizeof(TxWord)) || e.tx_slices.ensure(n_sl * sizeof(TxSlice)) ||
		    e.tx_cnt.ensure(n_sl * sizeof(TxCnt)) || e.tx_run.ensure(n_sl * 4) || e.tx_bytes.ensure((n_sl + 1) * 8) || e.tx_dest.ensure((n_sl + 1) * 8) || e.tx_tmp.ensure(std::max<size_t>(tmp, 16))) return -1;
		MM2GB_HIP(hipMemcpyAsync(e.tx_recs.ptr, p.recs.data(), n_recs * sizeof(TxRec), hipMemcpyHostToDevice, e.stream));
		if (!p.words.empty()) MM2GB_HIP(hipMemcpyAsync(e.tx_words.ptr, p.words.data(), p.words.size() * sizeof(TxWord), hipMemcpyHostToDevice, e.stream));
		MM2GB_HIP(hipMemcpyAsync(e.tx_slices.ptr, p.slices.data(), n_sl * sizeof(TxSlice), hipMemcpyHostToDevice, e.stream));
		const TxRec *d_recs = (const TxRec*)e.tx_recs.ptr; const TxSlice *d_sl = (const TxSlice*)e.tx_slices.ptr; const TxWord *d_words = (const TxWord*)e.tx_words.ptr;
		const uint8_t *d_refs = (const uint8_t*)e.al_refs.ptr, *d_reads = (const uint8_t*)e.al_reads.ptr;
		hipLaunchKernelGGL((p.introns ? k_tx_pass<false, true> : k_tx_pass<false, false>), dim3((unsigned)n_sl), dim3(TX_WG), 0, e.stream, p.mode, (int)n_sl, d_recs, d_sl, d_words, d_refs, d_reads, (TxCnt*)e.tx_cnt.ptr,
		                   (const int32_t*)nullptr, (const int64_t*)nullptr, (char*)nullptr);
		MM2GB_HIP(hipGetLastError());
		hipLaunchKernelGGL(k_tx_carry, dim3((unsigned)((n_recs + 63) / 64)), dim3(64), 0, e.stream, p.mode, (int)n_recs, (int)n_sl, d_recs, (const TxCnt*)e.tx_cnt.ptr, (int32_t*)e.tx_run.ptr,
		                   (int64_t*)e.tx_bytes.ptr);
		MM2GB_HIP(hipGetLastError());
		MM2GB_HIP(rocprim::exclusive_scan(e.tx_tmp.ptr, tmp, (int64_t*)e.tx_bytes.ptr, (int64_t*)e.tx_dest.ptr, (int64_t)0, n_sl + 1, rocprim::plus<int64_t>(), e.stream));
		MM2GB_HIP(hipMemcpyAsync(dest.data(), e.tx_dest.ptr, (n_sl + 1) * 8, hipMemcpyDeviceToHost, e.stream));
		MM2GB_HIP(hipStreamSynchronize(e.stream));
	}
	const int64_t total = dest[n_sl];
	char *buf = (char*)malloc((size_t)std::max<int64_t>(total, 1));
	if (!buf) return fail(who + ": out of memory");
	guard.b = buf;
	if (total > 0) {
		if (e.tx_text.ensure((size_t)total)) return -1;
		hipLaunchKernelGGL((p.introns ? k_tx_pass<true, true> : k_tx_pass<true, false>), dim3((unsigned)n_sl), dim3(TX_WG), 0, e.stream, p.mode, (int)n_sl, (const TxRec*)e.tx_recs.ptr, (const TxSlice*)e.tx_slices.ptr,
		                   (const TxWord*)e.tx_words.ptr, (const uint8_t*)e.al_refs.ptr, (const uint8_t*)e.al_reads.ptr, (TxCnt*)nullptr, (const int32_t*)e.tx_run.ptr,
		                   (const int64_t*)e.tx_dest.ptr, (char*)e.tx_text.ptr);
		MM2GB_HIP(hipGetLastError());
		MM2GB_HIP(hipStreamSynchronize(e.stream));
		e.tx_s[2] = since(t0);
		t0 = clk::now();
		MM2GB_HIP(hipMemcpy(buf, e.tx_text.ptr, (size_t)total, hipMemcpyDeviceToHost));
		e.tx_s[3] = since(t0);
	} else e.tx_s[2] = since(t0);
	size_t k = 0;
	for (int64_t i = 0; i < n_regs; ++i) {
		if (k < n_recs && p.reg_of[k] == i) { off[i] = dest[(size_t)p.recs[k].s_first]; ++k; }
		else off[i] = k < n_recs ? dest[(size_t)p.recs[k].s_first] : total;
	}
	off[n_regs] = total;
	guard.a = guard.b = nullptr;
	*text_off = off; *text = buf;
	return 0;
}

} // namespace mm2gb

using namespace mm2gb;

namespace {

int aln_text_gpu_any(bool splice, const char *who_, mm2gb_engine_t *eng, int what, int32_t n_ref, const char *const *ref_seqs, const int32_t *ref_lens, int64_t n_reads,
                     const char *const *read_seqs, const int32_t *read_lens, int64_t n_regs, const mm2gb_reg_t *regs, const int32_t *read_of_reg, const mm2gb_aln_t *aln,
                     const uint32_t *cigar, int64_t **text_off, char **text)
{
	const std::string who = who_;
	if (!eng) return fail("mm2gb: null engine");
	if (!text_off || !text || n_ref < 0 || n_reads < 0 || (n_ref > 0 && (!ref_seqs || !ref_lens)) || (n_reads > 0 && (!read_seqs || !read_lens))) return fail(who + ": null argument");
	*text_off = nullptr; *text = nullptr;
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
	const int rc = aln_text_resident(e, splice, who_, what, n_ref, ref_lens, ref_at.data(), n_reads, read_lens, read_at.data(), n_regs, regs, read_of_reg, aln, cigar, text_off, text);
	e.tx_s[0] = s_up;
	return rc;
}

} // namespace

int mm2gb_aln_text_gpu(mm2gb_engine_t *eng, int what, int32_t n_ref, const char *const *ref_seqs, const int32_t *ref_lens, int64_t n_reads, const char *const *read_seqs,
                       const int32_t *read_lens, int64_t n_regs, const mm2gb_reg_t *regs, const int32_t *read_of_reg, const mm2gb_aln_t *aln, const uint32_t *cigar,
                       int64_t **text_off, char **text)
{
	return aln_text_gpu_any(false, "mm2gb_aln_text_gpu", eng, what, n_ref, ref_seqs, ref_lens, n_reads, read_seqs, read_lens, n_regs, regs, read_of_reg, aln, cigar, text_off, text);
}

int mm2gb_aln_text_splice_gpu(mm2gb_engine_t *eng, int what, int32_t n_ref, const char *const *ref_seqs, const int32_t *ref_lens, int64_t n_reads, const char *const *read_seqs,
                              const int32_t *read_lens, int64_t n_regs, const mm2gb_reg_t *regs, const int32_t *read_of_reg, const mm2gb_aln_t *aln, const uint32_t *cigar,
                              int64_t **text_off, char **text)
{
	return aln_text_gpu_any(true, "mm2gb_aln_text_splice_gpu", eng, what, n_ref, ref_seqs, ref_lens, n_reads, read_seqs, read_lens, n_regs, regs, read_of_reg, aln, cigar, text_off, text);
}

int mm2gb_aln_text_gpu_info(mm2gb_engine_t *eng, int64_t *consts2, double *s4)
{
	if (!eng || !consts2) return fail("mm2gb_aln_text_gpu_info: null argument");
	consts2[0] = TX_SLICE; consts2[1] = TX_WG;
	if (s4) for (int i = 0; i < 4; ++i) s4[i] = eng->e.tx_s[i];
	return 0;
}
