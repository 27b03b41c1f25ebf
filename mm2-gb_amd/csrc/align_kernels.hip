// align_kernels.hip -- the device form of the alignment of hits (mm2gb_align_regs_gpu).  Planning, stitching and the per-read steps
// are align_host.cpp's; this unit is the DP backend of a round.  The batch's residues are uploaded once (one byte per base, the reads' forward
// strand only); per round k_al_gather writes every job's two stretches from them into the extension DP's input arenas (reverse complement and
// the left extension's reversal applied on the way), the DP runs on the resident bytes (ksw_run), k_al_zdrop walks the CIGAR of every
// first-pass gap fill where words and bytes lie, the host decides mm_test_zdrop's code from the 24 bytes per job that come back, and the
// fills that need it run again without the approximate maximum on the bytes already gathered.  The host never materialises a stretch.
// The short-read form's fills have no first-pass DP: k_al_ungapped scores the one-word alignment and walks it, a wave per fill.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "engine.h"
#include "align_host.h"
#include "host_chain.h"
#include "ksw_host.h"
#include "wave_scan.h"

namespace mm2gb {

constexpr int AL_SLICE = 4096;          // bytes of either stretch one workgroup of k_al_gather writes

struct AlDevJob { AlJob j; int64_t q_off, t_off; };
struct AlSlice { int32_t job, start; };

// one workgroup per slice of a job: bytes [start, start + AL_SLICE) of its query and of its target, a byte per thread and step (a wave's
// 64 stores are one contiguous line; the loads run forwards or backwards over one line too)
__global__ __launch_bounds__(256) void k_al_gather(const AlDevJob *__restrict__ jobs, const AlSlice *__restrict__ slices, int n_slices, const uint8_t *__restrict__ reads,
                                                   const uint8_t *__restrict__ refs, uint8_t *__restrict__ q, uint8_t *__restrict__ t)
{
	if ((int)blockIdx.x >= n_slices) return;
	const AlSlice s = slices[blockIdx.x];
	const AlDevJob d = jobs[s.job];
	const int qe = min(d.j.qlen, s.start + AL_SLICE), te = min(d.j.tlen, s.start + AL_SLICE);
	for (int k = s.start + (int)threadIdx.x; k < qe; k += 256) q[d.q_off + k] = al_query(reads, d.j, k);
	for (int k = s.start + (int)threadIdx.x; k < te; k += 256) t[d.t_off + k] = al_target(refs, d.j, k);
}

// mm_test_zdrop's walk (align_cell.h) for the gap fills of list[], one thread per job: a running maximum along a dependent walk, so what hides
// its latency is many walks at once; the list is ordered by length, neighbours walk about as far
__global__ __launch_bounds__(64) void k_al_zdrop(const AlDevJob *__restrict__ jobs, const int32_t *__restrict__ list, int n, const mm2gb_ksw_res_t *__restrict__ res,
                                                 const int64_t *__restrict__ off, const uint32_t *__restrict__ words, const uint8_t *__restrict__ q, const uint8_t *__restrict__ t,
                                                 int a, int b, int ambi, int gap_q, int gap_e, AlDrop *__restrict__ out)
{
	const int i = blockIdx.x * 64 + threadIdx.x;
	if (i >= n) return;
	const int job = list[i];
	const int64_t q_off = jobs[job].q_off, t_off = jobs[job].t_off;
	const uint32_t *w = words + off[job];
	out[i] = al_drop_walk(res[job].n_cigar, [&](int k) { return w[k]; }, [&](int k) { return (int)q[q_off + k]; }, [&](int k) { return (int)t[t_off + k]; }, a, b, ambi, gap_q, gap_e);
}

// Plain scans over a wave's lanes for k_al_ungapped's walk (wave_scan.h holds the skip-limited walks' scans): the sum and the 64-bit maximum over this lane and the lanes below it, and the
// 64-bit maximum and the sum over the whole wave in every lane.  By lane shuffles; every lane must be active.
__device__ __forceinline__ int al_wave_incl_sum(int v)
{
	for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(v, d, 64); if (scan_lane() >= d) v += o; }
	return v;
}
__device__ __forceinline__ long long al_wave_incl_max_i64(long long v)
{
	for (int d = 1; d < 64; d <<= 1) { const long long o = __shfl_up(v, d, 64); if (scan_lane() >= d && o > v) v = o; }
	return v;
}
__device__ __forceinline__ long long al_wave_max_i64(long long v)
{
	for (int d = 32; d > 0; d >>= 1) { const long long o = __shfl_xor(v, d, 64); if (o > v) v = o; }
	return v;
}
__device__ __forceinline__ int al_wave_sum(int v)
{
	for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
	return v;
}

// The short-read form's first pass over a fill (align.c:744-751) with mm_test_zdrop's walk over its one M word (align_cell.h: al_drop_walk), a wave per fill of
// list[], lanes taking the columns 64 at a time.  The fill's score (a / -b, + e2 at an ambiguous base) is a sum over the lanes.  The walk never leaves the diagonal,
// so its state is the prefix score under the real matrix, the running maximum with its column -- on score >= max the maximum moves forward (align.c:44), so the LAST
// column that holds it: the largest (score, column) pair at or below a lane -- and the largest drop max - score with its two ends, the first column that reaches it
// (strict >): the largest (drop, -column) pair.  Prefix score, maximum and largest drop are carried from one 64-column step to the next.
struct AlUngap { AlDrop d; int32_t score, pad_; };

__global__ __launch_bounds__(256) void k_al_ungapped(const AlDevJob *__restrict__ jobs, const int32_t *__restrict__ list, int n, const uint8_t *__restrict__ q, const uint8_t *__restrict__ t,
                                                    int a, int b, int ambi, int e2, AlUngap *__restrict__ out)
{
	const int fill = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = scan_lane();
	if (fill >= n) return;                      // (the whole wave)
	const AlDevJob d = jobs[list[fill]];
	const int len = d.j.qlen;
	const uint8_t *qq = q + d.q_off, *tt = t + d.t_off;
	constexpr long long NONE = INT64_MIN, STEP = 4294967296LL;
	int first_pass = 0, carry = 0, z_max = 0, z_from = -1, z_to = -1;
	long long best = NONE;                      // (the walk's max = INT32_MIN before the first column)
	for (int base = 0; base < len; base += 64) {
		const int k = base + lane;
		const bool on = k < len;
		int s = 0;
		if (on) { const int cq = qq[k], ct = tt[k]; first_pass += al_ungapped_score(a, b, e2, ct, cq); s = al_score(a, b, ambi, ct, cq); }
		const int score = carry + al_wave_incl_sum(s);
		long long top = on ? (long long)score * STEP + k : NONE;
		top = al_wave_incl_max_i64(top);
		if (best > top) top = best;
		const int from = (int)(top & 0xffffffffLL), z = on ? (int)(top >> 32) - score : -1;          // z == 0: this column is the maximum
		const long long deepest = al_wave_max_i64(on ? (long long)z * STEP + (0x7fffffff - k) : NONE);
		if ((int)(deepest >> 32) > z_max) {     // (the same in every lane)
			z_max = (int)(deepest >> 32);
			z_to = 0x7fffffff - (int)(deepest & 0xffffffffLL);
			z_from = __shfl(from, z_to - base, 64);
		}
		carry = __shfl(score, 63, 64); best = __shfl(top, 63, 64);
	}
	first_pass = al_wave_sum(first_pass);
	if (lane == 0) {
		AlUngap r;
		r.d.max_zdrop = z_max; r.d.t_from = r.d.q_from = z_from; r.d.t_to = r.d.q_to = z_to; r.d.pad_ = 0;
		r.score = first_pass; r.pad_ = 0;
		out[fill] = r;
	}
}

namespace {

using clk = std::chrono::steady_clock;
inline double since(clk::time_point t0) { return std::chrono::duration<double>(clk::now() - t0).count(); }

struct DevBackend : AlBackend {
	Engine &e;
	bool uploaded = false;
	explicit DevBackend(Engine &eng) : e(eng) {}

	int upload(const AlCtx &c)
	{
		const auto t0 = clk::now();
		MM2GB_HIP(hipSetDevice(e.device));
		if (e.al_refs.ensure(std::max<size_t>(c.refs.size(), 16)) || e.al_reads.ensure(std::max<size_t>(c.reads.size(), 16))) return -1;
		if (!c.refs.empty()) MM2GB_HIP(hipMemcpyAsync(e.al_refs.ptr, c.refs.data(), c.refs.size(), hipMemcpyHostToDevice, e.stream));
		if (!c.reads.empty()) MM2GB_HIP(hipMemcpyAsync(e.al_reads.ptr, c.reads.data(), c.reads.size(), hipMemcpyHostToDevice, e.stream));
		MM2GB_HIP(hipStreamSynchronize(e.stream));
		e.al_resident[0] = (int64_t)c.refs.size(); e.al_resident[1] = (int64_t)c.reads.size();
		uploaded = true;
		seconds[0] += since(t0);
		return 0;
	}

	int run(const AlCtx &c, std::vector<AlRun> &runs, std::vector<uint32_t> &pool) override
	{
		if (!uploaded && upload(c)) return -1;
		const size_t n = runs.size();
		if (n >= ((size_t)1 << 31)) return fail("mm2gb_align_regs: a round is limited to 2^31 jobs");
		// where every job's bytes go, and the slices that write them; a stretch over max_sw_mat is neither gathered nor run
		auto t0 = clk::now();
		std::vector<AlDevJob> dev(n);
		std::vector<mm2gb_ksw_job_t> kj(n);
		std::vector<AlSlice> slices;
		std::vector<char> big(n, 0);
		int64_t q_total = 0, t_total = 0;
		for (size_t k = 0; k < n; ++k) {
			AlRun &x = runs[k];
			x.code = 0;
			big[k] = al_too_big(c, x.j);
			dev[k].j = x.j;
			if ((big[k] && !x.ungapped) || dev[k].j.qlen < 0 || dev[k].j.tlen < 0) dev[k].j.qlen = dev[k].j.tlen = 0;      // (an ungapped first pass is no DP: no size limit, align.c:744)
			if (dev[k].j.qlen == 0 || dev[k].j.tlen == 0) dev[k].j.qlen = dev[k].j.tlen = 0;            // the DP returns at once: nothing to gather
			const bool twin = x.twin > 0 && (size_t)x.twin <= k;          // a chain's second trial: the first one's bytes, nothing gathered
			if (twin) { dev[k].q_off = dev[k - (size_t)x.twin].q_off; dev[k].t_off = dev[k - (size_t)x.twin].t_off; }
			else { dev[k].q_off = q_total; dev[k].t_off = t_total; q_total += (dev[k].j.qlen + 15) / 16 * 16; t_total += (dev[k].j.tlen + 15) / 16 * 16; }
			kj[k] = { dev[k].q_off, dev[k].t_off, dev[k].j.qlen, dev[k].j.tlen, x.w, x.zdrop, x.end_bonus, x.flag };
			for (int s = 0; !twin && s < std::max(dev[k].j.qlen, dev[k].j.tlen); s += AL_SLICE) slices.push_back({ (int32_t)k, s });
		}
		MM2GB_HIP(hipSetDevice(e.device));
		MM2GB_HIP(hipStreamSynchronize(e.stream));
		if (e.kw_q.ensure((size_t)std::max<int64_t>(q_total, 16)) || e.kw_t.ensure((size_t)std::max<int64_t>(t_total, 16)) || e.al_jobs.ensure(n * sizeof(AlDevJob)) ||
		    e.al_slices.ensure(std::max<size_t>(slices.size(), 1) * sizeof(AlSlice))) return -1;
		MM2GB_HIP(hipMemcpyAsync(e.al_jobs.ptr, dev.data(), n * sizeof(AlDevJob), hipMemcpyHostToDevice, e.stream));
		if (!slices.empty()) {
			MM2GB_HIP(hipMemcpyAsync(e.al_slices.ptr, slices.data(), slices.size() * sizeof(AlSlice), hipMemcpyHostToDevice, e.stream));
			hipLaunchKernelGGL(k_al_gather, dim3((unsigned)slices.size()), dim3(256), 0, e.stream, (const AlDevJob*)e.al_jobs.ptr, (const AlSlice*)e.al_slices.ptr, (int)slices.size(),
			                   (const uint8_t*)e.al_reads.ptr, (const uint8_t*)e.al_refs.ptr, (uint8_t*)e.kw_q.ptr, (uint8_t*)e.kw_t.ptr);
			MM2GB_HIP(hipGetLastError());
		}
		MM2GB_HIP(hipStreamSynchronize(e.stream));
		seconds[2] += since(t0);
		// first pass: every job but the short-read form's fills, which have none that is a DP
		t0 = clk::now();
		std::vector<int32_t> ung;               // the ungapped fills
		for (size_t k = 0; k < n; ++k) if (runs[k].ungapped) ung.push_back((int32_t)k);
		std::vector<mm2gb_ksw_res_t> res(n);
		uint32_t *cig1 = nullptr, *cig2 = nullptr;
		int64_t total1 = 0, total2 = 0;
		struct Free { uint32_t **a, **b; ~Free() { free(*a); free(*b); } } guard{ &cig1, &cig2 };
		if (ung.empty()) {
			if (ksw_run(e, c.kc, (int64_t)n, kj.data(), nullptr, nullptr, nullptr, true, res.data(), &cig1, &total1)) return -1;
		} else {
			std::vector<mm2gb_ksw_job_t> kj1;
			std::vector<int32_t> at1;
			for (size_t k = 0; k < n; ++k) {
				if (runs[k].ungapped) continue;
				if (runs[k].j.kind == 1) return fail("mm2gb_align_regs: a round mixes ungapped fills with first-pass DP fills");      // (k_al_zdrop indexes records and jobs alike)
				kj1.push_back(kj[k]); at1.push_back((int32_t)k);
			}
			std::vector<mm2gb_ksw_res_t> res1(kj1.size());
			if (!kj1.empty() && ksw_run(e, c.kc, (int64_t)kj1.size(), kj1.data(), nullptr, nullptr, nullptr, true, res1.data(), &cig1, &total1)) return -1;
			for (size_t i = 0; i < at1.size(); ++i) res[(size_t)at1[i]] = res1[i];
		}
		seconds[3] += since(t0);
		// mm_test_zdrop for the gap fills
		t0 = clk::now();
		std::vector<int32_t> list;
		for (size_t k = 0; k < n; ++k) if (runs[k].j.kind == 1 && !big[k] && !runs[k].ungapped) list.push_back((int32_t)k);
		std::stable_sort(list.begin(), list.end(), [&](int32_t a, int32_t b) { return kj[(size_t)a].qlen + kj[(size_t)a].tlen > kj[(size_t)b].qlen + kj[(size_t)b].tlen; });
		std::vector<AlDrop> drop(list.size());
		for (AlDrop &d : drop) { d.max_zdrop = 0; d.t_from = d.t_to = d.q_from = d.q_to = -1; d.pad_ = 0; }
		if (!list.empty() && total1 > 0) {          // without words no pack ran and kw_off is not set: every walk is the empty one
			if (e.al_list.ensure(list.size() * 4) || e.al_drop.ensure(list.size() * sizeof(AlDrop))) return -1;
			MM2GB_HIP(hipMemcpyAsync(e.al_list.ptr, list.data(), list.size() * 4, hipMemcpyHostToDevice, e.stream));
			hipLaunchKernelGGL(k_al_zdrop, dim3((unsigned)((list.size() + 63) / 64)), dim3(64), 0, e.stream, (const AlDevJob*)e.al_jobs.ptr, (const int32_t*)e.al_list.ptr, (int)list.size(),
			                   (const mm2gb_ksw_res_t*)e.kw_res.ptr, (const int64_t*)e.kw_off.ptr, (const uint32_t*)e.kw_pack.ptr, (const uint8_t*)e.kw_q.ptr, (const uint8_t*)e.kw_t.ptr,
			                   c.a, c.b, c.ambi, (int)c.opt.q, (int)c.opt.e, (AlDrop*)e.al_drop.ptr);
			MM2GB_HIP(hipGetLastError());
			MM2GB_HIP(hipMemcpyAsync(drop.data(), e.al_drop.ptr, list.size() * sizeof(AlDrop), hipMemcpyDeviceToHost, e.stream));
			MM2GB_HIP(hipStreamSynchronize(e.stream));
		}
		std::vector<int32_t> again;
		for (size_t i = 0; i < list.size(); ++i) {
			AlRun &x = runs[(size_t)list[i]];
			x.code = al_zdrop_code(c, x.j, drop[i]);
			if (x.code) again.push_back(list[i]);
		}
		// the ungapped fills: score and walk in one kernel; the record is made here, and the ones that drop go on to the second pass (one over max_sw_mat is not run)
		std::vector<AlUngap> first(ung.size());
		if (!ung.empty()) {
			if (e.al_list.ensure(ung.size() * 4) || e.al_drop.ensure(ung.size() * sizeof(AlUngap))) return -1;
			MM2GB_HIP(hipMemcpyAsync(e.al_list.ptr, ung.data(), ung.size() * 4, hipMemcpyHostToDevice, e.stream));
			hipLaunchKernelGGL(k_al_ungapped, dim3((unsigned)((ung.size() + 3) / 4)), dim3(256), 0, e.stream, (const AlDevJob*)e.al_jobs.ptr, (const int32_t*)e.al_list.ptr, (int)ung.size(),
			                   (const uint8_t*)e.kw_q.ptr, (const uint8_t*)e.kw_t.ptr, (int)c.opt.a, (int)c.opt.b, c.ambi, (int)c.opt.e2, (AlUngap*)e.al_drop.ptr);
			MM2GB_HIP(hipGetLastError());
			MM2GB_HIP(hipMemcpyAsync(first.data(), e.al_drop.ptr, ung.size() * sizeof(AlUngap), hipMemcpyDeviceToHost, e.stream));
			MM2GB_HIP(hipStreamSynchronize(e.stream));
		}
		KswEz reset;
		ksw_ez_reset(reset);
		for (size_t i = 0; i < ung.size(); ++i) {
			const size_t k = (size_t)ung[i];
			AlRun &x = runs[k];
			x.code = al_zdrop_code(c, x.j, first[i].d);
			if (!x.code) { KswEz z = reset; z.score = first[i].score; ksw_store(z, 1, &res[k]); }
			else if (big[k]) ksw_store(reset, 0, &res[k]);
			else again.push_back((int32_t)k);
		}
		seconds[4] += since(t0);
		// second pass on the bytes already gathered
		t0 = clk::now();
		std::vector<mm2gb_ksw_res_t> res2(again.size());
		if (!again.empty()) {
			std::vector<mm2gb_ksw_job_t> kj2(again.size());
			for (size_t i = 0; i < again.size(); ++i) {
				const AlRun &x = runs[(size_t)again[i]];
				kj2[i] = kj[(size_t)again[i]];
				kj2[i].flag = al_second_flag(x.flag); kj2[i].zdrop = al_second_zdrop(c, x.code);
			}
			if (ksw_run(e, c.kc, (int64_t)again.size(), kj2.data(), nullptr, nullptr, nullptr, true, res2.data(), &cig2, &total2)) return -1;
		}
		seconds[5] += since(t0);
		// the round's records and words
		t0 = clk::now();
		std::vector<int32_t> second(n, -1);
		for (size_t i = 0; i < again.size(); ++i) second[(size_t)again[i]] = (int32_t)i;
		pool.clear();
		pool.reserve((size_t)(total1 + total2));
		for (size_t k = 0; k < n; ++k) {
			const bool two = second[k] >= 0;
			const mm2gb_ksw_res_t &r = two ? res2[(size_t)second[k]] : res[k];
			const uint32_t *w = two ? cig2 : cig1;
			runs[k].res = r;
			runs[k].res.cigar_off = (int64_t)pool.size();
			if (runs[k].ungapped && !two) {       // the first pass's one M word, or nothing for a fill over max_sw_mat that dropped
				if (r.n_cigar > 0) pool.push_back((uint32_t)std::max(kj[k].qlen, 0) << 4);
				if (runs[k].code) runs[k].res.zdropped = 1;
				continue;
			}
			if (r.n_cigar > 0) pool.insert(pool.end(), w + r.cigar_off, w + r.cigar_off + r.n_cigar);
			if (big[k]) runs[k].res.zdropped = 1;
		}
		seconds[6] += since(t0);
		return 0;
	}
};

} // namespace

} // namespace mm2gb

using namespace mm2gb;

int mm2gb_align_regs_gpu(mm2gb_engine_t *eng, const mm2gb_align_opt_t *opt, int k, int idx_flag, int32_t n_ref, const char *const *ref_seqs, const int32_t *ref_lens,
                         int64_t n_reads, const char *const *read_seqs, const int32_t *read_lens, const int64_t *reg_off, const mm2gb_reg_t *regs,
                         const int64_t *anchor_off, const mm2gb_anchor_t *anchors, mm2gb_align_out_t *out)
{
	if (!eng) { if (out) memset(out, 0, sizeof *out); return fail("mm2gb: null engine"); }
	eng->e.al_resident[0] = eng->e.al_resident[1] = -1;          // until this call's backend has uploaded its batch
	DevBackend be(eng->e);
	return al_align_regs("mm2gb_align_regs_gpu", opt, nullptr, k, idx_flag, n_ref, ref_seqs, ref_lens, n_reads, read_seqs, read_lens, reg_off, regs, anchor_off, anchors,
	                     std::min(usable_cpus(), 16), &be, out, nullptr);
}

// MM_F_SR: the same backend; a fill marked ungapped goes through k_al_ungapped instead of a first-pass DP
int mm2gb_align_regs_sr_gpu(mm2gb_engine_t *eng, const mm2gb_align_opt_t *opt, int k, int idx_flag, int32_t n_ref, const char *const *ref_seqs, const int32_t *ref_lens,
                            int64_t n_reads, const char *const *read_seqs, const int32_t *read_lens, const int64_t *reg_off, const mm2gb_reg_t *regs,
                            const int64_t *anchor_off, const mm2gb_anchor_t *anchors, mm2gb_align_out_t *out, int64_t *sr_counts)
{
	if (!eng) { if (out) memset(out, 0, sizeof *out); return fail("mm2gb: null engine"); }
	eng->e.al_resident[0] = eng->e.al_resident[1] = -1;
	DevBackend be(eng->e);
	return al_align_regs("mm2gb_align_regs_sr_gpu", opt, nullptr, k, idx_flag, n_ref, ref_seqs, ref_lens, n_reads, read_seqs, read_lens, reg_off, regs, anchor_off, anchors,
	                     std::min(usable_cpus(), 16), &be, out, nullptr, false, sr_counts, true);
}

// q == q2 && e == e2: the same backend; the context's constants select the single-affine fill
int mm2gb_align_regs_extz_gpu(mm2gb_engine_t *eng, const mm2gb_align_opt_t *opt, int k, int idx_flag, int32_t n_ref, const char *const *ref_seqs, const int32_t *ref_lens,
                              int64_t n_reads, const char *const *read_seqs, const int32_t *read_lens, const int64_t *reg_off, const mm2gb_reg_t *regs,
                              const int64_t *anchor_off, const mm2gb_anchor_t *anchors, mm2gb_align_out_t *out)
{
	if (!eng) { if (out) memset(out, 0, sizeof *out); return fail("mm2gb: null engine"); }
	eng->e.al_resident[0] = eng->e.al_resident[1] = -1;
	DevBackend be(eng->e);
	return al_align_regs("mm2gb_align_regs_extz_gpu", opt, nullptr, k, idx_flag, n_ref, ref_seqs, ref_lens, n_reads, read_seqs, read_lens, reg_off, regs, anchor_off, anchors,
	                     std::min(usable_cpus(), 16), &be, out, nullptr, true);
}

// the spliced form: the same backend; the context's constants select the splice-aware fill, a job's flag word carries its trial's
// strand bits, and a second trial names the first as its twin
int mm2gb_align_regs_splice_gpu(mm2gb_engine_t *eng, const mm2gb_align_splice_opt_t *opt, int k, int idx_flag, int32_t n_ref, const char *const *ref_seqs,
                                const int32_t *ref_lens, int64_t n_reads, const char *const *read_seqs, const int32_t *read_lens, const int64_t *reg_off,
                                const mm2gb_reg_t *regs, const int64_t *anchor_off, const mm2gb_anchor_t *anchors, mm2gb_align_out_t *out, int64_t *splice_counts)
{
	if (!eng || !opt) { if (out) memset(out, 0, sizeof *out); return fail(!eng ? "mm2gb: null engine" : "mm2gb_align_regs_splice_gpu: null argument"); }
	eng->e.al_resident[0] = eng->e.al_resident[1] = -1;
	DevBackend be(eng->e);
	return al_align_regs("mm2gb_align_regs_splice_gpu", &opt->base, opt, k, idx_flag, n_ref, ref_seqs, ref_lens, n_reads, read_seqs, read_lens, reg_off, regs, anchor_off, anchors,
	                     std::min(usable_cpus(), 16), &be, out, splice_counts);
}
