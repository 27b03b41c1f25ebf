// ksw_kernels.hip -- the dual-affine extension DP on the device (mm2gb_ksw_extd2_gpu), the splice-aware one
// (mm2gb_ksw_exts2_gpu) and the single-affine one (mm2gb_ksw_extz2_gpu), which have the same shape: one fill kernel
// in three forms (k_ksw's FORM), one planner, one walk, one pack.
// One workgroup per job, taken from a cost-ordered list.  The anti-diagonals are walked in order; the cells of a diagonal's band (rounded out
// to groups of 16, as the definition in ksw_host.cpp has them) are dealt to the workgroup's threads by position: cell t belongs to thread
// t mod NT for the whole job, so every array a cell reads only from itself (u, y, y2, the score byte, H) needs no barrier, and the three it
// reads from its left neighbour (v, x, x2) are kept twice, diagonal r reading one copy and writing the other: one barrier per diagonal
// with the approximate maximum, two with the exact one (its reduction).  The state image lives in LDS when it fits, else in global memory.
// Direction bytes go to a per-job slab, one row per diagonal; k_ksw_walk walks back over them, one thread per job, and k_ksw_pack lays the
// batch's CIGAR words out in job order.  The arithmetic is ksw_cell.h's.
#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>
#include "engine.h"
#include "ksw_cell.h"
#include "ksw_host.h"

namespace mm2gb {

// threads of a workgroup by the width of a job's rows of direction bytes (its band rounded out, at most): up to KSW_BAND[0] cells a wave,
// up to KSW_BAND[1] four waves, beyond that eight, each thread then taking every KSW_NT[2]-th cell
constexpr int KSW_NT[3] = { 64, 256, 512 };
constexpr int KSW_BAND[2] = { 64, 256 };
// dynamic LDS a launch may ask for (the kernel's own static LDS stays below 1 KiB), and the sizes launches are made at
constexpr int KSW_LDS_MAX = 160 * 1024 - 1024;
constexpr int KSW_LDS_STEP[4] = { 8 * 1024, 32 * 1024, 64 * 1024, KSW_LDS_MAX };

struct KswDevJob { int64_t q_off, t_off, slab_off, cig_off; int32_t qlen, tlen, w, zdrop, end_bonus, flag, idx, ncol; };

// bytes of a job's state image: H when the exact maximum is wanted, u v x x2 twice, y, y2 (the splice-aware form: donor and acceptor) and
// the score bytes, target and query.  The single-affine form has neither x2 nor y2: 8 bytes a position where the dual-affine form has 11.
inline int64_t ksw_image_bytes(int form, int qlen, int tlen, int flag)
{
	const int64_t T = ksw_round16(tlen);
	return ((flag & MM2GB_KSW_APPROX_MAX) ? 0 : 4 * T) + (form == KSW_SPLICE ? 12 : form == KSW_SINGLE ? 8 : 11) * T + T + ksw_round16(qlen);
}

// The fill.  SPLICE: the splice-aware DP, the same walk over the anti-diagonals with ksw_cell_splice as the cell and donor[] / acceptor[] where
// y2 is.  It has no band (job.w is the longer side, so ksw_band binds nowhere and no row is empty: that exit is left out), a row is at most
// min(qlen, tlen) cells wide, and the image is proportional to the TARGET: a read's stretch across an intron of tens of kilobases has a
// narrow row over a long image, which then lives in global memory.  donor[] / acceptor[] are filled from the staged target, every thread
// the positions it owns, so the barrier after staging is the only one they need.  junc: their annotation bytes, or null (SPLICE only).
// SINGLE: the single-affine DP, ksw_cell_single as the cell over u, v, x (twice each), y and the score bytes alone, all zero at the start
// (its c.ini); a row's first v1 reaches three cells further (ksw_smear), and H takes its differences through ksw_diff.
template <int NT, bool IN_LDS, int FORM>
__global__ __launch_bounds__(NT) void k_ksw(const KswConst c, const KswDevJob *__restrict__ jobs, int lo, int hi, int *counter,
                                            const uint8_t *__restrict__ queries, const uint8_t *__restrict__ targets, const uint8_t *__restrict__ junc, uint8_t *slab,
                                            uint8_t *gimg, int64_t gimg_stride, mm2gb_ksw_res_t *res)
{
	extern __shared__ __align__(16) uint8_t smem[];
	__shared__ uint64_t part[2][NT / 64];
	__shared__ int s_job;
	__shared__ int8_t s_mat[25];
	constexpr bool SPLICE = FORM == KSW_SPLICE, SINGLE = FORM == KSW_SINGLE;
	const int tid = threadIdx.x;
	if (tid < 25) s_mat[tid] = c.mat[tid];                  // visible after the loop's first barrier
	uint8_t *img;
	if constexpr (IN_LDS) img = smem; else img = gimg + (int64_t)blockIdx.x * gimg_stride;
	for (;;) {
		__syncthreads();                                    // the last job's image and s_job are done with
		if (tid == 0) s_job = lo + atomicAdd(counter, 1);
		__syncthreads();
		if (s_job >= hi) break;
		const KswDevJob job = jobs[s_job];
		const int qlen = job.qlen, tlen = job.tlen, flag = job.flag, w = job.w, ncol = job.ncol, T = ksw_round16(tlen);
		const bool with_cigar = !(flag & MM2GB_KSW_SCORE_ONLY), approx = (flag & MM2GB_KSW_APPROX_MAX) != 0, right = (flag & MM2GB_KSW_RIGHT) != 0, generic = (flag & MM2GB_KSW_GENERIC_SC) != 0;
		int32_t *H = (int32_t*)img;
		int8_t *u = (int8_t*)img + (approx ? 0 : 4 * T), *v = u + 2 * T, *x = v + 2 * T, *x2 = x + (SINGLE ? 0 : 2 * T), *y = x2 + 2 * T;
		int8_t *y2 = y + T, *don = y + T, *acc = don + T, *s = SINGLE ? y + T : (SPLICE ? acc : y2) + T;      // y2, or donor and acceptor, or neither
		uint8_t *tg = (uint8_t*)(s + T), *qy = tg + T;
		for (int t = tid; t < T; t += NT) {
			u[t] = u[T + t] = v[t] = v[T + t] = x[t] = x[T + t] = y[t] = c.ini;
			if constexpr (SPLICE) x2[t] = x2[T + t] = c.ini2; else if constexpr (!SINGLE) x2[t] = x2[T + t] = y2[t] = c.ini2;
			s[t] = 0;
			if (!approx) H[t] = MM2GB_KSW_NEG_INF;
			if (t < tlen) tg[t] = targets[job.t_off + t];
		}
		for (int t = tid; t < qlen; t += NT) qy[t] = queries[job.q_off + t];
		__syncthreads();
		if constexpr (SPLICE) {
			const uint8_t *jn = junc ? junc + job.t_off : nullptr;
			for (int t = tid; t < T; t += NT) {
				int8_t d, a;
				ksw_splice_sites(c, flag, [&](int i) { return tg[i]; }, jn, tlen, t, &d, &a);
				don[t] = d; acc[t] = a;
			}
		}
		uint8_t *p = slab + job.slab_off;
		KswEz z;
		ksw_ez_reset(z);
		int32_t H0 = 0; int H0_t = 0, last_st = -1, last_en = -1;
		for (int r = 0; r < qlen + tlen - 1; ++r) {
			int st0, en0;
			ksw_band(r, qlen, tlen, w, &st0, &en0);
			if constexpr (!SPLICE) if (st0 > en0) { z.zdropped = 1; break; }      // without a band no row is empty
			const int st = st0 / 16 * 16, en = (en0 + 16) / 16 * 16 - 1, cur = (r & 1) * T, nxt = T - cur;
			int8_t bx1 = c.ini, bx21 = c.ini2, bv1 = c.ini;
			if (st > 0) { if (st - 1 >= last_st && st - 1 <= last_en) { bx1 = x[cur + st - 1]; if constexpr (!SINGLE) bx21 = x2[cur + st - 1]; bv1 = v[cur + st - 1]; } }
			else bv1 = ksw_edge<FORM>(c, r);
			if (en >= r && (r & (NT - 1)) == tid) { y[r] = c.ini; if constexpr (FORM == KSW_DUAL) y2[r] = c.ini2; u[cur + r] = ksw_edge<FORM>(c, r); }
			const int s_end = generic ? en0 + 1 : min(T, st0 + ((en0 - st0) / 16 + 1) * 16);
			for (int t = st0 + ((tid - st0) & (NT - 1)); t < s_end; t += NT)
				s[t] = ksw_score(c, s_mat, generic, ksw_target_byte((const uint8_t*)tg, (const uint8_t*)qy, qlen, tlen, T, t), ksw_query_byte((const uint8_t*)qy, qlen, r, t));
			uint8_t *pr = p + (int64_t)r * ncol - st;
			for (int t = st + ((tid - st) & (NT - 1)); t <= en; t += NT) {
				const bool first = t == st;
				KswCell o;
				if constexpr (SINGLE) {
					const int8_t x1 = first ? bx1 : x[cur + t - 1], v1 = first ? bv1 : ksw_smear(bv1, t - st, v[cur + t - 1]);
					o = ksw_cell_single(c, right, s[t], x1, v1, u[cur + t], y[t]);
				} else {
					const int8_t x1 = first ? bx1 : x[cur + t - 1], v1 = first ? bv1 : v[cur + t - 1], x21 = first ? bx21 : x2[cur + t - 1];
					if constexpr (SPLICE) o = ksw_cell_splice(c, right, s[t], x1, v1, x21, u[cur + t], y[t], don[t], acc[t]);
					else o = ksw_cell(c, right, s[t], x1, v1, x21, u[cur + t], y[t], y2[t]);
				}
				u[nxt + t] = o.u; v[nxt + t] = o.v; x[nxt + t] = o.x; y[t] = o.y;
				if constexpr (!SINGLE) x2[nxt + t] = o.x2;
				if constexpr (FORM == KSW_DUAL) y2[t] = o.y2;
				if (with_cigar && t - st < ncol) pr[t] = o.d;
			}
			bool stop;
			if (!approx) {
				int32_t Hl = 0;
				if (r > 0 && en0 > 0 && (en0 & (NT - 1)) == tid) Hl = H[en0 - 1];      // before its owner moves it on
				__syncthreads();
				uint64_t key = 0;
				for (int t = st0 + ((tid - st0) & (NT - 1)); t <= en0; t += NT) {
					int32_t h;
					if (t == en0) h = r == 0 ? ksw_diff<FORM>(c, v[nxt]) - c.qe0 : en0 > 0 ? Hl + ksw_diff<FORM>(c, u[nxt + en0]) : H[en0] + ksw_diff<FORM>(c, v[nxt + en0]);
					else h = H[t] + ksw_diff<FORM>(c, v[nxt + t]);
					H[t] = h;
					const uint64_t k = ksw_max_key(h, t, st0, en0);
					key = k > key ? k : key;
				}
				for (int d = 32; d; d >>= 1) { const uint64_t o = __shfl_xor((unsigned long long)key, d, 64); key = o > key ? o : key; }
				if ((tid & 63) == 0) part[r & 1][tid >> 6] = key;
				__syncthreads();
				key = part[r & 1][0];
				for (int k = 1; k < NT / 64; ++k) key = part[r & 1][k] > key ? part[r & 1][k] : key;
				stop = ksw_row_exact(z, c, qlen, tlen, job.zdrop, r, st0, en0, en, ksw_key_H(key), ksw_key_t(key, st0, en0), H[en0], H[st0]);
			} else {
				__syncthreads();
				stop = ksw_row_approx<FORM>(z, c, qlen, tlen, job.zdrop, flag, r, st0, en0, H0, H0_t, [=](int t) { return ksw_diff<FORM>(c, v[nxt + t]); }, [=](int t) { return ksw_diff<FORM>(c, u[nxt + t]); });
			}
			if (stop) break;
			last_st = st; last_en = en;
		}
		// the record, and where the walk back starts (k_ksw_walk takes it from pad_ / cigar_off and clears them)
		int i0 = 0, j0 = 0;
		const bool walk = ksw_walk_from(z, SPLICE, qlen, tlen, job.end_bonus, flag, &i0, &j0);
		if (tid == 0) {
			mm2gb_ksw_res_t o;
			ksw_store(z, 0, &o);
			o.pad_ = walk; o.cigar_off = walk ? (int64_t)i0 << 32 | (uint32_t)j0 : 0;
			res[job.idx] = o;
		}
	}
}

// The walk back over a job's direction bytes, one thread per job: a walk is a chain of dependent loads, so what hides its latency is
// many walks at once.  Neighbours in the cost-ordered list walk about as far.  Words are left last operation first.
__global__ __launch_bounds__(64) void k_ksw_walk(const KswDevJob *__restrict__ jobs, int lo, int hi, int min_intron, const uint8_t *__restrict__ slab, uint32_t *cig_all, mm2gb_ksw_res_t *res)
{
	const int k = lo + blockIdx.x * 64 + threadIdx.x;
	if (k >= hi) return;
	const KswDevJob job = jobs[k];
	mm2gb_ksw_res_t *o = res + job.idx;
	if (!o->pad_) return;
	const int i0 = (int)(o->cigar_off >> 32), j0 = (int)(uint32_t)o->cigar_off;
	const uint8_t *p = slab + job.slab_off;
	uint32_t *cig = cig_all + job.cig_off;
	o->n_cigar = ksw_walk(job.qlen, job.tlen, job.w, min_intron, i0, j0, [&](int r, int col) { return (uint32_t)p[(int64_t)r * job.ncol + col]; }, [&](int n, uint32_t word) { cig[n] = word; });
	o->pad_ = 0; o->cigar_off = 0;
}

// every job's words from where its walk left them to where the batch's array wants them, first operation first unless REV_CIGAR is set
__global__ __launch_bounds__(64) void k_ksw_pack(const KswDevJob *__restrict__ jobs, int n_live, const mm2gb_ksw_res_t *__restrict__ res, const int64_t *__restrict__ off,
                                                 const uint32_t *__restrict__ cig_all, uint32_t *__restrict__ out)
{
	for (int j = blockIdx.x; j < n_live; j += gridDim.x) {
		const KswDevJob job = jobs[j];
		const int n = res[job.idx].n_cigar;
		const bool keep = (job.flag & MM2GB_KSW_REV_CIGAR) != 0;
		for (int k = threadIdx.x; k < n; k += 64) out[off[job.idx] + k] = cig_all[job.cig_off + (keep ? k : n - 1 - k)];
	}
}

namespace {

struct Launch { int lo, hi, nt_class, lds_class; int64_t lds, slab, img; };

// direction bytes one launch may hold (MM2GB_KSW_SLAB_MB, read at every call; 4 GiB): a batch that needs more runs as several launches
int64_t slab_budget()
{
	const char *e = getenv("MM2GB_KSW_SLAB_MB");
	const long long mb = e ? atoll(e) : 0;
	return (int64_t)(mb > 0 ? mb : 4096) << 20;
}

using Fill = void (*)(KswConst, const KswDevJob*, int, int, int*, const uint8_t*, const uint8_t*, const uint8_t*, uint8_t*, uint8_t*, int64_t, mm2gb_ksw_res_t*);
template <bool IN_LDS, int FORM>
constexpr Fill FILL[3] = { k_ksw<KSW_NT[0], IN_LDS, FORM>, k_ksw<KSW_NT[1], IN_LDS, FORM>, k_ksw<KSW_NT[2], IN_LDS, FORM> };
template <bool IN_LDS>
inline Fill fill_of(int form, int nt_class) { return (form == KSW_SPLICE ? FILL<IN_LDS, KSW_SPLICE> : form == KSW_SINGLE ? FILL<IN_LDS, KSW_SINGLE> : FILL<IN_LDS, KSW_DUAL>)[nt_class]; }

// launch k of a call: the fill for its classes and c.form (junc: its annotation bytes are in kw_junc)
int launch_one(Engine &e, const KswConst &c, bool junc, const Launch &L, int k, int grid)
{
	const bool in_lds = L.lds_class < 4;
	const Fill fill = in_lds ? fill_of<true>(c.form, L.nt_class) : fill_of<false>(c.form, L.nt_class);
	if (in_lds) MM2GB_HIP(hipFuncSetAttribute((const void*)fill, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.lds));
	hipLaunchKernelGGL(fill, dim3(grid), dim3(KSW_NT[L.nt_class]), in_lds ? (size_t)L.lds : 0, e.stream, c, (const KswDevJob*)e.kw_jobs.ptr, L.lo, L.hi, (int*)e.kw_cnt.ptr + k,
	                   (const uint8_t*)e.kw_q.ptr, (const uint8_t*)e.kw_t.ptr, junc ? (const uint8_t*)e.kw_junc.ptr : nullptr, (uint8_t*)e.kw_slab.ptr, (uint8_t*)e.kw_img.ptr, L.img,
	                   (mm2gb_ksw_res_t*)e.kw_res.ptr);
	MM2GB_HIP(hipGetLastError());
	return 0;
}

} // namespace

// The planning and the launches behind mm2gb_ksw_extd2_gpu and, by c.form, mm2gb_ksw_exts2_gpu (with junc, indexed like targets, or null) and mm2gb_ksw_extz2_gpu.  resident: the jobs' sequences already lie in kw_q / kw_t at their q_off / t_off
// (the alignment call's gather kernel put them there, align_kernels.hip) and nothing is uploaded.  Either way the records (n_cigar set) stay in
// kw_res, the packed words in kw_pack and their offsets in kw_off until the engine's next call.
int ksw_run(Engine &e, const KswConst &c, int64_t n_jobs, const mm2gb_ksw_job_t *jobs, const uint8_t *queries, const uint8_t *targets, const uint8_t *junc, bool resident,
            mm2gb_ksw_res_t *res, uint32_t **cigar, int64_t *n_cigar_total)
{
	if (n_jobs >= ((int64_t)1 << 31)) return fail("mm2gb_ksw_extd2_gpu / mm2gb_ksw_exts2_gpu: a batch is limited to 2^31 jobs");
	e.kw_ms[0] = e.kw_ms[1] = 0;
	*cigar = nullptr; *n_cigar_total = 0;
	// the jobs that run, each with its classes, cost and needs; the others get the reset record here
	struct Plan { KswDevJob d; int group; int64_t cost, slab, img; };
	std::vector<Plan> plan;
	KswEz reset;
	ksw_ez_reset(reset);
	int64_t q_bytes = 0, t_bytes = 0, cig_words = 0;
	for (int64_t j = 0; j < n_jobs; ++j) {
		const mm2gb_ksw_job_t &b = jobs[j];
		ksw_store(reset, 0, res + j);
		if (c.early || b.qlen <= 0 || b.tlen <= 0) continue;
		Plan P;
		const int w = ksw_width(b.qlen, b.tlen, c.form == KSW_SPLICE ? -1 : b.w), ncol = ksw_ncol16(b.qlen, b.tlen, w);
		const bool with_cigar = !(b.flag & MM2GB_KSW_SCORE_ONLY);
		P.d = { b.q_off, b.t_off, 0, cig_words, b.qlen, b.tlen, w, b.zdrop, b.end_bonus, b.flag, (int32_t)j, ncol };
		P.img = ksw_image_bytes(c.form, b.qlen, b.tlen, b.flag);
		P.slab = with_cigar ? ((int64_t)(b.qlen + b.tlen - 1) * ncol + 15) / 16 * 16 : 0;
		P.cost = (int64_t)(b.qlen + b.tlen - 1) * ((ncol + KSW_NT[2] - 1) / KSW_NT[2]);
		const int nt_class = ncol <= KSW_BAND[0] ? 0 : ncol <= KSW_BAND[1] ? 1 : 2;
		int lds_class = 0;
		while (lds_class < 4 && P.img > KSW_LDS_STEP[lds_class]) ++lds_class;      // 4: the image lives in global memory
		P.group = lds_class * 3 + nt_class;
		if (with_cigar) cig_words += (int64_t)b.qlen + b.tlen + 2;
		q_bytes = std::max(q_bytes, b.q_off + b.qlen); t_bytes = std::max(t_bytes, b.t_off + b.tlen);
		plan.push_back(P);
	}
	if (plan.empty()) return 0;
	// most expensive first within a class; a launch takes jobs of one class while their direction bytes fit the slab
	std::stable_sort(plan.begin(), plan.end(), [](const Plan &a, const Plan &b) { return a.group != b.group ? a.group > b.group : a.cost > b.cost; });
	std::vector<Launch> launches;
	std::vector<KswDevJob> dev(plan.size());
	const int64_t budget = slab_budget();
	int64_t slab_max = 0, img_max = 0;
	for (size_t k = 0; k < plan.size(); ++k) {
		const Plan &P = plan[k];
		if (launches.empty() || launches.back().nt_class + 3 * launches.back().lds_class != P.group || (launches.back().slab > 0 && launches.back().slab + P.slab > budget))
			launches.push_back({ (int)k, (int)k, P.group % 3, P.group / 3, 0, 0, 0 });
		Launch &L = launches.back();
		dev[k] = P.d; dev[k].slab_off = L.slab;
		L.slab += P.slab; L.hi = (int)k + 1;
		if (L.lds_class < 4) L.lds = KSW_LDS_STEP[L.lds_class]; else L.img = std::max(L.img, (P.img + 255) / 256 * 256);
		slab_max = std::max(slab_max, L.slab);
	}
	const int grid_global = e.n_cu * 2;
	for (const Launch &L : launches) img_max = std::max(img_max, L.img * std::min<int64_t>(grid_global, L.hi - L.lo));

	MM2GB_HIP(hipSetDevice(e.device));
	MM2GB_HIP(hipStreamSynchronize(e.stream));
	if (e.kw_jobs.ensure(dev.size() * sizeof(KswDevJob)) || (!resident && (e.kw_q.ensure((size_t)q_bytes) || e.kw_t.ensure((size_t)t_bytes))) || (junc && e.kw_junc.ensure((size_t)t_bytes)) || e.kw_res.ensure((size_t)n_jobs * sizeof(mm2gb_ksw_res_t)) ||
	    e.kw_slab.ensure((size_t)std::max<int64_t>(slab_max, 16)) || e.kw_cig.ensure((size_t)std::max<int64_t>(cig_words, 4) * 4) || e.kw_img.ensure((size_t)std::max<int64_t>(img_max, 16)) ||
	    e.kw_cnt.ensure(launches.size() * 4) || e.kw_off.ensure((size_t)n_jobs * 8)) return -1;
	hipEvent_t ev[4] = {};
	struct Events { hipEvent_t *e; ~Events() { for (int k = 0; k < 4; ++k) if (e[k]) (void)hipEventDestroy(e[k]); } } guard{ ev };
	for (hipEvent_t &x : ev) MM2GB_HIP(hipEventCreate(&x));
	MM2GB_HIP(hipMemcpyAsync(e.kw_jobs.ptr, dev.data(), dev.size() * sizeof(KswDevJob), hipMemcpyHostToDevice, e.stream));
	if (!resident) {
		MM2GB_HIP(hipMemcpyAsync(e.kw_q.ptr, queries, (size_t)q_bytes, hipMemcpyHostToDevice, e.stream));
		MM2GB_HIP(hipMemcpyAsync(e.kw_t.ptr, targets, (size_t)t_bytes, hipMemcpyHostToDevice, e.stream));
		if (junc) MM2GB_HIP(hipMemcpyAsync(e.kw_junc.ptr, junc, (size_t)t_bytes, hipMemcpyHostToDevice, e.stream));
	} else if ((size_t)q_bytes > e.kw_q.bytes || (size_t)t_bytes > e.kw_t.bytes) return fail("mm2gb_ksw_extd2_gpu: a resident job lies outside the sequence arenas");
	MM2GB_HIP(hipMemcpyAsync(e.kw_res.ptr, res, (size_t)n_jobs * sizeof(mm2gb_ksw_res_t), hipMemcpyHostToDevice, e.stream));
	MM2GB_HIP(hipMemsetAsync(e.kw_cnt.ptr, 0, launches.size() * 4, e.stream));
	MM2GB_HIP(hipEventRecord(ev[0], e.stream));
	for (size_t k = 0; k < launches.size(); ++k) {
		const Launch &L = launches[k];
		const int nt = KSW_NT[L.nt_class], n = L.hi - L.lo;
		const int per_cu = L.lds_class < 4 ? (int)std::max<int64_t>(1, std::min<int64_t>(std::min(2048 / nt, 8), (160 * 1024) / (L.lds + 1024))) : 2;
		if (launch_one(e, c, junc != nullptr, L, (int)k, std::min(n, e.n_cu * per_cu))) return -1;
		e.kw_class_jobs[L.lds_class < 4 ? 0 : 1] += n;
		if (L.slab > 0) {
			hipLaunchKernelGGL(k_ksw_walk, dim3((n + 63) / 64), dim3(64), 0, e.stream, (const KswDevJob*)e.kw_jobs.ptr, L.lo, L.hi, c.form == KSW_SPLICE ? c.long_thres : 0, (const uint8_t*)e.kw_slab.ptr, (uint32_t*)e.kw_cig.ptr,
			                   (mm2gb_ksw_res_t*)e.kw_res.ptr);
			MM2GB_HIP(hipGetLastError());
		}
	}
	MM2GB_HIP(hipEventRecord(ev[1], e.stream));
	MM2GB_HIP(hipMemcpyAsync(res, e.kw_res.ptr, (size_t)n_jobs * sizeof(mm2gb_ksw_res_t), hipMemcpyDeviceToHost, e.stream));
	MM2GB_HIP(hipStreamSynchronize(e.stream));
	if (ksw_gather(n_jobs, res, cigar, n_cigar_total)) return -1;
	float ms = 0;
	MM2GB_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
	e.kw_ms[0] = ms;
	if (*n_cigar_total == 0) return 0;
	std::vector<int64_t> off((size_t)n_jobs);
	for (int64_t j = 0; j < n_jobs; ++j) off[(size_t)j] = res[j].cigar_off;
	if (e.kw_pack.ensure((size_t)*n_cigar_total * 4)) { free(*cigar); *cigar = nullptr; return -1; }
	auto pack = [&]() -> int {
		MM2GB_HIP(hipMemcpyAsync(e.kw_off.ptr, off.data(), (size_t)n_jobs * 8, hipMemcpyHostToDevice, e.stream));
		MM2GB_HIP(hipEventRecord(ev[2], e.stream));
		hipLaunchKernelGGL(k_ksw_pack, dim3((unsigned)std::min<size_t>(dev.size(), (size_t)e.n_cu * 32)), dim3(64), 0, e.stream, (const KswDevJob*)e.kw_jobs.ptr, (int)dev.size(),
		                   (const mm2gb_ksw_res_t*)e.kw_res.ptr, (const int64_t*)e.kw_off.ptr, (const uint32_t*)e.kw_cig.ptr, (uint32_t*)e.kw_pack.ptr);
		MM2GB_HIP(hipGetLastError());
		MM2GB_HIP(hipEventRecord(ev[3], e.stream));
		MM2GB_HIP(hipStreamSynchronize(e.stream));
		MM2GB_HIP(hipMemcpyAsync(*cigar, e.kw_pack.ptr, (size_t)*n_cigar_total * 4, hipMemcpyDeviceToHost, e.s_out));
		MM2GB_HIP(hipStreamSynchronize(e.s_out));
		MM2GB_HIP(hipEventElapsedTime(&ms, ev[2], ev[3]));
		e.kw_ms[1] = ms;
		return 0;
	};
	if (pack()) { free(*cigar); *cigar = nullptr; *n_cigar_total = 0; return -1; }
	return 0;
}

} // namespace mm2gb

using namespace mm2gb;

int mm2gb_ksw_extd2_gpu(mm2gb_engine_t *eng, const mm2gb_ksw_param_t *param, int64_t n_jobs, const mm2gb_ksw_job_t *jobs, const uint8_t *queries,
                        const uint8_t *targets, mm2gb_ksw_res_t *res, uint32_t **cigar, int64_t *n_cigar_total)
{
	if (!eng) return fail("mm2gb: null engine");
	if (ksw_check("mm2gb_ksw_extd2_gpu", param, n_jobs, jobs, queries, targets, res, cigar, n_cigar_total)) return -1;
	return ksw_run(eng->e, ksw_derive(*param), n_jobs, jobs, queries, targets, nullptr, false, res, cigar, n_cigar_total);
}

int mm2gb_ksw_exts2_gpu(mm2gb_engine_t *eng, const mm2gb_ksw_splice_param_t *param, int64_t n_jobs, const mm2gb_ksw_job_t *jobs, const uint8_t *queries,
                        const uint8_t *targets, const uint8_t *junc, mm2gb_ksw_res_t *res, uint32_t **cigar, int64_t *n_cigar_total)
{
	if (!eng) return fail("mm2gb: null engine");
	if (ksw_check_splice("mm2gb_ksw_exts2_gpu", param, n_jobs, jobs, queries, targets, res, cigar, n_cigar_total)) return -1;
	return ksw_run(eng->e, ksw_derive_splice(*param), n_jobs, jobs, queries, targets, junc, false, res, cigar, n_cigar_total);
}

int mm2gb_ksw_extz2_gpu(mm2gb_engine_t *eng, const mm2gb_ksw_param_t *param, int64_t n_jobs, const mm2gb_ksw_job_t *jobs, const uint8_t *queries,
                        const uint8_t *targets, mm2gb_ksw_res_t *res, uint32_t **cigar, int64_t *n_cigar_total)
{
	if (!eng) return fail("mm2gb: null engine");
	if (ksw_check_single("mm2gb_ksw_extz2_gpu", param, n_jobs, jobs, queries, targets, res, cigar, n_cigar_total)) return -1;
	return ksw_run(eng->e, ksw_derive_single(*param), n_jobs, jobs, queries, targets, nullptr, false, res, cigar, n_cigar_total);
}

int mm2gb_ksw_gpu_class_jobs(mm2gb_engine_t *eng, int64_t *jobs2)
{
	if (!eng || !jobs2) return fail("mm2gb_ksw_gpu_class_jobs: null argument");
	jobs2[0] = eng->e.kw_class_jobs[0]; jobs2[1] = eng->e.kw_class_jobs[1];
	return 0;
}

int mm2gb_ksw_gpu_info(mm2gb_engine_t *eng, int64_t *consts6, double *ms2)
{
	if (consts6) { consts6[0] = KSW_NT[0]; consts6[1] = KSW_NT[1]; consts6[2] = KSW_NT[2]; consts6[3] = KSW_BAND[0]; consts6[4] = KSW_BAND[1]; consts6[5] = KSW_LDS_MAX; }
	if (ms2) { if (!eng) return fail("mm2gb: null engine"); ms2[0] = eng->e.kw_ms[0]; ms2[1] = eng->e.kw_ms[1]; }
	return 0;
}
