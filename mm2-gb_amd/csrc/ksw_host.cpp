// ksw_host.cpp -- the dual-affine extension DP (mm2gb_ksw_extd2_host), the splice-aware one (mm2gb_ksw_exts2_host) and the
// single-affine one (mm2gb_ksw_extz2_host) on host threads: the definitions the device forms are held to.
// One job at a time per thread, one cell at a time, over the same arrays the reference's vector code keeps: six difference
// arrays and the score bytes, rounded out to groups of 16 cells, 32-bit H when the exact maximum is wanted, one row of direction bytes per
// anti-diagonal.  The arithmetic is ksw_cell.h's, shared with the kernel.
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "engine.h"
#include "host_threads.h"
#include "ksw_cell.h"
#include "ksw_host.h"

namespace mm2gb {

namespace {

// what every DP refuses in a job: flag bits outside known, bad lengths, too many cells, residues >= m (looked at from m = min_m on: below
// it the DP returns before it reads a residue)
int check_jobs(const std::string &w, int m, int known, int64_t n_jobs, const mm2gb_ksw_job_t *jobs, const uint8_t *queries, const uint8_t *targets, int min_m = 2)
{
	static const struct { int bit; const char *name; } refused[] = { { 0x20, "bit 0x20 (unassigned)" }, { 0x100, "KSW_EZ_SPLICE_FOR" }, { 0x200, "KSW_EZ_SPLICE_REV" }, { 0x400, "KSW_EZ_SPLICE_FLANK" } };
	for (int64_t j = 0; j < n_jobs; ++j) {
		const mm2gb_ksw_job_t &b = jobs[j];
		const std::string at = w + ": job " + std::to_string(j) + ": ";
		if (b.flag & ~known) {
			for (const auto &x : refused) if (b.flag & ~known & x.bit) return fail(at + "flag " + x.name + " is not supported");
			return fail(at + "unknown flag bits " + std::to_string(b.flag & ~known));
		}
		if (b.qlen < 0 || b.tlen < 0 || b.q_off < 0 || b.t_off < 0) return fail(at + "negative length or offset");
		if ((int64_t)b.qlen * b.tlen > MM2GB_KSW_MAX_CELLS) return fail(at + "qlen * tlen = " + std::to_string((int64_t)b.qlen * b.tlen) + " exceeds MM2GB_KSW_MAX_CELLS");
		if ((b.qlen > 0 && !queries) || (b.tlen > 0 && !targets)) return fail(at + "null sequence array");
		if (m >= min_m) {
			for (int k = 0; k < b.qlen; ++k) if (queries[b.q_off + k] >= m) return fail(at + "query residue >= m at " + std::to_string(k));
			for (int k = 0; k < b.tlen; ++k) if (targets[b.t_off + k] >= m) return fail(at + "target residue >= m at " + std::to_string(k));
		}
	}
	return 0;
}

// what both parameter records are refused for first: null arguments and m
template <class Param>
int check_head(const std::string &w, const Param *param, int64_t n_jobs, const mm2gb_ksw_job_t *jobs, const mm2gb_ksw_res_t *res, uint32_t **cigar, int64_t *n_cigar_total)
{
	if (!param || n_jobs < 0 || (n_jobs > 0 && (!jobs || !res)) || !cigar || !n_cigar_total) return fail(w + ": null argument");
	if (param->m < 0 || param->m > 5) return fail(w + ": m must be 0..5");
	return 0;
}

} // namespace

int ksw_check(const char *who, const mm2gb_ksw_param_t *param, int64_t n_jobs, const mm2gb_ksw_job_t *jobs, const uint8_t *queries, const uint8_t *targets,
              const mm2gb_ksw_res_t *res, uint32_t **cigar, int64_t *n_cigar_total)
{
	const std::string w = who;
	if (check_head(w, param, n_jobs, jobs, res, cigar, n_cigar_total)) return -1;
	return check_jobs(w, param->m, KSW_FLAGS_KNOWN, n_jobs, jobs, queries, targets);
}

// The parameters are refused before anything is looked at that returns early: e <= 0 is an error even where q2 <= q + e.
int ksw_check_splice(const char *who, const mm2gb_ksw_splice_param_t *param, int64_t n_jobs, const mm2gb_ksw_job_t *jobs, const uint8_t *queries, const uint8_t *targets,
                     const mm2gb_ksw_res_t *res, uint32_t **cigar, int64_t *n_cigar_total)
{
	const std::string w = who;
	if (check_head(w, param, n_jobs, jobs, res, cigar, n_cigar_total)) return -1;
	if (param->e <= 0) return fail(w + ": e must be above 0 (the reference divides by it)");
	if (param->q < 0 || param->q2 < 0) return fail(w + ": q and q2 must not be negative");
	if (param->q + param->e > 127) return fail(w + ": q + e exceeds 127");
	if (param->noncan < 0) return fail(w + ": noncan must be 0..127");
	if (param->junc_bonus < 0) return fail(w + ": junc_bonus must be 0..127");
	return check_jobs(w, param->m, KSW_FLAGS_KNOWN | KSW_SPLICE_BITS, n_jobs, jobs, queries, targets);
}

// The single-affine form: what ksw_check refuses, then the costs (options.c:205, 215), then the jobs once more for the residues of m == 1,
// which this DP reads.  The splice bits are outside KSW_FLAGS_KNOWN and so refused by name.
int ksw_check_single(const char *who, const mm2gb_ksw_param_t *param, int64_t n_jobs, const mm2gb_ksw_job_t *jobs, const uint8_t *queries, const uint8_t *targets,
                     const mm2gb_ksw_res_t *res, uint32_t **cigar, int64_t *n_cigar_total)
{
	const std::string w = who;
	if (ksw_check(who, param, n_jobs, jobs, queries, targets, res, cigar, n_cigar_total)) return -1;
	if (param->q <= 0 || param->e <= 0) return fail(w + ": q and e must be above 0");
	if (2 * (param->q + param->e) > 127) return fail(w + ": 2 * (q + e) exceeds 127");
	return param->m == 1 ? check_jobs(w, 1, KSW_FLAGS_KNOWN, n_jobs, jobs, queries, targets, 1) : 0;
}

namespace {

struct Scratch { std::vector<int8_t> a; std::vector<int32_t> H; std::vector<uint8_t> p; std::vector<uint32_t> cig; };

// FORM: c.form.  The splice-aware form (junc the job's annotation bytes or null) has no band, and y2's array holds donor[] with acceptor[]
// behind the score bytes.  The single-affine form reads neither x2 nor y2; its arrays start as zeros, which is what its c.ini is.
template <int FORM>
void one_job(const KswConst &c, const mm2gb_ksw_job_t &job, const uint8_t *query, const uint8_t *target, const uint8_t *junc, Scratch &S,
             mm2gb_ksw_res_t *out, std::vector<uint32_t> &words)
{
	constexpr bool SPLICE = FORM == KSW_SPLICE;
	KswEz z;
	ksw_ez_reset(z);
	const int qlen = job.qlen, tlen = job.tlen, flag = job.flag;
	if (c.early || qlen <= 0 || tlen <= 0) { ksw_store(z, 0, out); return; }
	const int w = ksw_width(qlen, tlen, SPLICE ? -1 : job.w), T = ksw_round16(tlen), ncol = ksw_ncol16(qlen, tlen, w);
	const bool with_cigar = !(flag & MM2GB_KSW_SCORE_ONLY), approx = (flag & MM2GB_KSW_APPROX_MAX) != 0, right = (flag & MM2GB_KSW_RIGHT) != 0, generic = (flag & MM2GB_KSW_GENERIC_SC) != 0;
	S.a.resize((size_t)T * 8);
	int8_t *u = S.a.data(), *v = u + T, *x = v + T, *y = x + T, *x2 = y + T, *y2 = x2 + T, *s = y2 + T, *don = y2, *acc = s + T;
	memset(u, c.ini, (size_t)T * 4); memset(x2, c.ini2, (size_t)T * 2); memset(s, 0, (size_t)T);
	if (SPLICE) for (int t = 0; t < T; ++t) ksw_splice_sites(c, flag, [&](int i) { return target[i]; }, junc, tlen, t, don + t, acc + t);
	int32_t *H = nullptr;
	if (!approx) { S.H.assign((size_t)T, MM2GB_KSW_NEG_INF); H = S.H.data(); }
	if (with_cigar) S.p.resize((size_t)(qlen + tlen - 1) * ncol);
	uint8_t *p = S.p.data();
	int32_t H0 = 0; int H0_t = 0, last_st = -1, last_en = -1;
	for (int r = 0; r < qlen + tlen - 1; ++r) {
		int st0, en0;
		ksw_band(r, qlen, tlen, w, &st0, &en0);
		if (st0 > en0) { z.zdropped = 1; break; }
		const int st = st0 / 16 * 16, en = (en0 + 16) / 16 * 16 - 1;
		int8_t x1 = c.ini, x21 = c.ini2, v1 = c.ini;
		if (st > 0) { if (st - 1 >= last_st && st - 1 <= last_en) { x1 = x[st - 1]; x21 = x2[st - 1]; v1 = v[st - 1]; } }
		else v1 = ksw_edge<FORM>(c, r);
		const int8_t bv1 = v1;                             // the single-affine form smears it over three more cells (6d-c 9)
		if (en >= r) { y[r] = c.ini; if (!SPLICE) y2[r] = c.ini2; u[r] = ksw_edge<FORM>(c, r); }
		// the score bytes: whole groups of 16 from st0 unless the matrix is looked up, and nothing beyond the array (trap 2)
		const int s_end = generic ? en0 + 1 : std::min(T, st0 + ((en0 - st0) / 16 + 1) * 16);
		for (int t = st0; t < s_end; ++t) s[t] = ksw_score(c, c.mat, generic, ksw_target_byte(target, query, qlen, tlen, T, t), ksw_query_byte(query, qlen, r, t));
		uint8_t *pr = with_cigar ? p + (size_t)r * ncol - st : nullptr;
		for (int t = st; t <= en; ++t) {
			const KswCell o = FORM == KSW_SINGLE ? ksw_cell_single(c, right, s[t], x1, ksw_smear(bv1, t - st, v1), u[t], y[t])
			                : SPLICE ? ksw_cell_splice(c, right, s[t], x1, v1, x21, u[t], y[t], don[t], acc[t]) : ksw_cell(c, right, s[t], x1, v1, x21, u[t], y[t], y2[t]);
			x1 = x[t]; v1 = v[t]; x21 = x2[t];
			u[t] = o.u; v[t] = o.v; x[t] = o.x; y[t] = o.y;
			if (FORM != KSW_SINGLE) x2[t] = o.x2;
			if (FORM == KSW_DUAL) y2[t] = o.y2;
			if (pr) pr[t] = o.d;
		}
		bool stop;
		if (!approx) {
			uint64_t key;
			if (r > 0) {
				H[en0] = en0 > 0 ? H[en0 - 1] + ksw_diff<FORM>(c, u[en0]) : H[en0] + ksw_diff<FORM>(c, v[en0]);
				key = ksw_max_key(H[en0], en0, st0, en0);
				for (int t = st0; t < en0; ++t) { H[t] += ksw_diff<FORM>(c, v[t]); key = std::max(key, ksw_max_key(H[t], t, st0, en0)); }
			} else { H[0] = ksw_diff<FORM>(c, v[0]) - c.qe0; key = ksw_max_key(H[0], 0, 0, 0); }
			stop = ksw_row_exact(z, c, qlen, tlen, job.zdrop, r, st0, en0, en, ksw_key_H(key), ksw_key_t(key, st0, en0), H[en0], H[st0]);
		} else {
			stop = ksw_row_approx<FORM>(z, c, qlen, tlen, job.zdrop, flag, r, st0, en0, H0, H0_t, [&](int t) { return ksw_diff<FORM>(c, v[t]); }, [&](int t) { return ksw_diff<FORM>(c, u[t]); });
		}
		if (stop) break;
		last_st = st; last_en = en;
	}
	int i0 = 0, j0 = 0, n = 0;
	if (ksw_walk_from(z, SPLICE, qlen, tlen, job.end_bonus, flag, &i0, &j0)) {
		S.cig.resize((size_t)qlen + tlen + 2);
		n = ksw_walk(qlen, tlen, w, SPLICE ? c.long_thres : 0, i0, j0, [&](int r, int col) { return (uint32_t)p[(size_t)r * ncol + col]; }, [&](int k, uint32_t word) { S.cig[(size_t)k] = word; });
		if (!(flag & MM2GB_KSW_REV_CIGAR)) std::reverse(S.cig.begin(), S.cig.begin() + n);
		words.insert(words.end(), S.cig.begin(), S.cig.begin() + n);
	}
	ksw_store(z, n, out);
}

using OneJob = void (*)(const KswConst&, const mm2gb_ksw_job_t&, const uint8_t*, const uint8_t*, const uint8_t*, Scratch&, mm2gb_ksw_res_t*, std::vector<uint32_t>&);
inline OneJob one_job_of(const KswConst &c) { return c.form == KSW_SPLICE ? one_job<KSW_SPLICE> : c.form == KSW_SINGLE ? one_job<KSW_SINGLE> : one_job<KSW_DUAL>; }

} // namespace

void ksw_one_host(const KswConst &c, const mm2gb_ksw_job_t &job, const uint8_t *query, const uint8_t *target, mm2gb_ksw_res_t *out, std::vector<uint32_t> &words)
{
	static thread_local Scratch S;                        // carries only capacity between calls: one_job sizes and writes every array for a job before it reads it
	one_job_of(c)(c, job, query, target, nullptr, S, out, words);
}

int ksw_gather(int64_t n_jobs, mm2gb_ksw_res_t *res, uint32_t **cigar, int64_t *n_cigar_total)
{
	int64_t total = 0;
	for (int64_t j = 0; j < n_jobs; ++j) { res[j].cigar_off = total; total += res[j].n_cigar; }
	*n_cigar_total = total; *cigar = nullptr;
	if (total > 0 && !(*cigar = (uint32_t*)malloc((size_t)total * 4))) return fail("mm2gb_ksw_extd2: out of memory for the CIGAR words");
	return 0;
}

} // namespace mm2gb

using namespace mm2gb;

namespace {

int host_batch(const KswConst &c, int64_t n_jobs, const mm2gb_ksw_job_t *jobs, const uint8_t *queries, const uint8_t *targets, const uint8_t *junc,
               int n_threads, mm2gb_ksw_res_t *res, uint32_t **cigar, int64_t *n_cigar_total)
{
	const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(n_threads, 256), n_jobs));
	// jobs are dealt in runs of 16; a thread keeps the words of its jobs with the job's index, and they are laid out in job order at the end
	std::vector<std::vector<uint32_t>> words((size_t)nt);
	std::vector<int64_t> where((size_t)std::max<int64_t>(n_jobs, 1), 0);
	std::vector<int32_t> who((size_t)std::max<int64_t>(n_jobs, 1), 0);
	std::atomic<int64_t> next(0);
	const OneJob one = one_job_of(c);
	auto work = [&](int k) {
		Scratch S;
		for (;;) {
			const int64_t lo = next.fetch_add(16), hi = std::min(n_jobs, lo + 16);
			if (lo >= n_jobs) break;
			for (int64_t j = lo; j < hi; ++j) {
				who[(size_t)j] = k; where[(size_t)j] = (int64_t)words[(size_t)k].size();
				one(c, jobs[j], queries + jobs[j].q_off, targets + jobs[j].t_off, junc ? junc + jobs[j].t_off : nullptr, S, res + j, words[(size_t)k]);
			}
		}
	};
	run_on_threads(nt, work);
	if (ksw_gather(n_jobs, res, cigar, n_cigar_total)) return -1;
	for (int64_t j = 0; j < n_jobs; ++j)
		if (res[j].n_cigar > 0) memcpy(*cigar + res[j].cigar_off, words[(size_t)who[(size_t)j]].data() + where[(size_t)j], (size_t)res[j].n_cigar * 4);
	return 0;
}

} // namespace

int mm2gb_ksw_extd2_host(const mm2gb_ksw_param_t *param, int64_t n_jobs, const mm2gb_ksw_job_t *jobs, const uint8_t *queries, const uint8_t *targets,
                         int n_threads, mm2gb_ksw_res_t *res, uint32_t **cigar, int64_t *n_cigar_total)
{
	if (ksw_check("mm2gb_ksw_extd2_host", param, n_jobs, jobs, queries, targets, res, cigar, n_cigar_total)) return -1;
	return host_batch(ksw_derive(*param), n_jobs, jobs, queries, targets, nullptr, n_threads, res, cigar, n_cigar_total);
}

int mm2gb_ksw_exts2_host(const mm2gb_ksw_splice_param_t *param, int64_t n_jobs, const mm2gb_ksw_job_t *jobs, const uint8_t *queries, const uint8_t *targets,
                         const uint8_t *junc, int n_threads, mm2gb_ksw_res_t *res, uint32_t **cigar, int64_t *n_cigar_total)
{
	if (ksw_check_splice("mm2gb_ksw_exts2_host", param, n_jobs, jobs, queries, targets, res, cigar, n_cigar_total)) return -1;
	return host_batch(ksw_derive_splice(*param), n_jobs, jobs, queries, targets, junc, n_threads, res, cigar, n_cigar_total);
}

// q2 and e2 of the record are not read
int mm2gb_ksw_extz2_host(const mm2gb_ksw_param_t *param, int64_t n_jobs, const mm2gb_ksw_job_t *jobs, const uint8_t *queries, const uint8_t *targets,
                         int n_threads, mm2gb_ksw_res_t *res, uint32_t **cigar, int64_t *n_cigar_total)
{
	if (ksw_check_single("mm2gb_ksw_extz2_host", param, n_jobs, jobs, queries, targets, res, cigar, n_cigar_total)) return -1;
	return host_batch(ksw_derive_single(*param), n_jobs, jobs, queries, targets, nullptr, n_threads, res, cigar, n_cigar_total);
}
