// est_err.cpp -- mm_est_err's walk (esterr.c:30-61) as a batched call on host threads: the definition of mm2gb_est_err_gpu (est_err_kernels.hip)
// and what the mapper's divergence estimate calls per read.  The walk is written as the reference writes it; the pow of esterr.c:62 is left to
// the caller (mm2gb_est_err_div), so that both forms give the same div bit for bit.
#include <cmath>
#include <string>
#include "engine.h"
#include "est_err.h"
#include "host_threads.h"

namespace mm2gb {

namespace {
// esterr.c:7-14
inline int32_t for_qpos(int32_t qlen, const mm2gb_anchor_t &a)
{
	const int32_t x = (int32_t)a.y, span = (int32_t)(a.y >> 32 & 0xff);
	return a.x >> 63 ? qlen - 1 - (x + 1 - span) : x;
}
}

void est_err_read(int32_t qlen, int64_t n_regs, const mm2gb_reg_t *regs, const mm2gb_anchor_t *a, int32_t n, const uint64_t *mini_pos, const int32_t *ref_len,
                  mm2gb_est_err_t *out, uint64_t *sum_k_out)
{
	uint64_t sum_k = 0;
	for (int32_t i = 0; i < n; ++i) sum_k += mini_pos[i] >> 32 & 0xff;
	*sum_k_out = sum_k;
	const float avg_k = n > 0 ? (float)sum_k / n : 0.0f;
	for (int64_t i = 0; i < n_regs; ++i) {
		const mm2gb_reg_t &r = regs[i];
		const bool rev = (r.flags >> 10) & 1;
		out[i].n_match = 0; out[i].n_tot = -1;
		if (n == 0 || r.cnt == 0) continue;                                                        // esterr.c:36, 45
		auto anchor = [&](int32_t k) -> const mm2gb_anchor_t & { return rev ? a[r.as + r.cnt - 1 - k] : a[r.as + k]; };   // in query order
		const int32_t x0 = for_qpos(qlen, anchor(0));
		int32_t L = 0, R = n - 1, st = -1;
		while (L <= R) {                                                                           // esterr.c:16-28
			const int32_t m = (int32_t)(((uint64_t)L + (uint64_t)R) >> 1), y = (int32_t)mini_pos[m];
			if (y < x0) L = m + 1; else if (y > x0) R = m - 1; else { st = m; break; }
		}
		if (st < 0) continue;                                                                      // esterr.c:47-51
		int32_t en = st, n_match = 1;
		for (int32_t k = 1, j = st + 1; j < n && k < r.cnt; ++j)                                   // esterr.c:53-58
			if (for_qpos(qlen, anchor(k)) == (int32_t)mini_pos[j]) { ++k; en = j; ++n_match; }
		int32_t n_tot = en - st + 1;
		if (r.qs > avg_k && r.rs > avg_k) ++n_tot;                                                 // esterr.c:60-61
		if (qlen - r.qs > avg_k && ref_len[r.rid] - r.re > avg_k) ++n_tot;
		out[i].n_match = n_match; out[i].n_tot = n_tot;
	}
}

int est_err_check(const char *who, int64_t n_reads, const int64_t *reg_off, const mm2gb_reg_t *regs, const int64_t *anchor_off, const mm2gb_anchor_t *anchors, const int32_t *qlen,
                  const int64_t *mini_off, const uint64_t *mini_pos, int32_t n_ref, const int32_t *ref_len, const mm2gb_est_err_t *out, const uint64_t *sum_k)
{
	const std::string w(who);
	if (n_reads < 0 || !reg_off || !anchor_off || !mini_off || (n_reads > 0 && (!qlen || !sum_k))) return fail(w + ": null argument");
	if (reg_off[0] != 0 || anchor_off[0] != 0 || mini_off[0] != 0) return fail(w + ": reg_off[0], anchor_off[0] and mini_off[0] must be 0");
	for (int64_t r = 0; r < n_reads; ++r) {
		if (reg_off[r + 1] < reg_off[r] || anchor_off[r + 1] < anchor_off[r] || mini_off[r + 1] < mini_off[r]) return fail(w + ": offsets must be non-decreasing");
		if (mini_off[r + 1] - mini_off[r] >= ((int64_t)1 << 31) || anchor_off[r + 1] - anchor_off[r] >= ((int64_t)1 << 31)) return fail(w + ": a read is limited to 2^31 minimizers and anchors");
	}
	if ((reg_off[n_reads] > 0 && (!regs || !out || !ref_len || n_ref <= 0)) || (anchor_off[n_reads] > 0 && !anchors) || (mini_off[n_reads] > 0 && !mini_pos)) return fail(w + ": null buffer");
	for (int64_t r = 0; r < n_reads; ++r) {
		const int64_t n_a = anchor_off[r + 1] - anchor_off[r];
		for (int64_t j = reg_off[r]; j < reg_off[r + 1]; ++j) {
			const mm2gb_reg_t &g = regs[j];
			if (g.cnt < 0 || g.as < 0 || (int64_t)g.as + g.cnt > n_a) return fail(w + ": a record's anchors lie outside its read's");
			if (g.rid < 0 || g.rid >= n_ref) return fail(w + ": a record names a reference sequence >= n_ref");
		}
	}
	return 0;
}

} // namespace mm2gb

using namespace mm2gb;

extern "C" {

int mm2gb_est_err_host(int64_t n_reads, const int64_t *reg_off, const mm2gb_reg_t *regs, const int64_t *anchor_off, const mm2gb_anchor_t *anchors, const int32_t *qlen,
                       const int64_t *mini_off, const uint64_t *mini_pos, int32_t n_ref, const int32_t *ref_len, int n_threads, mm2gb_est_err_t *out, uint64_t *sum_k)
{
	if (est_err_check("mm2gb_est_err_host", n_reads, reg_off, regs, anchor_off, anchors, qlen, mini_off, mini_pos, n_ref, ref_len, out, sum_k)) return -1;
	for_each_on_threads((size_t)n_reads, n_threads, 8, [&](size_t r) {
		est_err_read(qlen[r], reg_off[r + 1] - reg_off[r], regs + reg_off[r], anchors + anchor_off[r], (int32_t)(mini_off[r + 1] - mini_off[r]), mini_pos + mini_off[r], ref_len,
		             out + reg_off[r], sum_k + r);
	});
	return 0;
}

// esterr.c:39, 62 from the walk's result: -1 where the walk did not start
float mm2gb_est_err_div(int32_t n_match, int32_t n_tot, uint64_t sum_k, int32_t n_mini)
{
	if (n_tot < 0 || n_mini <= 0) return -1.0f;
	const float avg_k = (float)sum_k / n_mini;
	return n_match >= n_tot ? 0.0f : (float)(1.0 - pow((double)n_match / n_tot, 1.0 / avg_k));
}

} // extern "C"
