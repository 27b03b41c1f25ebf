// align_host.cpp -- base-level alignment of hits (mm2gb_align_regs_host): mm_align_skeleton (align.c:960-1020) with what it calls
// in align.c and hit.c, written from scratch as a batch call.  A chain's DP jobs -- left extension, gap fills, right extension -- follow from its
// anchors alone (no DP result moves a job's coordinates; a z-drop only ends the chain and splits off a tail), so a chain is PLANNED into a
// job list, the jobs are run by a backend, and the results are STITCHED; split tails and inversion alignments are the next round's jobs.
// The host form runs a read at a time with the host DP (ksw_host.cpp) as its backend; the device form (align_kernels.hip) runs every read
// of the batch through the same planning and stitching with the device's DP behind it.  The host form is the definition.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "engine.h"
#include "host_threads.h"
#include "align_host.h"
#include "host_chain.h"
#include "ksw_host.h"

namespace mm2gb {

namespace {

constexpr uint64_t SEED_LONG_JOIN = 1ULL << 40, SEED_IGNORE = 1ULL << 41, SEED_TANDEM = 1ULL << 42, SEED_SELF = 1ULL << 43;
// mm_reg1_t's bit-field word (minimap.h:115)
constexpr uint32_t RF_SPLIT1 = 1u << 8, RF_SPLIT2 = 1u << 9, RF_REV = 1u << 10, RF_INV = 1u << 11, RF_SAM_PRI = 1u << 12, RF_SEG_SPLIT = 1u << 15, RF_SPLIT_INV = 1u << 24;
constexpr int PARENT_UNSET = -1, PARENT_TMP_PRI = -2;

inline int32_t ax(const mm2gb_anchor_t &a) { return (int32_t)a.x; }
inline int32_t ay(const mm2gb_anchor_t &a) { return (int32_t)a.y; }
inline int32_t aspan(const mm2gb_anchor_t &a) { return (int32_t)(a.y >> 32 & 0xff); }

struct Fill { int32_t rs, qs, re, qe, i, run; };
struct Plan { int32_t as1, cnt1, rid, rev, rs, qs, re, qe, rs0, qs0, re0, qe0, left, right, n_runs, trials; std::vector<Fill> fills; };      // n_runs: its jobs; trials: 2 when they lie in the round twice
enum { ST_DONE, ST_FRESH, ST_PENDING, ST_INV_FRESH, ST_INV_PENDING };
struct Reg {
	mm2gb_reg_t r;
	bool has_p = false;
	int32_t dp_score = 0, dp_max = 0, dp_max2 = 0, n_ambi = 0, trans_strand = 0;
	std::vector<uint32_t> cig;
	int state = ST_FRESH, plan = -1;
	AlRun inv;                       // an inversion's alignment job, and where its coordinates start from
	int32_t inv_q = 0;
};
struct Read {
	int64_t id = 0;
	int32_t qlen = 0, n_a = 0, rounds = 0;
	std::vector<mm2gb_anchor_t> a;
	std::vector<Reg> regs;
	std::vector<Plan> plans;
	std::vector<AlRun> runs;         // this round's jobs; first_run: where they begin in the round's array
	int64_t first_run = 0;
	int64_t cnt[MM2GB_ALN_N_COUNTS] = {};
	int64_t scnt[MM2GB_SPL_N_COUNTS] = {};      // the spliced form's
	int64_t srcnt[MM2GB_SR_N_COUNTS] = {};      // the short-read form's
};

inline uint8_t read_base(const AlCtx &c, int64_t read, int strand, int p)
{
	const int64_t at = c.read_at[(size_t)read];
	if (!strand) return c.reads[(size_t)(at + p)];
	const int n = (int)(c.read_at[(size_t)read + 1] - at);
	const uint8_t x = c.reads[(size_t)(at + n - 1 - p)];
	return x < 4 ? 3 - x : 4;
}

// ---- mm_reg_set_coor with mm_cal_fuzzy_len (hit.c:8-38), not on the query strand ----
void reg_set_coor(mm2gb_reg_t &r, int32_t qlen, const mm2gb_anchor_t *a)
{
	const int32_t k = r.as, q_span = aspan(a[k]);
	const bool rev = a[k].x >> 63;
	r.flags = rev ? r.flags | RF_REV : r.flags & ~RF_REV;
	r.rid = (int32_t)(a[k].x << 1 >> 33);
	r.rs = ax(a[k]) + 1 > q_span ? ax(a[k]) + 1 - q_span : 0;
	r.re = ax(a[k + r.cnt - 1]) + 1;
	if (!rev) { r.qs = ay(a[k]) + 1 - q_span; r.qe = ay(a[k + r.cnt - 1]) + 1; }
	else { r.qs = qlen - (ay(a[k + r.cnt - 1]) + 1); r.qe = qlen - (ay(a[k]) + 1 - q_span); }
	r.mlen = r.blen = 0;
	if (r.cnt <= 0) return;
	r.mlen = r.blen = aspan(a[r.as]);
	for (int i = r.as + 1; i < r.as + r.cnt; ++i) {
		const int span = aspan(a[i]), tl = ax(a[i]) - ax(a[i - 1]), ql = ay(a[i]) - ay(a[i - 1]);
		r.blen += tl > ql ? tl : ql;
		r.mlen += tl > span && ql > span ? span : tl < ql ? tl : ql;
	}
}

// ---- mm_split_reg (hit.c:106-123); false: nothing split ----
bool split_reg(mm2gb_reg_t &r, mm2gb_reg_t &r2, int n, int qlen, const mm2gb_anchor_t *a)
{
	if (n <= 0 || n >= r.cnt) return false;
	r2 = r;
	r2.id = -1;
	r2.flags &= ~(RF_SAM_PRI | RF_SPLIT_INV);
	r2.cnt = r.cnt - n;
	r2.score = (int32_t)(r.score * ((float)r2.cnt / r.cnt) + .499);
	r2.as = r.as + n;
	if (r.parent == r.id) r2.parent = PARENT_TMP_PRI;
	reg_set_coor(r2, qlen, a);
	r.cnt -= r2.cnt;
	r.score -= r2.score;
	reg_set_coor(r, qlen, a);
	r.flags |= RF_SPLIT1; r2.flags |= RF_SPLIT2;
	return true;
}

// ---- mm_fix_bad_ends (align.c:462-496) ----
void fix_bad_ends(const mm2gb_reg_t &r, const mm2gb_anchor_t *a, int bw, int min_match, int32_t *as, int32_t *cnt)
{
	int32_t i, l, m;
	*as = r.as; *cnt = r.cnt;
	if (r.cnt < 3) return;
	m = l = aspan(a[r.as]);
	for (i = r.as + 1; i < r.as + r.cnt - 1; ++i) {
		const int32_t q_span = aspan(a[i]);
		if (a[i].y & SEED_LONG_JOIN) break;
		const int32_t lr = ax(a[i]) - ax(a[i - 1]), lq = ay(a[i]) - ay(a[i - 1]), mn = lr < lq ? lr : lq, mx = lr > lq ? lr : lq;
		if (mx - mn > l >> 1) *as = i;
		l += mn;
		m += mn < q_span ? mn : q_span;
		if (l >= bw << 1 || (m >= min_match && m >= bw) || m >= r.mlen >> 1) break;
	}
	*cnt = r.as + r.cnt - *as;
	m = l = aspan(a[r.as + r.cnt - 1]);
	for (i = r.as + r.cnt - 2; i > *as; --i) {
		const int32_t q_span = aspan(a[i + 1]);
		if (a[i + 1].y & SEED_LONG_JOIN) break;
		const int32_t lr = ax(a[i + 1]) - ax(a[i]), lq = ay(a[i + 1]) - ay(a[i]), mn = lr < lq ? lr : lq, mx = lr > lq ? lr : lq;
		if (mx - mn > l >> 1) *cnt = i + 1 - *as;
		l += mn;
		m += mn < q_span ? mn : q_span;
		if (l >= bw << 1 || (m >= min_match && m >= bw) || m >= r.mlen >> 1) break;
	}
}

int ll_i16(const AlCtx &c, int qlen, const uint8_t *query, int tlen, const uint8_t *target, int gapo, int gape, int *qe, int *te);

// ---- mm_seed_ext_score (align.c:526-551): the anchor's span widened by anchor_ext_len on both sides, the query on the anchor's strand ----
int seed_ext_score(const AlCtx &c, const Read &R, const mm2gb_anchor_t &a)
{
	const int32_t q_span = aspan(a), rid = (int32_t)(a.x << 1 >> 33), ext = c.anchor_ext_len, strand = (int32_t)(a.x >> 63);
	const int32_t ref_len = (int32_t)(c.ref_at[(size_t)rid + 1] - c.ref_at[(size_t)rid]);
	int32_t re = ax(a) + 1, rs = re - q_span, qe = ay(a) + 1, qs = qe - q_span;
	rs = rs - ext > 0 ? rs - ext : 0;
	qs = qs - ext > 0 ? qs - ext : 0;
	re = re + ext < ref_len ? re + ext : ref_len;
	qe = qe + ext < R.qlen ? qe + ext : R.qlen;
	std::vector<uint8_t> q((size_t)std::max(qe - qs, 0)), t((size_t)std::max(re - rs, 0));
	for (int k = 0; k < qe - qs; ++k) q[(size_t)k] = read_base(c, R.id, strand, qs + k);
	for (int k = 0; k < re - rs; ++k) t[(size_t)k] = c.refs[(size_t)(c.ref_at[(size_t)rid] + rs + k)];
	int q_off, t_off;
	return ll_i16(c, (int)q.size(), q.data(), (int)t.size(), t.data(), c.opt.q, c.opt.e, &q_off, &t_off);
}

// ---- mm_fix_bad_ends_splice (align.c:553-571): an end anchor shorter than ln(distance to its neighbour) + anchor_ext_shift is probed and, where
//      the probe's score / a is below that too, left out.  Reads positions, spans and sequences; no seed flag, no DP result ----
void fix_bad_ends_splice(const AlCtx &c, Read &R, const mm2gb_reg_t &r, const mm2gb_anchor_t *a, int32_t *as, int32_t *cnt)
{
	*as = r.as; *cnt = r.cnt;
	if (r.cnt < 3) return;
	double log_gap = log(ax(a[r.as + 1]) - ax(a[r.as]));
	if (aspan(a[r.as]) < log_gap + c.anchor_ext_shift) {
		const int score = seed_ext_score(c, R, a[r.as]);
		if ((double)score / c.mat[0] < log_gap + c.anchor_ext_shift) { ++*as; --*cnt; ++R.scnt[MM2GB_SPL_N_END_FLT_HEAD]; }
		else ++R.scnt[MM2GB_SPL_N_END_FLT_PROBE_KEPT];
	}
	log_gap = log(ax(a[r.as + r.cnt - 1]) - ax(a[r.as + r.cnt - 2]));
	if (aspan(a[r.as + r.cnt - 1]) < log_gap + c.anchor_ext_shift) {
		const int score = seed_ext_score(c, R, a[r.as + r.cnt - 1]);
		if ((double)score / c.mat[0] < log_gap + c.anchor_ext_shift) { --*cnt; ++R.scnt[MM2GB_SPL_N_END_FLT_TAIL]; }
		else ++R.scnt[MM2GB_SPL_N_END_FLT_PROBE_KEPT];
	}
}

// ---- collect_long_gaps, mm_filter_bad_seeds, mm_filter_bad_seeds_alt (align.c:370-460) ----
inline int gap_at(const mm2gb_anchor_t *a, int i) { return (ay(a[i]) - ay(a[i - 1])) - (ax(a[i]) - ax(a[i - 1])); }

bool collect_long_gaps(int as1, int cnt1, const mm2gb_anchor_t *a, int min_gap, std::vector<int> &K)
{
	K.clear();
	for (int i = 1; i < cnt1; ++i) {
		const int gap = gap_at(a, as1 + i);
		if (gap < -min_gap || gap > min_gap) K.push_back(i);
	}
	return K.size() > 1;
}

void filter_bad_seeds(int as1, int cnt1, mm2gb_anchor_t *a, int min_gap, int diff_thres, int max_ext_len, int max_ext_cnt, std::vector<int> &K)
{
	if (!collect_long_gaps(as1, cnt1, a, min_gap, K)) return;
	const int n = (int)K.size();
	int max = 0, max_st = -1, max_en = -1;
	for (int k = 0;; ++k) {
		int gap, l, n_ins = 0, n_del = 0, max_diff = 0, max_diff_l = -1;
		if (k == n || k >= max_en) {
			if (max_en > 0)
				for (int i = K[max_st]; i < K[max_en]; ++i) a[as1 + i].y |= SEED_IGNORE;
			max = 0; max_st = max_en = -1;
			if (k == n) break;
		}
		const int i = K[k];
		gap = gap_at(a, as1 + i);
		if (gap > 0) n_ins += gap; else n_del += -gap;
		const int qs = ay(a[as1 + i - 1]), rs = ax(a[as1 + i - 1]);
		for (l = k + 1; l < n && l <= k + max_ext_cnt; ++l) {
			const int j = K[l];
			if (ay(a[as1 + j]) - qs > max_ext_len || ax(a[as1 + j]) - rs > max_ext_len) break;
			gap = gap_at(a, as1 + j);
			if (gap > 0) n_ins += gap; else n_del += -gap;
			const int diff = n_ins + n_del - abs(n_ins - n_del);
			if (max_diff < diff) { max_diff = diff; max_diff_l = l; }
		}
		if (max_diff > diff_thres && max_diff > max) { max = max_diff; max_st = k; max_en = max_diff_l; }
	}
}

void filter_bad_seeds_alt(int as1, int cnt1, mm2gb_anchor_t *a, int min_gap, int max_ext, std::vector<int> &K)
{
	if (!collect_long_gaps(as1, cnt1, a, min_gap, K)) return;
	const int n = (int)K.size();
	for (int k = 0; k < n;) {
		const int i = K[k];
		int l, gap1 = gap_at(a, as1 + i), re1 = ax(a[as1 + i]), qe1 = ay(a[as1 + i]);
		gap1 = gap1 > 0 ? gap1 : -gap1;
		for (l = k + 1; l < n; ++l) {
			const int j = K[l];
			if (ay(a[as1 + j]) - qe1 > max_ext || ax(a[as1 + j]) - re1 > max_ext) break;
			int gap2 = gap_at(a, as1 + j);
			const int q_span_pre = aspan(a[as1 + j - 1]), rs2 = ax(a[as1 + j - 1]) + q_span_pre, qs2 = ay(a[as1 + j - 1]) + q_span_pre;
			const int m = rs2 - re1 < qs2 - qe1 ? rs2 - re1 : qs2 - qe1;
			gap2 = gap2 > 0 ? gap2 : -gap2;
			if (m > gap1 + gap2) break;
			re1 = ax(a[as1 + j]); qe1 = ay(a[as1 + j]);
			gap1 = gap2;
		}
		if (l > k + 1) {
			const int end = K[l - 1];
			for (int j = K[k]; j < end; ++j) a[as1 + j].y |= SEED_IGNORE;
			a[as1 + end].y |= SEED_LONG_JOIN;
		}
		k = l;
	}
}

// ---- mm_adjust_minier (align.c:344-368): where an anchor's alignment coordinates lie.  HPC: the start of the query's run that ends the
//      minimizer (the loop never looks at index 0, as the reference's does not), and the start of the reference's run read backwards ----
void adjust_minier(const AlCtx &c, Read &R, const mm2gb_anchor_t &a, int32_t *r, int32_t *q)
{
	if (c.idx_flag & MM2GB_I_HPC) {
		const int strand = (int)(a.x >> 63);
		int i;
		*q = ay(a);
		const uint8_t cq = read_base(c, R.id, strand, *q);
		for (i = *q - 1; i > 0; --i)
			if (read_base(c, R.id, strand, i) != cq) break;
		if (i + 1 != *q) ++R.cnt[MM2GB_ALN_N_HPC_MOVED];
		*q = i + 1;
		const int64_t off0 = c.ref_at[(size_t)(a.x << 1 >> 33)], off = off0 + ax(a);
		const uint8_t ct = c.refs[(size_t)off];
		int64_t t;
		for (t = off - 1; t >= off0; --t)
			if (c.refs[(size_t)t] != ct) break;
		if (off - t > 1) ++R.cnt[MM2GB_ALN_N_HPC_MOVED];
		*r = ax(a) + 1 - (int)(off - t);
	} else {
		*r = ax(a) - (c.k >> 1);
		*q = ay(a) - (c.k >> 1);
	}
}

inline AlRun make_run(const AlCtx &c, const Read &R, int rid, int rev, int q0, int qlen, int t0, int tlen, int flip, int kind, int w, int zdrop, int end_bonus, int flag)
{
	AlRun x;
	memset(&x, 0, sizeof x);
	x.j.q_at = c.read_at[(size_t)R.id]; x.j.t_at = c.ref_at[(size_t)rid];
	x.j.qn = R.qlen; x.j.tn = (int32_t)(c.ref_at[(size_t)rid + 1] - c.ref_at[(size_t)rid]); x.j.q0 = q0; x.j.qlen = qlen; x.j.t0 = t0; x.j.tlen = tlen; x.j.rev = rev; x.j.flip = flip; x.j.kind = kind;
	x.w = w; x.zdrop = zdrop; x.end_bonus = end_bonus; x.flag = flag;      // twin = 0 by the memset
	return x;
}

// ---- the DP's splice bits of a trial (align.c:612-616): splice_flag holds MM_F_SPLICE_FOR and / or _REV, which swap on a reverse-strand chain ----
inline int splice_bits(const AlCtx &c, int64_t splice_flag, int rev)
{
	int x = 0;
	if (splice_flag & MM2GB_F_SPLICE_FOR) x |= rev ? MM2GB_KSW_SPLICE_REV : MM2GB_KSW_SPLICE_FOR;
	if (splice_flag & MM2GB_F_SPLICE_REV) x |= rev ? MM2GB_KSW_SPLICE_FOR : MM2GB_KSW_SPLICE_REV;
	if (c.opt.flag & MM2GB_F_SPLICE_FLANK) x |= MM2GB_KSW_SPLICE_FLANK;
	return x;
}
inline bool two_trials(const AlCtx &c) { return c.splice && (c.opt.flag & MM2GB_F_SPLICE_FOR) && (c.opt.flag & MM2GB_F_SPLICE_REV); }

// ---- the first half of mm_align1 (align.c:573-700 and the coordinates of 700-803): a chain's job list.  false: the chain has no anchors.
//      Spliced form: the plan reads anchors' positions and spans and the sequences alone (the seed flags the filters SET are read by the job
//      loop below, and both trials would set the same ones), so a chain is planned once and its jobs entered once per trial with that trial's
//      splice bits, the second copy marked as the first's twin ----
bool plan_chain(const AlCtx &c, Read &R, const Reg &g, Plan &P, std::vector<int> &K)
{
	const mm2gb_align_opt_t &o = c.opt;
	const mm2gb_reg_t &r = g.r;
	if (r.cnt == 0) return false;
	mm2gb_anchor_t *a = R.a.data();
	const int32_t rid = (int32_t)(a[r.as].x << 1 >> 33), rev = (int32_t)(a[r.as].x >> 63), ref_len = (int32_t)(c.ref_at[(size_t)rid + 1] - c.ref_at[(size_t)rid]), qlen = R.qlen;
	int32_t as1, cnt1, rs, qs, re, qe, rs0, qs0, re0, qe0, rs1, qs1, re1, qe1, i, l;
	if (o.flag & MM2GB_F_NO_END_FLT) { as1 = r.as; cnt1 = r.cnt; }
	else if (c.splice) fix_bad_ends_splice(c, R, r, a, &as1, &cnt1);
	else fix_bad_ends(r, a, o.bw, o.min_chain_score * 2, &as1, &cnt1);
	filter_bad_seeds(as1, cnt1, a, 10, 40, o.max_gap >> 1, 10, K);
	filter_bad_seeds_alt(as1, cnt1, a, 30, o.max_gap >> 1, K);
	adjust_minier(c, R, a[as1], &rs, &qs);
	adjust_minier(c, R, a[as1 + cnt1 - 1], &re, &qe);
	// the region's bounds
	rs0 = ax(a[r.as]) + 1 - aspan(a[r.as]);
	qs0 = ay(a[r.as]) + 1 - aspan(a[r.as]);
	if (rs0 < 0) rs0 = 0;
	rs1 = qs1 = 0;
	for (i = r.as - 1, l = 0; i >= 0 && a[i].x >> 32 == a[r.as].x >> 32; --i) {
		const int32_t x = ax(a[i]) + 1 - aspan(a[i]), y = ay(a[i]) + 1 - aspan(a[i]);
		if (x < rs0 && y < qs0) {
			if (++l > o.min_cnt) {
				l = rs0 - x > qs0 - y ? rs0 - x : qs0 - y;
				rs1 = rs0 - l; qs1 = qs0 - l;
				if (rs1 < 0) rs1 = 0;
				break;
			}
		}
	}
	if (qs > 0 && rs > 0) {
		l = qs < o.max_gap ? qs : o.max_gap;
		qs1 = qs1 > qs - l ? qs1 : qs - l;
		qs0 = qs0 < qs1 ? qs0 : qs1;
		l += l * o.a > o.q ? (l * o.a - o.q) / o.e : 0;
		l = l < o.max_gap ? l : o.max_gap;
		l = l < rs ? l : rs;
		rs1 = rs1 > rs - l ? rs1 : rs - l;
		rs0 = rs0 < rs1 ? rs0 : rs1;
		rs0 = rs0 < rs ? rs0 : rs;
	} else { rs0 = rs; qs0 = qs; }
	re0 = ax(a[r.as + r.cnt - 1]) + 1;
	qe0 = ay(a[r.as + r.cnt - 1]) + 1;
	re1 = ref_len; qe1 = qlen;
	for (i = r.as + r.cnt, l = 0; i < R.n_a && a[i].x >> 32 == a[r.as].x >> 32; ++i) {
		const int32_t x = ax(a[i]) + 1, y = ay(a[i]) + 1;
		if (x > re0 && y > qe0) {
			if (++l > o.min_cnt) {
				l = x - re0 > y - qe0 ? x - re0 : y - qe0;
				re1 = re0 + l; qe1 = qe0 + l;
				break;
			}
		}
	}
	if (qe < qlen && re < ref_len) {
		l = qlen - qe < o.max_gap ? qlen - qe : o.max_gap;
		qe1 = qe1 < qe + l ? qe1 : qe + l;
		qe0 = qe0 > qe1 ? qe0 : qe1;
		l += l * o.a > o.q ? (l * o.a - o.q) / o.e : 0;
		l = l < o.max_gap ? l : o.max_gap;
		l = l < ref_len - re ? l : ref_len - re;
		re1 = re1 < re + l ? re1 : re + l;
		re0 = re0 > re1 ? re0 : re1;
	} else { re0 = re; qe0 = qe; }
	if (a[r.as].y & SEED_SELF) {
		int max_ext = r.qs > r.rs ? r.qs - r.rs : r.rs - r.qs;
		if (r.rs - rs0 > max_ext) rs0 = r.rs - max_ext;
		if (r.qs - qs0 > max_ext) qs0 = r.qs - max_ext;
		max_ext = r.qe > r.re ? r.qe - r.re : r.re - r.qe;
		if (re0 - r.re > max_ext) re0 = r.re + max_ext;
		if (qe0 - r.qe > max_ext) qe0 = r.qe + max_ext;
	}
	P.as1 = as1; P.cnt1 = cnt1; P.rid = rid; P.rev = rev; P.rs = rs; P.qs = qs; P.re = re; P.qe = qe; P.rs0 = rs0; P.qs0 = qs0; P.re0 = re0; P.qe0 = qe0;
	P.left = P.right = -1;
	P.fills.clear();
	if (rev) { ++R.cnt[MM2GB_ALN_N_REV_CHAIN]; ++R.scnt[MM2GB_SPL_N_REV_CHAIN]; }
	// the jobs
	const int first = (int)R.runs.size();
	if (qs > 0 && rs > 0) {
		P.left = (int)R.runs.size();
		if (rs0 == 0) ++R.cnt[MM2GB_ALN_N_LEFT_AT_0];
		R.runs.push_back(make_run(c, R, rid, rev, qs0, qs - qs0, rs0, rs - rs0, 1, 0, c.bw, (g.r.flags & RF_SPLIT_INV) ? o.zdrop_inv : o.zdrop, o.end_bonus,
		                          MM2GB_KSW_EXTZ_ONLY | MM2GB_KSW_RIGHT | MM2GB_KSW_REV_CIGAR));
	}
	for (i = 1; i < cnt1; ++i) {
		if ((a[as1 + i].y & (SEED_IGNORE | SEED_TANDEM)) && i != cnt1 - 1) continue;
		adjust_minier(c, R, a[as1 + i], &re, &qe);
		if (i == cnt1 - 1 || (a[as1 + i].y & SEED_LONG_JOIN) || (qe - qs >= o.min_ksw_len && re - rs >= o.min_ksw_len)) {
			int bw1 = c.bw_long;
			if (a[as1 + i].y & SEED_LONG_JOIN) bw1 = qe - qs > re - rs ? qe - qs : re - rs;
			P.fills.push_back({ rs, qs, re, qe, i, (int)R.runs.size() });
			R.runs.push_back(make_run(c, R, rid, rev, qs, qe - qs, rs, re - rs, 0, 1, bw1, o.zdrop, -1, MM2GB_KSW_APPROX_MAX));
			rs = re; qs = qe;
		} else ++R.cnt[MM2GB_ALN_N_GAP_SKIPPED];
	}
	if (qe < qe0 && re < re0) {
		P.right = (int)R.runs.size();
		R.runs.push_back(make_run(c, R, rid, rev, qe, qe0 - qe, re, re0 - re, 0, 2, c.bw, o.zdrop, o.end_bonus, MM2GB_KSW_EXTZ_ONLY));
	}
	P.n_runs = (int)R.runs.size() - first; P.trials = 1;
	if (c.splice) {
		P.trials = two_trials(c) ? 2 : 1;
		if (P.trials == 1) ++R.scnt[MM2GB_SPL_N_SINGLE_TRIAL];
		const int bits0 = splice_bits(c, P.trials == 2 ? MM2GB_F_SPLICE_FOR : o.flag, rev), bits1 = splice_bits(c, MM2GB_F_SPLICE_REV, rev);
		for (int k = 0; k < P.n_runs; ++k) {
			if (P.trials == 2) { AlRun x = R.runs[(size_t)(first + k)]; x.flag |= bits1; x.twin = P.n_runs; R.runs.push_back(x); }      // lands at first + n_runs + k
			R.runs[(size_t)(first + k)].flag |= bits0;
		}
	}
	return true;
}

// ---- mm_max_stretch (align.c:498-524): the run of anchors on one diagonal with the largest sum of matching bases ----
void max_stretch(const mm2gb_reg_t &r, const mm2gb_anchor_t *a, int32_t *as, int32_t *cnt)
{
	*as = r.as; *cnt = r.cnt;
	if (r.cnt < 2) return;
	int32_t i, max_score = -1, max_i = -1, max_len = 0, score = aspan(a[r.as]), len = 1;
	for (i = r.as + 1; i < r.as + r.cnt; ++i) {
		const int32_t q_span = aspan(a[i]), lr = ax(a[i]) - ax(a[i - 1]), lq = ay(a[i]) - ay(a[i - 1]);
		if (lq == lr) { score += lq < q_span ? lq : q_span; ++len; }
		else {
			if (score > max_score) { max_score = score; max_len = len; max_i = i - len; }
			score = q_span; len = 1;
		}
	}
	if (score > max_score) { max_len = len; max_i = i - len; }
	*as = max_i; *cnt = max_len;
}

// ---- plan_chain under MM_F_SR (the is_sr branches of align.c:592-597, 623-630, 724-731): the stretch, the whole read as the query's bounds, the target's from what
//      end_bonus lets an extension pay for, and ONE fill over the stretch, marked ungapped: its first pass is not a DP (the backends) ----
bool plan_chain_sr(const AlCtx &c, Read &R, const Reg &g, Plan &P)
{
	const mm2gb_align_opt_t &o = c.opt;
	const mm2gb_reg_t &r = g.r;
	if (r.cnt == 0) return false;
	const mm2gb_anchor_t *a = R.a.data();
	const int32_t rid = (int32_t)(a[r.as].x << 1 >> 33), rev = (int32_t)(a[r.as].x >> 63), ref_len = (int32_t)(c.ref_at[(size_t)rid + 1] - c.ref_at[(size_t)rid]), qlen = R.qlen;
	int32_t as1, cnt1, l;
	max_stretch(r, a, &as1, &cnt1);
	if (cnt1 < r.cnt) ++R.srcnt[MM2GB_SR_N_STRETCH_SHORT];
	const int32_t rs = ax(a[as1]) + 1 - aspan(a[as1]), qs = ay(a[as1]) + 1 - aspan(a[as1]), re = ax(a[as1 + cnt1 - 1]) + 1, qe = ay(a[as1 + cnt1 - 1]) + 1;
	int32_t rs0, re0, qs0 = 0, qe0 = qlen;
	l = qs;
	l += l * o.a + o.end_bonus > o.q ? (l * o.a + o.end_bonus - o.q) / o.e : 0;
	rs0 = rs - l > 0 ? rs - l : 0;
	l = qlen - qe;
	l += l * o.a + o.end_bonus > o.q ? (l * o.a + o.end_bonus - o.q) / o.e : 0;
	re0 = re + l < ref_len ? re + l : ref_len;
	if (a[r.as].y & SEED_SELF) {
		int max_ext = r.qs > r.rs ? r.qs - r.rs : r.rs - r.qs;
		if (r.rs - rs0 > max_ext) rs0 = r.rs - max_ext;
		if (r.qs - qs0 > max_ext) qs0 = r.qs - max_ext;
		max_ext = r.qe > r.re ? r.qe - r.re : r.re - r.qe;
		if (re0 - r.re > max_ext) re0 = r.re + max_ext;
		if (qe0 - r.qe > max_ext) qe0 = r.qe + max_ext;
	}
	P.as1 = as1; P.cnt1 = cnt1; P.rid = rid; P.rev = rev; P.rs = rs; P.qs = qs; P.re = re; P.qe = qe; P.rs0 = rs0; P.qs0 = qs0; P.re0 = re0; P.qe0 = qe0;
	P.left = P.right = -1;
	P.fills.clear();
	if (rev) ++R.cnt[MM2GB_ALN_N_REV_CHAIN];
	const int first = (int)R.runs.size();
	if (qs > 0 && rs > 0) {
		P.left = (int)R.runs.size();
		if (rs0 == 0) ++R.cnt[MM2GB_ALN_N_LEFT_AT_0];
		R.runs.push_back(make_run(c, R, rid, rev, qs0, qs - qs0, rs0, rs - rs0, 1, 0, c.bw, (g.r.flags & RF_SPLIT_INV) ? o.zdrop_inv : o.zdrop, o.end_bonus,
		                          MM2GB_KSW_EXTZ_ONLY | MM2GB_KSW_RIGHT | MM2GB_KSW_REV_CIGAR));
	}
	{
		int bw1 = c.bw_long;
		if (a[as1 + cnt1 - 1].y & SEED_LONG_JOIN) bw1 = qe - qs > re - rs ? qe - qs : re - rs;
		P.fills.push_back({ rs, qs, re, qe, cnt1 - 1, (int)R.runs.size() });
		R.runs.push_back(make_run(c, R, rid, rev, qs, qe - qs, rs, re - rs, 0, 1, bw1, o.zdrop, -1, MM2GB_KSW_APPROX_MAX));      // (the flag is the second pass's, less al_second_flag's bit)
		R.runs.back().ungapped = 1;
	}
	if (qe < qe0 && re < re0) {
		P.right = (int)R.runs.size();
		R.runs.push_back(make_run(c, R, rid, rev, qe, qe0 - qe, re, re0 - re, 0, 2, c.bw, o.zdrop, o.end_bonus, MM2GB_KSW_EXTZ_ONLY));
	}
	P.n_runs = (int)R.runs.size() - first; P.trials = 1;
	return true;
}

// ---- mg_log2 (mmpriv.h:118-126) ----
inline float mg_log2(float x)
{
	union { float f; uint32_t i; } z = { x };
	float log_2 = (float)(((z.i >> 23) & 255) - 128);
	z.i &= ~(255u << 23);
	z.i += 127u << 23;
	log_2 += (-0.34484843f * z.f + 2.02466578f) * z.f - 0.67487759f;
	return log_2;
}

// ---- mm_fix_cigar (align.c:91-167) on a record's words; Q / T: residues from the alignment's start ----
template <class FQ, class FT>
void fix_cigar(Read &R, Reg &g, FQ Q, FT T, int *qshift, int *tshift)
{
	std::vector<uint32_t> &cg = g.cig;
	mm2gb_reg_t &r = g.r;
	int32_t toff = 0, qoff = 0, to_shrink = 0;
	uint32_t k, n_cigar = (uint32_t)cg.size();
	*qshift = *tshift = 0;
	if (n_cigar <= 1) return;
	for (k = 0; k < n_cigar; ++k) {
		const uint32_t op = cg[k] & 0xf, len = cg[k] >> 4;
		if (len == 0) to_shrink = 1;
		if (op == 0) { toff += len; qoff += len; }
		else if (op == 1 || op == 2) {
			if (k > 0 && k < n_cigar - 1 && (cg[k - 1] & 0xf) == 0 && (cg[k + 1] & 0xf) == 0) {
				int l;
				const int prev_len = (int)(cg[k - 1] >> 4);
				if (op == 1) { for (l = 0; l < prev_len; ++l) if (Q(qoff - 1 - l) != Q(qoff + (int)len - 1 - l)) break; }
				else         { for (l = 0; l < prev_len; ++l) if (T(toff - 1 - l) != T(toff + (int)len - 1 - l)) break; }
				if (l > 0) { cg[k - 1] -= (uint32_t)l << 4; cg[k + 1] += (uint32_t)l << 4; qoff -= l; toff -= l; }
				if (l == prev_len) to_shrink = 1;
			}
			if (op == 1) qoff += len; else toff += len;
		} else if (op == 3) toff += len;
	}
	for (k = 0; k < n_cigar - 2; ++k) {
		if ((cg[k] & 0xf) > 0 && (cg[k] & 0xf) + (cg[k + 1] & 0xf) == 3) {
			uint32_t l, s[3] = { 0, 0, 0 };
			for (l = k; l < n_cigar; ++l) {
				const uint32_t op = cg[l] & 0xf;
				if (op == 1 || op == 2 || cg[l] >> 4 == 0) s[op] += cg[l] >> 4;
				else break;
			}
			if (s[1] > 0 && s[2] > 0 && l - k > 2) {
				cg[k] = s[1] << 4 | 1;
				cg[k + 1] = s[2] << 4 | 2;
				for (k += 2; k < l; ++k) cg[k] &= 0xf;
				to_shrink = 1;
			}
			k = l;
		}
	}
	if (to_shrink) {
		uint32_t l = 0;
		for (k = 0; k < n_cigar; ++k) if (cg[k] >> 4 != 0) cg[l++] = cg[k];
		n_cigar = l;
		for (k = l = 0; k < n_cigar; ++k)
			if (k == n_cigar - 1 || (cg[k] & 0xf) != (cg[k + 1] & 0xf)) cg[l++] = cg[k];
			else cg[k + 1] += cg[k] >> 4 << 4;
		n_cigar = l;
	}
	if (n_cigar > 0 && ((cg[0] & 0xf) == 1 || (cg[0] & 0xf) == 2)) {
		const int32_t l = (int32_t)(cg[0] >> 4);
		if ((cg[0] & 0xf) == 1) {
			if (r.flags & RF_REV) r.qe -= l; else r.qs += l;
			*qshift = l;
		} else { r.rs += l; *tshift = l; }
		--n_cigar;
		memmove(cg.data(), cg.data() + 1, (size_t)n_cigar * 4);
		++R.cnt[MM2GB_ALN_N_LEAD_GAP_CUT];
	}
	cg.resize(n_cigar);
}

// ---- mm_update_extra (align.c:240-289), no =/X; log_gap off under MM_F_SR (align.c:819) ----
template <class FQ, class FT>
void update_extra(const AlCtx &c, Read &R, Reg &g, FQ Q0, FT T0)
{
	if (!g.has_p) return;
	int qshift, tshift, toff = 0, qoff = 0;
	double s = 0.0, max = 0.0;
	fix_cigar(R, g, Q0, T0, &qshift, &tshift);
	auto Q = [&](int k) { return Q0(k + qshift); };
	auto T = [&](int k) { return T0(k + tshift); };
	mm2gb_reg_t &r = g.r;
	const int8_t q = (int8_t)c.opt.q, e = (int8_t)c.opt.e;
	r.blen = r.mlen = 0;
	for (uint32_t w : g.cig) {
		const uint32_t op = w & 0xf;
		const int len = (int)(w >> 4);
		if (op == 0) {
			int n_ambi = 0, n_diff = 0;
			for (int l = 0; l < len; ++l) {
				const int cq = Q(qoff + l), ct = T(toff + l);
				if (ct > 3 || cq > 3) ++n_ambi;
				else if (ct != cq) ++n_diff;
				s += c.mat[ct * 5 + cq];
				if (s < 0) s = 0;
				else max = max > s ? max : s;
			}
			r.blen += len - n_ambi; r.mlen += len - (n_ambi + n_diff); g.n_ambi += n_ambi;
			toff += len; qoff += len;
		} else if (op == 1 || op == 2) {
			int n_ambi = 0;
			for (int l = 0; l < len; ++l)
				if ((op == 1 ? Q(qoff + l) : T(toff + l)) > 3) ++n_ambi;
			r.blen += len - n_ambi; g.n_ambi += n_ambi;
			if (c.sr) s -= q + e;
			else s -= q + (double)e * mg_log2((float)(1.0 + len));
			if (s < 0) s = 0;
			if (op == 1) qoff += len; else toff += len;
		} else if (op == 3) toff += len;
	}
	g.dp_max = (int32_t)(max + .499);
}

// ---- ksw_ll_i16 (ksw2_ll_sse.c:85-152) with ksw_ll_qinit's 16-bit profile, lane by lane: eight interleaved stripes of the query padded to a
//      multiple of eight (a padded position scores 0 and can carry the maximum on, so it takes part), E taken from H before the lazy pass
//      over F, that pass ended when no lane's F beats H - (o + e), and the reference's ties: the LAST target row and the LAST stripe position
//      holding the maximum.  The 16-bit saturation cannot bite: a stretch is shorter than max_gap = 5000 bases at 2 a base.  Returns the score ----
int ll_i16(const AlCtx &c, int qlen, const uint8_t *query, int tlen, const uint8_t *target, int gapo, int gape, int *qe, int *te)
{
	*qe = *te = -1;
	const int slen = (qlen + 7) / 8, n = slen * 8, gapoe = gapo + gape;
	if (slen == 0) { if (tlen > 0) *te = tlen - 1; return 0; }
	std::vector<int32_t> prof((size_t)5 * n), Hbuf((size_t)4 * n, 0);
	for (int a = 0; a < 5; ++a)
		for (int j = 0; j < slen; ++j)
			for (int k = 0; k < 8; ++k) { const int p = j + k * slen; prof[(size_t)a * n + j * 8 + k] = p >= qlen ? 0 : c.mat[a * 5 + query[p]]; }
	int32_t *H0 = Hbuf.data(), *H1 = H0 + n, *E = H1 + n, *Hmax = E + n;
	int gmax = 0;
	for (int i = 0; i < tlen; ++i) {
		int32_t f[8] = {}, mx[8] = {}, h[8];
		const int32_t *S = prof.data() + (size_t)target[i] * n;
		for (int k = 0; k < 8; ++k) h[k] = k ? H0[(slen - 1) * 8 + k - 1] : 0;
		for (int j = 0; j < slen; ++j)
			for (int k = 0; k < 8; ++k) {
				int32_t hh = h[k] + S[j * 8 + k], e = E[j * 8 + k];
				hh = std::max(hh, e); hh = std::max(hh, f[k]);
				mx[k] = std::max(mx[k], hh);
				H1[j * 8 + k] = hh;
				hh = std::max(0, hh - gapoe);
				e = std::max(std::max(0, e - gape), hh);
				E[j * 8 + k] = e;
				f[k] = std::max(std::max(0, f[k] - gape), hh);
				h[k] = H0[j * 8 + k];
			}
		bool done = false;
		for (int kk = 0; kk < 8 && !done; ++kk) {
			for (int k = 7; k > 0; --k) f[k] = f[k - 1];
			f[0] = 0;
			for (int j = 0; j < slen; ++j) {
				bool any = false;
				for (int k = 0; k < 8; ++k) {
					int32_t hh = std::max(H1[j * 8 + k], f[k]);
					H1[j * 8 + k] = hh;
					hh = std::max(0, hh - gapoe);
					f[k] = std::max(0, f[k] - gape);
					any |= f[k] > hh;
				}
				if (!any) { done = true; break; }
			}
		}
		int imax = 0;
		for (int k = 0; k < 8; ++k) imax = std::max(imax, mx[k]);
		if (imax >= gmax) { gmax = imax; *te = i; memcpy(Hmax, H1, (size_t)n * 4); }
		std::swap(H0, H1);
	}
	for (int i = 0; i < n; ++i)
		if (Hmax[i] == gmax) *qe = i / 8 + i % 8 * slen;
	return gmax;
}

// ---- mm_align1_inv's tests and probe (align.c:828-859): true with the alignment's job in `out` ----
bool inv_prepare(const AlCtx &c, Read &R, const mm2gb_reg_t &r1, const mm2gb_reg_t &r2, Reg &out)
{
	const mm2gb_align_opt_t &o = c.opt;
	if (!(r1.flags & RF_SPLIT1) || !(r2.flags & RF_SPLIT2)) return false;
	if (r1.id != r1.parent && r1.parent != PARENT_TMP_PRI) return false;
	if (r2.id != r2.parent && r2.parent != PARENT_TMP_PRI) return false;
	const int rev1 = (r1.flags & RF_REV) != 0, rev2 = (r2.flags & RF_REV) != 0;
	if (r1.rid != r2.rid || rev1 != rev2) return false;
	const int ql = rev1 ? r1.qs - r2.qe : r2.qs - r1.qe, tl = r2.rs - r1.re;
	if (ql < o.min_chain_score || ql > o.max_gap) return false;
	if (tl < o.min_chain_score || tl > o.max_gap) return false;
	const int strand = rev1 ? 0 : 1, base = rev1 ? r2.qe : R.qlen - r2.qs;
	AlRun probe = make_run(c, R, r1.rid, strand, base, ql, r1.re, tl, 1, 3, 0, 0, 0, 0);
	std::vector<uint8_t> qs((size_t)ql), ts((size_t)tl);
	for (int k = 0; k < ql; ++k) qs[(size_t)k] = al_query(c.reads.data(), probe.j, k);
	for (int k = 0; k < tl; ++k) ts[(size_t)k] = al_target(c.refs.data(), probe.j, k);
	int q_off, t_off;
	const int score = ll_i16(c, ql, qs.data(), tl, ts.data(), o.q, o.e, &q_off, &t_off);
	if (score < o.min_dp_max) return false;
	q_off = ql - (q_off + 1); t_off = tl - (t_off + 1);
	out = Reg();
	memset(&out.r, 0, sizeof out.r);
	out.inv = make_run(c, R, r1.rid, strand, base + q_off, ql - q_off, r1.re + t_off, tl - t_off, 0, 3, (int)(o.bw * 1.5), o.zdrop, -1, MM2GB_KSW_EXTZ_ONLY);
	out.r.id = -1; out.r.parent = PARENT_UNSET; out.r.rid = r1.rid; out.r.div = -1.0f;
	out.r.flags = RF_INV | (rev1 ? 0 : RF_REV);
	out.inv_q = rev1 ? r2.qe + q_off : r2.qs - q_off;       // r_inv->rev == 0 <=> r1->rev
	out.r.rs = r1.re + t_off;
	out.state = ST_INV_FRESH;
	return true;
}

void append_cigar(Read &R, Reg &g, const AlRun &x, const uint32_t *pool)
{
	const int n = x.res.n_cigar;
	if (n <= 0) return;
	const uint32_t *w = pool + x.res.cigar_off;
	g.has_p = true;
	if (!g.cig.empty() && (g.cig.back() & 0xf) == (w[0] & 0xf)) {
		g.cig.back() += w[0] >> 4 << 4;
		g.cig.insert(g.cig.end(), w + 1, w + n);
		++R.cnt[MM2GB_ALN_N_SEAM_MERGED];
		if ((w[0] & 0xf) == 3) ++R.scnt[MM2GB_SPL_N_N_SEAM_MERGED];
	} else g.cig.insert(g.cig.end(), w, w + n);
}

inline int64_t run_cells(const AlRun &x) { return (int64_t)std::max(x.j.qlen, 0) * std::max(x.j.tlen, 0) * (x.code ? 2 : 1); }

inline bool has_intron(const AlRun &x, const uint32_t *pool)
{
	for (int k = 0; k < x.res.n_cigar; ++k) if ((pool[x.res.cigar_off + k] & 0xf) == 3) return true;
	return false;
}

// the N words of a finished record whose ends on the target are neither GT..AG nor CT..AC (information: MM2GB_SPL_N_NONCANONICAL_INTRON)
template <class FT>
int count_noncanonical(const Reg &g, FT T)
{
	int n = 0, toff = 0;
	for (uint32_t w : g.cig) {
		const int op = (int)(w & 0xf), len = (int)(w >> 4);
		if (op == 3 && len >= 4) {
			const int d0 = T(toff), d1 = T(toff + 1), a0 = T(toff + len - 2), a1 = T(toff + len - 1);
			if (!((d0 == 2 && d1 == 3 && a0 == 0 && a1 == 2) || (d0 == 1 && d1 == 3 && a0 == 0 && a1 == 1))) ++n;
		}
		if (op == 0 || op == 2 || op == 3) toff += len;
	}
	return n;
}

// ---- the second half of mm_align1 (align.c:712-822): a chain's results stitched into its record; true: tail holds what a z-drop split off.
//      ru: the jobs of the trial that is stitched (the plan's indices count from there) ----
bool stitch_chain(const AlCtx &c, Read &R, Reg &g, const Plan &P, const AlRun *ru, const uint32_t *pool, Reg &tail)
{
	const mm2gb_align_opt_t &o = c.opt;
	const mm2gb_anchor_t *a = R.a.data();
	int32_t rs1, qs1, re1, qe1;
	bool dropped = false, split = false;
	if (P.left >= 0) {
		const AlRun &x = ru[P.left];
		if (x.res.n_cigar > 0) { append_cigar(R, g, x, pool); g.dp_score += x.res.max; }
		rs1 = P.rs - (x.res.reach_end ? x.res.mqe_t + 1 : x.res.max_t + 1);
		qs1 = P.qs - (x.res.reach_end ? P.qs - P.qs0 : x.res.max_q + 1);
		++R.cnt[x.res.reach_end ? MM2GB_ALN_N_LEFT_END : MM2GB_ALN_N_LEFT_SHORT];
		if (c.splice && has_intron(x, pool)) ++R.scnt[MM2GB_SPL_N_LEFT_EXT_INTRON];
	} else { rs1 = P.rs; qs1 = P.qs; }
	re1 = P.rs; qe1 = P.qs;
	size_t used = 0;
	for (const Fill &f : P.fills) {
		const AlRun &x = ru[f.run];
		++used;
		re1 = f.re; qe1 = f.qe;
		++R.cnt[x.code ? MM2GB_ALN_N_FILL_TWO_PASS : MM2GB_ALN_N_FILL_ONE_PASS];
		if (x.ungapped) ++R.srcnt[x.code ? MM2GB_SR_N_FILL_RERUN : MM2GB_SR_N_FILL_UNGAPPED];
		if (x.code == 2) ++R.cnt[MM2GB_ALN_N_INV_PROBE_HIT];
		if (al_too_big(c, x.j) && (!x.ungapped || x.code)) { ++R.cnt[MM2GB_ALN_N_OVER_SW_MAT]; ++R.scnt[MM2GB_SPL_N_OVER_SW_MAT]; }
		if (c.splice) { if (x.code) ++R.scnt[MM2GB_SPL_N_FILL_TWO_PASS]; if (has_intron(x, pool)) ++R.scnt[MM2GB_SPL_N_FILL_INTRON]; }
		append_cigar(R, g, x, pool);
		if (x.res.zdropped) {
			int j;
			g.has_p = true;
			for (j = f.i - 1; j >= 0; --j)
				if (ax(a[P.as1 + j]) <= f.rs + x.res.max_t) break;
			dropped = true;
			if (j < 0) j = 0;
			g.dp_score += x.res.max;
			re1 = f.rs + (x.res.max_t + 1);
			qe1 = f.qs + (x.res.max_q + 1);
			if (P.cnt1 - (j + 1) >= o.min_cnt && split_reg(g.r, tail.r, P.as1 + j + 1 - g.r.as, R.qlen, a)) {
				split = true;
				if (x.code == 2) tail.r.flags |= RF_SPLIT_INV;
				++R.cnt[MM2GB_ALN_N_SPLIT]; ++R.scnt[MM2GB_SPL_N_SPLIT];
			} else ++R.cnt[MM2GB_ALN_N_SPLIT_REFUSED];
			break;
		} else g.dp_score += x.res.score;
	}
	if (!dropped && P.right >= 0) {
		const AlRun &x = ru[P.right];
		if (x.res.n_cigar > 0) { append_cigar(R, g, x, pool); g.dp_score += x.res.max; }
		re1 = P.re + (x.res.reach_end ? x.res.mqe_t + 1 : x.res.max_t + 1);
		qe1 = P.qe + (x.res.reach_end ? P.qe0 - P.qe : x.res.max_q + 1);
		++R.cnt[x.res.reach_end ? MM2GB_ALN_N_RIGHT_END : MM2GB_ALN_N_RIGHT_SHORT];
		if (c.splice && has_intron(x, pool)) ++R.scnt[MM2GB_SPL_N_RIGHT_EXT_INTRON];
	}
	if (dropped) {            // what ran behind the drop was speculation
		for (size_t k = used; k < P.fills.size(); ++k) R.cnt[MM2GB_ALN_N_CELLS_DISCARDED] += run_cells(ru[P.fills[k].run]);
		if (P.right >= 0) R.cnt[MM2GB_ALN_N_CELLS_DISCARDED] += run_cells(ru[P.right]);
	}
	g.r.rs = rs1; g.r.re = re1;
	if (!P.rev) { g.r.qs = qs1; g.r.qe = qe1; }
	else { g.r.qs = R.qlen - qe1; g.r.qe = R.qlen - qs1; }
	if (g.has_p) {
		const int strand = (g.r.flags & RF_REV) != 0;
		const int64_t t_at = c.ref_at[(size_t)P.rid];
		update_extra(c, R, g, [&](int k) { return (int)read_base(c, R.id, strand, qs1 + k); }, [&](int k) { return (int)c.refs[(size_t)(t_at + rs1 + k)]; });
		if (c.splice) R.scnt[MM2GB_SPL_N_NONCANONICAL_INTRON] += count_noncanonical(g, [&](int k) { return (int)c.refs[(size_t)(t_at + g.r.rs + k)]; });
	}
	return split;
}

// ---- a chain of the spliced form (align.c:980-1001): one trial, or both stitched from the same input record and the larger dp_score kept
//      (a tie: trial (qlen + dp_score) & 1); the loser's record, tail and counts are dropped.  trans_strand is set HERE, after mm_align1: the
//      flip to the read's strand at align.c:820-821 tests a field that is still 0 and never fires, and so a reverse-strand chain keeps 1 / 2
//      as the trial says.  The cells behind a drop in the trial dropped count as discarded too ----
bool stitch_trials(const AlCtx &c, Read &R, Reg &g, const Plan &P, const AlRun *ru, const uint32_t *pool, Reg &tail)
{
	if (P.trials == 1) {
		const bool split = stitch_chain(c, R, g, P, ru, pool, tail);
		g.trans_strand = (c.opt.flag & MM2GB_F_SPLICE_FOR) ? 1 : 2;
		return split;
	}
	Reg s[2] = { g, g }, s2[2];
	bool split[2];
	int64_t cnt0[MM2GB_ALN_N_COUNTS], scnt0[MM2GB_SPL_N_COUNTS], cnt[2][MM2GB_ALN_N_COUNTS], scnt[2][MM2GB_SPL_N_COUNTS];
	memcpy(cnt0, R.cnt, sizeof cnt0); memcpy(scnt0, R.scnt, sizeof scnt0);
	for (int t = 0; t < 2; ++t) {
		memcpy(R.cnt, cnt0, sizeof cnt0); memcpy(R.scnt, scnt0, sizeof scnt0);
		split[t] = stitch_chain(c, R, s[t], P, ru + (size_t)t * P.n_runs, pool, s2[t]);
		memcpy(cnt[t], R.cnt, sizeof cnt0); memcpy(scnt[t], R.scnt, sizeof scnt0);
	}
	int which, trans_strand;
	if (s[0].dp_score > s[1].dp_score) { which = 0; trans_strand = 1; }
	else if (s[0].dp_score < s[1].dp_score) { which = 1; trans_strand = 2; }
	else { trans_strand = 3; which = (R.qlen + s[0].dp_score) & 1; }
	memcpy(R.cnt, cnt[which], sizeof cnt0); memcpy(R.scnt, scnt[which], sizeof scnt0);
	R.cnt[MM2GB_ALN_N_CELLS_DISCARDED] += cnt[!which][MM2GB_ALN_N_CELLS_DISCARDED] - cnt0[MM2GB_ALN_N_CELLS_DISCARDED];
	++R.scnt[trans_strand == 1 ? MM2GB_SPL_N_TRIAL_FOR_WON : trans_strand == 2 ? MM2GB_SPL_N_TRIAL_REV_WON : which ? MM2GB_SPL_N_TRIAL_TIE_KEPT_1 : MM2GB_SPL_N_TRIAL_TIE_KEPT_0];
	g = std::move(s[which]);
	g.trans_strand = trans_strand;
	if (split[which]) tail = std::move(s2[which]);
	return split[which];
}

// ---- mm_align1_inv's end (align.c:860-879): false: no words came back, the record is dropped ----
bool finish_inv(const AlCtx &c, Read &R, Reg &g, const AlRun &x, const uint32_t *pool)
{
	if (x.res.n_cigar == 0) return false;
	append_cigar(R, g, x, pool);
	g.dp_score = x.res.max;
	if (!(g.r.flags & RF_REV)) { g.r.qs = g.inv_q; g.r.qe = g.r.qs + x.res.max_q + 1; }
	else { g.r.qe = g.inv_q; g.r.qs = g.r.qe - (x.res.max_q + 1); }
	g.r.re = g.r.rs + x.res.max_t + 1;
	const AlJob j = x.j;
	update_extra(c, R, g, [&](int k) { return (int)al_query(c.reads.data(), j, k); }, [&](int k) { return (int)al_target(c.refs.data(), j, k); });
	++R.cnt[MM2GB_ALN_N_INV];
	return true;
}

// ---- mm_squeeze_a (hit.c:311-329) ----
void squeeze_a(Read &R)
{
	std::vector<uint64_t> aux(R.regs.size());
	for (size_t i = 0; i < R.regs.size(); ++i) aux[i] = (uint64_t)(uint32_t)R.regs[i].r.as << 32 | i;
	std::sort(aux.begin(), aux.end());
	int as = 0;
	for (uint64_t v : aux) {
		mm2gb_reg_t &r = R.regs[(size_t)(uint32_t)v].r;
		if (r.as != as) { memmove(&R.a[(size_t)as], &R.a[(size_t)r.as], (size_t)r.cnt * 16); r.as = as; }
		as += r.cnt;
	}
	R.n_a = as;
}

// ---- mm_filter_regs (hit.c:290-309) ----
void filter_regs(const AlCtx &c, Read &R)
{
	const mm2gb_align_opt_t &o = c.opt;
	size_t k = 0;
	for (size_t i = 0; i < R.regs.size(); ++i) {
		Reg &g = R.regs[i];
		int flt = 0;
		if (!(g.r.flags & RF_INV) && !(g.r.flags & RF_SEG_SPLIT) && g.r.cnt < o.min_cnt) flt = 1;
		if (g.has_p) {
			if (g.r.mlen < o.min_chain_score) flt = 1;
			else if (g.dp_max < o.min_dp_max) flt = 1;
			else if (g.r.qs > R.qlen * o.max_clip_ratio && R.qlen - g.r.qe > R.qlen * o.max_clip_ratio) flt = 1;
		}
		if (!flt) { if (k < i) R.regs[k] = std::move(g); ++k; }
		else ++R.cnt[MM2GB_ALN_N_FILTERED];
	}
	R.regs.resize(k);
}

// ---- mm_update_dp_max with mm_event_identity and mm_recal_max_dp (align.c:895-958) ----
void update_dp_max(const AlCtx &c, Read &R)
{
	const float frac = c.opt.rank_frac;
	const int n_regs = (int)R.regs.size(), a = c.opt.a, b = c.opt.b;
	int32_t max = -1, max2 = -1, max_i = -1;
	if (n_regs < 2) return;
	for (int i = 0; i < n_regs; ++i) {
		const Reg &g = R.regs[(size_t)i];
		if (!g.has_p) continue;
		if (g.dp_max > max) { max2 = max; max = g.dp_max; max_i = i; }
		else if (g.dp_max > max2) max2 = g.dp_max;
	}
	if (max_i < 0 || max < 0 || max2 < 0) return;
	const Reg &top = R.regs[(size_t)max_i];
	if (top.r.qe - top.r.qs < (double)R.qlen * frac) return;
	if (max2 < (double)max * frac) return;
	auto gaps = [](const Reg &g, int32_t *n_gap, int32_t *n_gapo) {
		*n_gap = *n_gapo = 0;
		for (uint32_t w : g.cig) if ((w & 0xf) == 1 || (w & 0xf) == 2) { ++*n_gapo; *n_gap += (int32_t)(w >> 4); }
	};
	int32_t n_gap, n_gapo;
	gaps(top, &n_gap, &n_gapo);
	double div = 1. - (double)top.r.mlen / (top.r.blen + top.n_ambi - n_gap + n_gapo);
	if (div < 0.02) div = 0.02;
	double b2 = 0.5 / div;
	if (b2 * a < b) b2 = (double)a / b;
	for (Reg &g : R.regs) {
		if (!g.has_p) continue;
		double gap_cost = 0.0;
		n_gap = n_gapo = 0;
		for (uint32_t w : g.cig)
			if ((w & 0xf) == 1 || (w & 0xf) == 2) { gap_cost += b2 + (double)mg_log2((float)(1.0 + (int32_t)(w >> 4))); ++n_gapo; n_gap += (int32_t)(w >> 4); }
		const int32_t n_mis = g.r.blen + g.n_ambi - g.r.mlen - n_gap;
		g.dp_max = (int32_t)(a * (g.r.mlen - b2 * n_mis - gap_cost) + .499);
		if (g.dp_max < 0) g.dp_max = 0;
	}
	++R.cnt[MM2GB_ALN_N_DP_MAX_REWRITTEN];
}

// ---- mm_hit_sort (hit.c:188-218), no ALT contigs ----
void hit_sort(Read &R)
{
	const int n = (int)R.regs.size();
	if (n <= 1) return;
	std::vector<mm2gb_anchor_t> aux;
	for (int i = 0; i < n; ++i) {
		const Reg &g = R.regs[(size_t)i];
		if ((g.r.flags & RF_INV) || g.r.cnt > 0) {
			const int score = g.has_p ? g.dp_max : g.r.score;
			aux.push_back({ (uint64_t)score << 32 | g.r.hash, (uint64_t)i });
		}
	}
	sort_by_x_like_host(aux.data(), aux.data() + aux.size());
	std::vector<Reg> t;
	t.reserve(aux.size());
	for (size_t i = aux.size(); i-- > 0;) t.push_back(std::move(R.regs[(size_t)aux[i].y]));
	R.regs.swap(t);
}

// every read of `reads` through rounds of planning, DP and stitching; the per-read steps on nt threads
int drive(const AlCtx &c, std::vector<Read*> &reads, AlBackend &be, int nt, double *seconds)
{
	using clk = std::chrono::steady_clock;
	std::vector<AlRun> runs;
	std::vector<uint32_t> pool;
	for (;;) {
		auto t0 = clk::now();
		for_each_on_threads(reads.size(), nt, 1, [&](size_t k) {
			Read &R = *reads[k];
			std::vector<int> K;
			R.runs.clear(); R.plans.clear();
			for (Reg &g : R.regs) {
				if (g.state == ST_FRESH) {
					Plan P;
					if (c.sr ? plan_chain_sr(c, R, g, P) : plan_chain(c, R, g, P, K)) { g.plan = (int)R.plans.size(); R.plans.push_back(std::move(P)); g.state = ST_PENDING; }
					else g.state = ST_DONE;
				} else if (g.state == ST_INV_FRESH) { g.plan = (int)R.runs.size(); R.runs.push_back(g.inv); g.state = ST_INV_PENDING; }
			}
		});
		runs.clear();
		for (Read *R : reads) { R->first_run = (int64_t)runs.size(); runs.insert(runs.end(), R->runs.begin(), R->runs.end()); if (!R->runs.empty()) ++R->rounds; }
		if (seconds) seconds[1] += std::chrono::duration<double>(clk::now() - t0).count();
		if (runs.empty()) break;
		for (const AlRun &x : runs)           // nothing is read outside a sequence, on either side of the link
			if ((x.j.qlen > 0 && (x.j.q0 < 0 || x.j.q0 + x.j.qlen > x.j.qn)) || (x.j.tlen > 0 && (x.j.t0 < 0 || x.j.t0 + x.j.tlen > x.j.tn)))
				return fail("mm2gb_align_regs: a stretch leaves its sequence (anchors and sequences do not belong together)");
		for (const AlRun &x : runs)           // align.c:745 asserts it
			if (x.ungapped && (x.j.qlen != x.j.tlen || x.j.qlen < 0)) return fail("mm2gb_align_regs_sr: a stretch's two sides differ in length (anchors that do not lie on one diagonal in ascending order)");
		pool.clear();
		if (be.run(c, runs, pool)) return -1;
		t0 = clk::now();
		for_each_on_threads(reads.size(), nt, 1, [&](size_t k) {
			Read &R = *reads[k];
			if (R.runs.empty()) return;
			const AlRun *ru = runs.data() + R.first_run;
			for (size_t n = 0; n < R.runs.size(); ++n) { ++R.cnt[MM2GB_ALN_N_JOBS]; R.cnt[MM2GB_ALN_N_CELLS] += run_cells(ru[n]); }
			for (size_t i = 0; i < R.regs.size(); ++i) {
				if (R.regs[i].state == ST_PENDING) {
					Reg tail;
					const Plan &P = R.plans[(size_t)R.regs[i].plan];
					const bool split = c.splice ? stitch_trials(c, R, R.regs[i], P, ru, pool.data(), tail) : stitch_chain(c, R, R.regs[i], P, ru, pool.data(), tail);
					R.regs[i].state = ST_DONE;
					if (c.splice && i > 0 && (R.regs[i].r.flags & RF_SPLIT2) && R.regs[i].trans_strand != R.regs[i - 1].trans_strand) ++R.scnt[MM2GB_SPL_N_TAIL_OTHER_STRAND];
					if (split) R.regs.insert(R.regs.begin() + (ptrdiff_t)i + 1, std::move(tail));          // mm_insert_reg: next round's chain
					if (i > 0 && (R.regs[i].r.flags & RF_SPLIT_INV) && !(c.opt.flag & MM2GB_F_NO_INV)) {
						Reg inv;
						if (inv_prepare(c, R, R.regs[i - 1].r, R.regs[i].r, inv)) { R.regs.insert(R.regs.begin() + (ptrdiff_t)i + 1, std::move(inv)); ++i; }
					}
				} else if (R.regs[i].state == ST_INV_PENDING) {
					if (finish_inv(c, R, R.regs[i], ru[R.regs[i].plan], pool.data())) R.regs[i].state = ST_DONE;
					else { R.regs.erase(R.regs.begin() + (ptrdiff_t)i); --i; }
				}
			}
		});
		if (seconds) seconds[7] += std::chrono::duration<double>(clk::now() - t0).count();
	}
	auto t0 = clk::now();
	for_each_on_threads(reads.size(), nt, 1, [&](size_t k) {
		Read &R = *reads[k];
		filter_regs(c, R);
		if (!c.sr && R.qlen >= c.opt.rank_min_len) { update_dp_max(c, R); filter_regs(c, R); }          // align.c:1014
		hit_sort(R);
		if (R.rounds >= 3) ++R.cnt[MM2GB_ALN_N_READS_3_ROUNDS];
	});
	if (seconds) seconds[7] += std::chrono::duration<double>(clk::now() - t0).count();
	return 0;
}

// the host's DP backend: a job at a time on the calling thread
struct HostBackend : AlBackend {
	std::vector<uint8_t> q, t;
	int run(const AlCtx &c, std::vector<AlRun> &runs, std::vector<uint32_t> &pool) override
	{
		KswEz reset;
		ksw_ez_reset(reset);
		for (AlRun &x : runs) {
			const int qlen = std::max(x.j.qlen, 0), tlen = std::max(x.j.tlen, 0);
			x.code = 0;
			if (al_too_big(c, x.j) && !x.ungapped) { ksw_store(reset, 0, &x.res); x.res.zdropped = 1; continue; }
			q.resize((size_t)qlen); t.resize((size_t)tlen);
			for (int k = 0; k < qlen; ++k) q[(size_t)k] = al_query(c.reads.data(), x.j, k);
			for (int k = 0; k < tlen; ++k) t[(size_t)k] = al_target(c.refs.data(), x.j, k);
			mm2gb_ksw_job_t job = { 0, 0, qlen, tlen, x.w, x.zdrop, x.end_bonus, x.flag };
			size_t at = pool.size();
			if (x.ungapped) {             // align.c:744-757: the one-word first pass, the walk, and the DP only where it drops
				KswEz z = reset;
				z.score = 0;
				for (int k = 0; k < qlen; ++k) z.score += al_ungapped_score(c.opt.a, c.opt.b, c.opt.e2, t[(size_t)k], q[(size_t)k]);
				const uint32_t word = (uint32_t)qlen << 4;
				const AlDrop d = al_drop_walk(1, [&](int) { return word; }, [&](int k) { return (int)q[(size_t)k]; }, [&](int k) { return (int)t[(size_t)k]; }, c.a, c.b, c.ambi, c.opt.q, c.opt.e);
				x.code = al_zdrop_code(c, x.j, d);
				if (!x.code) { ksw_store(z, 1, &x.res); pool.push_back(word); x.res.cigar_off = (int64_t)at; continue; }
				if (al_too_big(c, x.j)) { ksw_store(reset, 0, &x.res); x.res.zdropped = 1; continue; }
				job.flag = al_second_flag(x.flag);
				ksw_one_host(c.kc, job, q.data(), t.data(), &x.res, pool);
				x.res.cigar_off = (int64_t)at;
				continue;
			}
			ksw_one_host(c.kc, job, q.data(), t.data(), &x.res, pool);
			x.res.cigar_off = (int64_t)at;
			if (x.j.kind != 1) continue;
			const uint32_t *w = pool.data() + at;
			const AlDrop d = al_drop_walk(x.res.n_cigar, [&](int k) { return w[k]; }, [&](int k) { return (int)q[(size_t)k]; }, [&](int k) { return (int)t[(size_t)k]; },
			                              c.a, c.b, c.ambi, c.opt.q, c.opt.e);
			x.code = al_zdrop_code(c, x.j, d);
			if (!x.code) continue;
			pool.resize(at);
			job.flag = al_second_flag(x.flag); job.zdrop = al_second_zdrop(c, x.code);
			ksw_one_host(c.kc, job, q.data(), t.data(), &x.res, pool);
			x.res.cigar_off = (int64_t)at;
		}
		return 0;
	}
};

} // namespace

int al_zdrop_code(const AlCtx &c, const AlJob &j, const AlDrop &d)
{
	const mm2gb_align_opt_t &o = c.opt;
	const int q_len = d.q_to - d.q_from, t_len = d.t_to - d.t_from;
	if (!(o.flag & (MM2GB_F_SPLICE | MM2GB_F_SR | MM2GB_F_FOR_ONLY | MM2GB_F_REV_ONLY)) && d.max_zdrop > o.zdrop_inv && q_len < o.max_gap && t_len < o.max_gap) {
		std::vector<uint8_t> q2((size_t)std::max(q_len, 0)), ts((size_t)std::max(t_len, 0));
		for (int i = 0; i < q_len; ++i) { const uint8_t x = al_query(c.reads.data(), j, d.q_to - i - 1); q2[(size_t)i] = x >= 4 ? 4 : 3 - x; }
		for (int i = 0; i < t_len; ++i) ts[(size_t)i] = al_target(c.refs.data(), j, d.t_from + i);
		int q_off, t_off;
		const int score = ll_i16(c, std::max(q_len, 0), q2.data(), std::max(t_len, 0), ts.data(), o.q, o.e, &q_off, &t_off);
		if (score >= o.min_chain_score * o.a && score >= o.min_dp_max) return 2;
	}
	return d.max_zdrop > o.zdrop ? 1 : 0;
}

void pack_residues(int32_t n_ref, const char *const *ref_seqs, const int32_t *ref_lens, int64_t n_reads, const char *const *read_seqs, const int32_t *read_lens, int nt,
                   std::vector<int64_t> &ref_at, std::vector<int64_t> &read_at, std::vector<uint8_t> &refs, std::vector<uint8_t> &reads)
{
	ref_at.assign((size_t)n_ref + 1, 0); read_at.assign((size_t)n_reads + 1, 0);
	for (int32_t i = 0; i < n_ref; ++i) ref_at[(size_t)i + 1] = ref_at[(size_t)i] + ref_lens[i];
	for (int64_t i = 0; i < n_reads; ++i) read_at[(size_t)i + 1] = read_at[(size_t)i] + read_lens[i];
	refs.resize((size_t)ref_at.back()); reads.resize((size_t)read_at.back());
	for_each_on_threads((size_t)n_ref, nt, 1, [&](size_t i) { for (int32_t p = 0; p < ref_lens[i]; ++p) refs[(size_t)(ref_at[i] + p)] = nt4(ref_seqs[i][p]); });
	for_each_on_threads((size_t)n_reads, nt, 1, [&](size_t i) { for (int32_t p = 0; p < read_lens[i]; ++p) reads[(size_t)(read_at[i] + p)] = nt4(read_seqs[i][p]); });
}

int al_align_regs(const char *who_, const mm2gb_align_opt_t *opt_, const mm2gb_align_splice_opt_t *spl, int k, int idx_flag, int32_t n_ref, const char *const *ref_seqs, const int32_t *ref_lens,
                  int64_t n_reads, const char *const *read_seqs, const int32_t *read_lens, const int64_t *reg_off, const mm2gb_reg_t *regs,
                  const int64_t *anchor_off, const mm2gb_anchor_t *anchors, int n_threads, AlBackend *whole_batch, mm2gb_align_out_t *out, int64_t *splice_counts, bool single, int64_t *sr_counts, bool sr)
{
	const std::string who = who_;
	if (!out) return fail(who + ": null argument");
	memset(out, 0, sizeof *out);
	if (splice_counts) memset(splice_counts, 0, MM2GB_SPL_N_COUNTS * 8);
	if (sr_counts) memset(sr_counts, 0, MM2GB_SR_N_COUNTS * 8);
	mm2gb_align_opt_t opt_own;
	const mm2gb_align_opt_t *opt = opt_;
	if (spl && opt_) {            // options.c:70-71: either strand flag implies MM_F_SPLICE
		opt_own = *opt_;
		if (opt_own.flag & (MM2GB_F_SPLICE_FOR | MM2GB_F_SPLICE_REV)) opt_own.flag |= MM2GB_F_SPLICE;
		opt = &opt_own;
	}
	if (!opt || n_reads < 0 || n_ref < 0 || (n_ref > 0 && (!ref_seqs || !ref_lens)) || (n_reads > 0 && (!read_seqs || !read_lens || !reg_off || !anchor_off))) return fail(who + ": null argument");
	static const struct { int64_t bit; const char *name; } refused[] = { { MM2GB_F_SPLICE, "MM_F_SPLICE" }, { MM2GB_F_SR, "MM_F_SR" }, { MM2GB_F_QSTRAND, "MM_F_QSTRAND" }, { MM2GB_F_EQX, "MM_F_EQX" } };
	for (const auto &x : refused) if ((opt->flag & x.bit) && !(spl && x.bit == MM2GB_F_SPLICE) && !(sr && x.bit == MM2GB_F_SR)) return fail(who + ": " + x.name + " is not supported");
	if (sr) {
		if (!(opt->flag & MM2GB_F_SR)) return fail(who + ": the flag word lacks MM_F_SR (the calls without _sr align other reads)");
		if (idx_flag & MM2GB_I_HPC) return fail(who + ": an index with MM2GB_I_HPC is not supported (align.c:583)");
	}
	mm2gb_ksw_splice_param_t sp;
	if (spl) {
		if (!(opt->flag & MM2GB_F_SPLICE)) return fail(who + ": the flag word lacks MM_F_SPLICE (the calls without _splice align unspliced reads)");
		if (idx_flag & MM2GB_I_HPC) return fail(who + ": an index with MM2GB_I_HPC is not supported");
		if (opt->e <= 0) return fail(who + ": e must be above 0 (the reference divides by it)");
		if (opt->q <= 0 || opt->q2 < 0 || opt->q > 127 || opt->q2 > 127 || spl->noncan < 0 || spl->noncan > 127 || spl->junc_bonus < 0 || spl->junc_bonus > 127)
			return fail(who + ": q must be 1..127 and q2, noncan and junc_bonus 0..127");
		if (spl->anchor_ext_len < 0) return fail(who + ": anchor_ext_len must not be negative");
	}
	if (!spl && !single && opt->q == opt->q2 && opt->e == opt->e2) return fail(who + ": q == q2 && e == e2 selects ksw_extz2_sse, which is not supported");
	if (single && (opt->q != opt->q2 || opt->e != opt->e2))
		return fail(who + ": q != q2 || e != e2 selects ksw_extd2_sse: that is mm2gb_align_regs_host / mm2gb_align_regs_gpu");
	if (opt->max_sw_mat <= 0 || opt->max_sw_mat > MM2GB_KSW_MAX_CELLS) return fail(who + ": max_sw_mat must be in 1 .. MM2GB_KSW_MAX_CELLS");
	if (opt->e <= 0 || opt->q <= 0 || (spl ? opt->q + opt->e : opt->q + opt->e + opt->q2 + opt->e2) > 127) return fail(who + ": gap penalties out of range");      // single: 2(q + e)
	for (int64_t r = 0; r < n_reads; ++r) {
		const int64_t na = anchor_off[r + 1] - anchor_off[r];
		if (na < 0 || reg_off[r + 1] < reg_off[r] || read_lens[r] < 0) return fail(who + ": read " + std::to_string(r) + ": offsets not ascending");
		for (int64_t i = anchor_off[r]; i < anchor_off[r + 1]; ++i)
			if (anchors[i].y >> 48 & 0xff) return fail(who + ": read " + std::to_string(r) + ": multi-segment reads are not supported");
		for (int64_t i = reg_off[r]; i < reg_off[r + 1]; ++i) {
			const mm2gb_reg_t &g = regs[i];
			if (g.flags & RF_SEG_SPLIT) return fail(who + ": read " + std::to_string(r) + ": multi-segment reads are not supported");
			if (g.as < 0 || g.cnt < 0 || (int64_t)g.as + g.cnt > na) return fail(who + ": read " + std::to_string(r) + ": record " + std::to_string(i - reg_off[r]) + ": as + cnt leaves the read's anchors");
			for (int64_t t = 0; t < g.cnt; ++t) {
				const mm2gb_anchor_t &a = anchors[anchor_off[r] + g.as + t];
				const int64_t rid = (int64_t)(a.x << 1 >> 33);
				if (rid >= n_ref || ax(a) < 0 || ax(a) >= ref_lens[rid] || ay(a) < 0 || ay(a) >= read_lens[r])
					return fail(who + ": read " + std::to_string(r) + ": an anchor lies outside its sequences");
			}
		}
	}
	AlCtx c;
	c.opt = *opt; c.k = k; c.idx_flag = idx_flag;
	c.a = opt->a < 0 ? -opt->a : opt->a; c.b = opt->b < 0 ? -opt->b : opt->b; c.ambi = opt->sc_ambi < 0 ? -opt->sc_ambi : opt->sc_ambi;
	c.bw = (int)(opt->bw * 1.5 + 1.); c.bw_long = (int)(opt->bw_long * 1.5 + 1.);
	if (c.bw_long < c.bw) c.bw_long = c.bw;
	for (int i = 0; i < 5; ++i) for (int j = 0; j < 5; ++j) c.mat[i * 5 + j] = (int8_t)al_score(c.a, c.b, c.ambi, i, j);
	if (spl) {
		sp.m = 5; memcpy(sp.mat, c.mat, 25); sp.q = (int8_t)opt->q; sp.e = (int8_t)opt->e; sp.q2 = (int8_t)opt->q2; sp.noncan = (int8_t)spl->noncan; sp.junc_bonus = (int8_t)spl->junc_bonus;
		c.kc = ksw_derive_splice(sp);
		c.splice = true; c.noncan = spl->noncan; c.junc_bonus = spl->junc_bonus; c.anchor_ext_len = spl->anchor_ext_len; c.anchor_ext_shift = spl->anchor_ext_shift;
	} else {
		mm2gb_ksw_param_t kp;
		kp.m = 5; memcpy(kp.mat, c.mat, 25); kp.q = (int8_t)opt->q; kp.e = (int8_t)opt->e; kp.q2 = (int8_t)opt->q2; kp.e2 = (int8_t)opt->e2;
		c.kc = single ? ksw_derive_single(kp) : ksw_derive(kp);          // align.c:331; nothing else of the call reads q2 or e2
	}
	c.sr = sr;
	c.n_ref = n_ref; c.n_reads = n_reads;
	const int nt = std::min(n_threads, 256);
	pack_residues(n_ref, ref_seqs, ref_lens, n_reads, read_seqs, read_lens, nt, c.ref_at, c.read_at, c.refs, c.reads);
	std::vector<Read> R((size_t)n_reads);
	for_each_on_threads((size_t)n_reads, nt, 1, [&](size_t r) {
		Read &x = R[r];
		x.id = (int64_t)r; x.qlen = read_lens[r];
		x.a.assign(anchors + anchor_off[r], anchors + anchor_off[r + 1]);
		x.regs.resize((size_t)(reg_off[r + 1] - reg_off[r]));
		for (size_t i = 0; i < x.regs.size(); ++i) x.regs[i].r = regs[reg_off[r] + (int64_t)i];
		squeeze_a(x);
	});
	int rc = 0;
	if (whole_batch) {
		std::vector<Read*> all;
		for (Read &x : R) all.push_back(&x);
		rc = drive(c, all, *whole_batch, nt, out->seconds);
		for (int s : { 0, 2, 3, 4, 5, 6 }) out->seconds[s] = whole_batch->seconds[s];
	} else {
		std::atomic<int> bad(0);
		for_each_on_threads((size_t)n_reads, nt, 1, [&](size_t r) {
			static thread_local HostBackend be;               // carries only the capacity of q and t between calls: run() sizes and fills both for every job
			std::vector<Read*> one{ &R[r] };
			if (drive(c, one, be, 1, nullptr)) bad = 1;
		});
		rc = bad ? -1 : 0;
	}
	if (rc) return -1;
	// the batch's arrays
	int64_t n_regs = 0, n_cigar = 0;
	for (const Read &x : R) for (const Reg &g : x.regs) { ++n_regs; if (g.has_p) n_cigar += (int64_t)g.cig.size(); }
	out->reg_off = (int64_t*)malloc((size_t)(n_reads + 1) * 8);
	out->regs = (mm2gb_reg_t*)malloc((size_t)std::max<int64_t>(n_regs, 1) * sizeof(mm2gb_reg_t));
	out->aln = (mm2gb_aln_t*)malloc((size_t)std::max<int64_t>(n_regs, 1) * sizeof(mm2gb_aln_t));
	out->cigar = (uint32_t*)malloc((size_t)std::max<int64_t>(n_cigar, 1) * 4);
	if (!out->reg_off || !out->regs || !out->aln || !out->cigar) { mm2gb_align_out_free(out); return fail(who + ": out of memory for the results"); }
	int64_t nr = 0, nc = 0;
	for (int64_t r = 0; r < n_reads; ++r) {
		out->reg_off[r] = nr;
		for (const Reg &g : R[(size_t)r].regs) {
			out->regs[nr] = g.r;
			mm2gb_aln_t &p = out->aln[nr++];
			memset(&p, 0, sizeof p);
			p.cigar_off = -1;
			if (!g.has_p) continue;
			p.dp_score = g.dp_score; p.dp_max = g.dp_max; p.dp_max2 = g.dp_max2; p.n_ambi = g.n_ambi; p.trans_strand = g.trans_strand; p.n_cigar = (int32_t)g.cig.size(); p.cigar_off = nc;
			if (!g.cig.empty()) memcpy(out->cigar + nc, g.cig.data(), g.cig.size() * 4);
			nc += (int64_t)g.cig.size();
		}
		for (int k2 = 0; k2 < MM2GB_ALN_N_COUNTS; ++k2) {
			if (k2 == MM2GB_ALN_N_ROUNDS) out->counts[k2] = std::max<int64_t>(out->counts[k2], R[(size_t)r].rounds);
			else out->counts[k2] += R[(size_t)r].cnt[k2];
		}
		if (splice_counts) for (int k2 = 0; k2 < MM2GB_SPL_N_COUNTS; ++k2) splice_counts[k2] += R[(size_t)r].scnt[k2];
		if (sr_counts) for (int k2 = 0; k2 < MM2GB_SR_N_COUNTS; ++k2) sr_counts[k2] += R[(size_t)r].srcnt[k2];
	}
	out->reg_off[n_reads] = nr;
	out->n_regs = n_regs; out->n_cigar = n_cigar;
	return 0;
}

} // namespace mm2gb

using namespace mm2gb;

namespace mm2gb {
// options.c:95-131 on top of mm_mapopt_init's a=2 b=4 q=4 e=2 q2=24 e2=1, zdrop 400 / 200, min_dp_max = 40 * 2, max_gap 5000, bw 500 / 20000,
// min_mid_occ 10, max_mid_occ 1000000, best_n 5.  map-pb changes the index alone (options.c:102-103); MM_F_RMQ is 0x80000000
static const PresetRow preset_table[] = {
	//  name        a  b   q   e  q2  e2  zdrop inv  min_dp_max max_gap bw    bw_long  flag         min/max_mid_occ best_n
	{ "map-ont",    2, 4,  4,  2, 24, 1,  400,  200, 80,        5000,   500,  20000,   0,           10, 1000000,    5 },
	{ "map-pb",     2, 4,  4,  2, 24, 1,  400,  200, 80,        5000,   500,  20000,   0,           10, 1000000,    5 },
	{ "map-hifi",   1, 4,  6,  2, 26, 1,  400,  200, 200,       10000,  500,  20000,   0,           50, 500,        5 },
	{ "map-ccs",    1, 4,  6,  2, 26, 1,  400,  200, 200,       10000,  500,  20000,   0,           50, 500,        5 },
	{ "asm5",       1, 19, 39, 3, 81, 1,  200,  200, 200,       10000,  1000, 100000,  0x80000000LL, 50, 500,       50 },
	{ "asm10",      1, 9,  16, 2, 41, 1,  200,  200, 200,       10000,  1000, 100000,  0x80000000LL, 50, 500,       50 },
	{ "asm20",      1, 4,  6,  2, 26, 1,  200,  200, 200,       10000,  1000, 100000,  0x80000000LL, 50, 500,       50 },
};
const char *const preset_names = "map-ont, map-pb, map-hifi, map-ccs, asm5, asm10, asm20";
const PresetRow *preset_row(const char *name)
{
	for (const PresetRow &r : preset_table) if (!strcmp(r.name, name)) return &r;
	return nullptr;
}
}

int mm2gb_align_opt_init(mm2gb_align_opt_t *opt, const char *preset)
{
	if (!opt || !preset) return fail("mm2gb_align_opt_init: null argument");
	const PresetRow *p = preset_row(preset);
	if (!p) return fail(std::string("mm2gb_align_opt_init: preset ") + preset + " is not supported (" + preset_names + ")");
	memset(opt, 0, sizeof *opt);            // options.c:14-66, then the preset's row
	opt->flag = p->map_flag;                // (mm_mapopt_t has one flag word: the asm presets' MM_F_RMQ stands here too; the alignment calls do not look at it)
	opt->min_cnt = 3; opt->min_chain_score = 40; opt->bw = p->bw; opt->bw_long = p->bw_long; opt->max_gap = p->max_gap;
	opt->a = p->a; opt->b = p->b; opt->q = p->q; opt->e = p->e; opt->q2 = p->q2; opt->e2 = p->e2; opt->sc_ambi = 1;
	opt->zdrop = p->zdrop; opt->zdrop_inv = p->zdrop_inv; opt->end_bonus = -1;
	opt->min_dp_max = p->min_dp_max; opt->min_ksw_len = 200;
	opt->max_clip_ratio = 1.0f; opt->max_sw_mat = 100000000;
	opt->rank_min_len = 500; opt->rank_frac = 0.9f;
	return 0;
}

int mm2gb_align_splice_opt_init(mm2gb_align_splice_opt_t *opt, const char *preset)
{
	if (!opt || !preset) return fail("mm2gb_align_splice_opt_init: null argument");
	const bool hq = !strcmp(preset, "splice:hq");
	if (strcmp(preset, "splice") != 0 && strcmp(preset, "cdna") != 0 && !hq) return fail(std::string("mm2gb_align_splice_opt_init: preset ") + preset + " is not supported (splice, cdna, splice:hq)");
	memset(opt, 0, sizeof *opt);            // options.c:14-66, then 151-162
	mm2gb_align_opt_t &o = opt->base;
	o.flag = MM2GB_F_SPLICE | MM2GB_F_SPLICE_FOR | MM2GB_F_SPLICE_REV | MM2GB_F_SPLICE_FLANK;
	o.min_cnt = 3; o.min_chain_score = 40; o.max_gap = 2000; o.bw = o.bw_long = 200000;
	o.a = 1; o.b = 2; o.q = 2; o.e = 1; o.q2 = 32; o.e2 = 0; o.sc_ambi = 1;
	opt->noncan = 9; opt->junc_bonus = 9;
	if (hq) { opt->junc_bonus = 5; o.b = 4; o.q = 6; o.q2 = 24; }
	o.zdrop = 200; o.zdrop_inv = 100; o.end_bonus = -1;
	o.min_dp_max = 80; o.min_ksw_len = 200;            // mm_mapopt_init's min_chain_score * a with ITS a = 2; the preset does not touch it
	opt->anchor_ext_len = 20; opt->anchor_ext_shift = 6;
	o.max_clip_ratio = 1.0f; o.max_sw_mat = MM2GB_KSW_MAX_CELLS;            // the departure: the preset's 0 means no limit
	o.rank_min_len = 500; o.rank_frac = 0.9f;
	return 0;
}

int mm2gb::al_align_regs_host(const char *who, const mm2gb_align_opt_t *opt, const mm2gb_align_splice_opt_t *spl, int k, int idx_flag, int32_t n_ref, const char *const *ref_seqs,
                              const int32_t *ref_lens, int64_t n_reads, const char *const *read_seqs, const int32_t *read_lens, const int64_t *reg_off, const mm2gb_reg_t *regs,
                              const int64_t *anchor_off, const mm2gb_anchor_t *anchors, int n_threads, mm2gb_align_out_t *out, int64_t *splice_counts, bool single, int64_t *sr_counts, bool sr)
{
	// MM2GB_ALIGN_ROUNDS=batch (read at every call): the device form's schedule -- every read in one sequence of rounds, planning and stitching on
	// n_threads threads -- with the host DP behind it; the same bytes come out.  For checking that schedule where there is no device.
	const char *mode = getenv("MM2GB_ALIGN_ROUNDS");
	if (mode && !strcmp(mode, "batch")) {
		HostBackend be;
		return al_align_regs(who, opt, spl, k, idx_flag, n_ref, ref_seqs, ref_lens, n_reads, read_seqs, read_lens, reg_off, regs, anchor_off, anchors, n_threads, &be, out, splice_counts, single, sr_counts, sr);
	}
	return al_align_regs(who, opt, spl, k, idx_flag, n_ref, ref_seqs, ref_lens, n_reads, read_seqs, read_lens, reg_off, regs, anchor_off, anchors, n_threads, nullptr, out, splice_counts, single, sr_counts, sr);
}

int mm2gb_align_regs_host(const mm2gb_align_opt_t *opt, int k, int idx_flag, int32_t n_ref, const char *const *ref_seqs, const int32_t *ref_lens,
                          int64_t n_reads, const char *const *read_seqs, const int32_t *read_lens, const int64_t *reg_off, const mm2gb_reg_t *regs,
                          const int64_t *anchor_off, const mm2gb_anchor_t *anchors, int n_threads, mm2gb_align_out_t *out)
{
	return al_align_regs_host("mm2gb_align_regs_host", opt, nullptr, k, idx_flag, n_ref, ref_seqs, ref_lens, n_reads, read_seqs, read_lens, reg_off, regs, anchor_off, anchors, n_threads, out, nullptr);
}

int mm2gb_align_regs_splice_host(const mm2gb_align_splice_opt_t *opt, int k, int idx_flag, int32_t n_ref, const char *const *ref_seqs, const int32_t *ref_lens,
                                 int64_t n_reads, const char *const *read_seqs, const int32_t *read_lens, const int64_t *reg_off, const mm2gb_reg_t *regs,
                                 const int64_t *anchor_off, const mm2gb_anchor_t *anchors, int n_threads, mm2gb_align_out_t *out, int64_t *splice_counts)
{
	if (!opt) { if (out) memset(out, 0, sizeof *out); return fail("mm2gb_align_regs_splice_host: null argument"); }
	return al_align_regs_host("mm2gb_align_regs_splice_host", &opt->base, opt, k, idx_flag, n_ref, ref_seqs, ref_lens, n_reads, read_seqs, read_lens, reg_off, regs, anchor_off, anchors, n_threads, out, splice_counts);
}

int mm2gb_align_regs_extz_host(const mm2gb_align_opt_t *opt, int k, int idx_flag, int32_t n_ref, const char *const *ref_seqs, const int32_t *ref_lens,
                               int64_t n_reads, const char *const *read_seqs, const int32_t *read_lens, const int64_t *reg_off, const mm2gb_reg_t *regs,
                               const int64_t *anchor_off, const mm2gb_anchor_t *anchors, int n_threads, mm2gb_align_out_t *out)
{
	return al_align_regs_host("mm2gb_align_regs_extz_host", opt, nullptr, k, idx_flag, n_ref, ref_seqs, ref_lens, n_reads, read_seqs, read_lens, reg_off, regs, anchor_off, anchors, n_threads, out, nullptr, true);
}

void mm2gb_align_sr_opt_init(mm2gb_align_opt_t *o)          // options.c:14-66, then 133-150
{
	memset(o, 0, sizeof *o);
	o->flag = MM2GB_F_SR | MM2GB_F_FRAG_MODE | MM2GB_F_NO_PRINT_2ND | MM2GB_F_HEAP_SORT;
	o->min_cnt = 2; o->min_chain_score = 25; o->bw = o->bw_long = 100; o->max_gap = 100;
	o->a = 2; o->b = 8; o->q = 12; o->e = 2; o->q2 = 24; o->e2 = 1; o->sc_ambi = 1; o->zdrop = o->zdrop_inv = 100; o->end_bonus = 10; o->min_dp_max = 40; o->min_ksw_len = 200;
	o->max_clip_ratio = 1.0f; o->max_sw_mat = 100000000; o->rank_min_len = 500; o->rank_frac = 0.9f;
}

int mm2gb_align_regs_sr_host(const mm2gb_align_opt_t *opt, int k, int idx_flag, int32_t n_ref, const char *const *ref_seqs, const int32_t *ref_lens,
                             int64_t n_reads, const char *const *read_seqs, const int32_t *read_lens, const int64_t *reg_off, const mm2gb_reg_t *regs,
                             const int64_t *anchor_off, const mm2gb_anchor_t *anchors, int n_threads, mm2gb_align_out_t *out, int64_t *sr_counts)
{
	return al_align_regs_host("mm2gb_align_regs_sr_host", opt, nullptr, k, idx_flag, n_ref, ref_seqs, ref_lens, n_reads, read_seqs, read_lens, reg_off, regs, anchor_off, anchors, n_threads, out, nullptr, false, sr_counts, true);
}

void mm2gb_align_out_free(mm2gb_align_out_t *out)
{
	if (!out) return;
	free(out->reg_off); free(out->regs); free(out->aln); free(out->cigar);
	out->reg_off = nullptr; out->regs = nullptr; out->aln = nullptr; out->cigar = nullptr;
	out->n_regs = out->n_cigar = 0;
}
