// ksw_cell.h -- internal: the dual-affine extension DP's constants, band, cell update, row bookkeeping and backtrack, one definition
// for the host form (ksw_host.cpp) and the device's (ksw_kernels.hip).  DESIGN 6d says what each piece has to reproduce and why.
// The splice-aware DP uses the same pieces with a cell and site bytes of its own, and so does the single-affine DP
// (DESIGN 6d-c), whose bytes live in another domain; both at the end of this file.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mm2gb_chain.h"

namespace mm2gb {

constexpr int KSW_FLAGS_KNOWN = MM2GB_KSW_SCORE_ONLY | MM2GB_KSW_RIGHT | MM2GB_KSW_GENERIC_SC | MM2GB_KSW_APPROX_MAX | MM2GB_KSW_APPROX_DROP |
                                MM2GB_KSW_EXTZ_ONLY | MM2GB_KSW_REV_CIGAR;

// What the parameters come to once per batch.  q, e, q2, e2 are the tuple AFTER it has been ordered so that q + e <= q2 + e2;
// qe0 is q + e BEFORE that (the first cell's H is taken from it: trap 1).  form: which DP.  The splice-aware form has
// e2 = 0 and the two splice numbers; the single-affine form has e2 = e, ini = ini2 = 0 and the two bytes of its shifted
// domain, shift = 2(q + e) and cap = mat[0] + shift, both wrapped.  What only one form reads is 0 in the others.  All of it lies behind the
// bytes: with them in front of mat[] the dual-affine kernels take two more VGPRs and the global-image ones lose a wave of occupancy.
enum { KSW_DUAL = 0, KSW_SPLICE = 1, KSW_SINGLE = 2 };
struct KswConst {
	int    m, q, e, q2, e2, qe0, long_thres, long_diff, early;
	int8_t mat[25], sc_mch, sc_mis, sc_N, ini, ini2, q8, q28, qe8, qe28;
	int    form, noncan, junc_bonus;
	int8_t shift, cap;
};

__host__ __device__ inline int8_t ksw_i8(int v) { return (int8_t)(uint8_t)(unsigned)v; }      // wrap to 8 bits (trap 7)

// Either parameter record.  The splice-aware form has one long gap without an extension cost: e2 = 0, with which long_thres, long_diff, ini2
// and qe28 below are ksw_exts2's.  Its own are the second early return, tested before anything is divided by e (e > 0: ksw_check_splice),
// and the wildcard: -e, not -e2 (trap 10; 6d-b 5).
template <class Param>
inline KswConst ksw_derive_as(const Param &p, int e2, bool splice)
{
	KswConst c = {};
	c.m = p.m; c.q = p.q; c.e = p.e; c.q2 = p.q2; c.e2 = e2; c.qe0 = c.q + c.e; c.form = splice ? KSW_SPLICE : KSW_DUAL;
	for (int i = 0; i < 25; ++i) c.mat[i] = p.mat[i];
	if (c.m <= 1 || (splice && c.q2 <= c.q + c.e)) { c.early = 1; return c; }
	if (c.q2 + c.e2 < c.q + c.e) { int t = c.q; c.q = c.q2; c.q2 = t; t = c.e; c.e = c.e2; c.e2 = t; }      // never with splice: q2 > q + e
	int min_sc = c.mat[1];                                  // the diagonal's first entry is not looked at
	for (int t = 1; t < c.m * c.m; ++t) min_sc = min_sc < c.mat[t] ? min_sc : c.mat[t];
	c.early = -min_sc > 2 * (c.q + c.e);                    // no mismatch could ever be seen
	c.long_thres = c.e != c.e2 ? (c.q2 - c.q) / (c.e - c.e2) - 1 : 0;      // C's truncating division
	if (c.q2 + c.e2 + c.long_thres * c.e2 > c.q + c.e + c.long_thres * c.e) ++c.long_thres;
	c.long_diff = c.long_thres * (c.e - c.e2) - (c.q2 - c.q) - c.e2;
	c.sc_mch = c.mat[0]; c.sc_mis = c.mat[1];
	c.sc_N = c.mat[c.m * c.m - 1] == 0 ? ksw_i8(splice ? -c.e : -c.e2) : c.mat[c.m * c.m - 1];
	c.ini = ksw_i8(-c.q - c.e); c.ini2 = ksw_i8(-c.q2 - c.e2);
	c.q8 = ksw_i8(c.q); c.q28 = ksw_i8(c.q2); c.qe8 = ksw_i8(c.q + c.e); c.qe28 = ksw_i8(c.q2 + c.e2);
	return c;
}
inline KswConst ksw_derive(const mm2gb_ksw_param_t &p) { return ksw_derive_as(p, p.e2, false); }
inline KswConst ksw_derive_splice(const mm2gb_ksw_splice_param_t &p)
{
	KswConst c = ksw_derive_as(p, 0, true);
	c.noncan = p.noncan; c.junc_bonus = p.junc_bonus;
	return c;
}
// The single-affine form reads m, mat, q and e.  Nothing is ordered and there is no long gap; m == 1 is no early return, the minimum starts
// from mat[1] whatever m is, and the wildcard is -e (6d-c 6, 7).  e2 = e is what the z-drop reads.
inline KswConst ksw_derive_single(const mm2gb_ksw_param_t &p)
{
	KswConst c = {};
	c.form = KSW_SINGLE;
	c.m = p.m; c.q = c.q2 = p.q; c.e = c.e2 = p.e; c.qe0 = c.q + c.e;
	for (int i = 0; i < 25; ++i) c.mat[i] = p.mat[i];
	if (c.m <= 0) { c.early = 1; return c; }
	int min_sc = c.mat[1];
	for (int t = 1; t < c.m * c.m; ++t) min_sc = min_sc < c.mat[t] ? min_sc : c.mat[t];
	c.early = -min_sc > 2 * (c.q + c.e);
	c.sc_mch = c.mat[0]; c.sc_mis = c.mat[1];
	c.sc_N = c.mat[c.m * c.m - 1] == 0 ? ksw_i8(-c.e) : c.mat[c.m * c.m - 1];
	c.q8 = ksw_i8(c.q); c.shift = ksw_i8(2 * (c.q + c.e)); c.cap = ksw_i8(c.mat[0] + 2 * (c.q + c.e));
	return c;
}

// a job's band half-width as the recurrences use it, and the width of a row of direction bytes
__host__ __device__ inline int ksw_width(int qlen, int tlen, int w)
{
	const int big = tlen > qlen ? tlen : qlen;
	return w < 0 || w > big ? big : w;                      // beyond the longer side the band binds nowhere
}
__host__ __device__ inline int ksw_ncol16(int qlen, int tlen, int w)
{
	int n = qlen < tlen ? qlen : tlen;
	n = n < w + 1 ? n : w + 1;
	return ((n + 15) / 16 + 1) * 16;
}
__host__ __device__ inline int ksw_round16(int n) { return (n + 15) / 16 * 16; }

// cells [st0, en0] of anti-diagonal r; empty when st0 > en0 (trap 8)
__host__ __device__ inline void ksw_band(int r, int qlen, int tlen, int w, int *st0, int *en0)
{
	int st = 0, en = tlen - 1;
	if (st < r - qlen + 1) st = r - qlen + 1;
	if (en > r) en = r;
	if (st < (r - w + 1) >> 1) st = (r - w + 1) >> 1;
	if (en > (r + w) >> 1) en = (r + w) >> 1;
	*st0 = st; *en0 = en;
}

// u of the cell on the first column / v left of the first row, at anti-diagonal r: the long gap takes over at long_thres.  The
// single-affine form's is q with nothing subtracted (6d-c 5).
template <int FORM = KSW_DUAL>
__host__ __device__ inline int8_t ksw_edge(const KswConst &c, int r)
{
	if (FORM == KSW_SINGLE) return r == 0 ? (int8_t)0 : c.q8;
	return r == 0 ? c.ini : r < c.long_thres ? ksw_i8(-c.e) : r == c.long_thres ? ksw_i8(c.long_diff) : ksw_i8(-c.e2);
}
// what a row's bookkeeping adds to H for a difference byte b (a row's u or v): the byte itself, signed; in the single-affine form the
// byte read as unsigned, less q + e (6d-c 1)
template <int FORM>
__host__ __device__ inline int32_t ksw_diff(const KswConst &c, int8_t b)
{
	return FORM == KSW_SINGLE ? (int32_t)(uint8_t)b - c.qe0 : (int32_t)b;
}

// The byte the score pass finds at target position t.  The pass works in groups of 16 from st0, so it reads up to 15 positions past the
// target's end: zeros up to the next multiple of 16 (T), then the reversed query, which lies behind the target (trap 2).
template <class Seq>
__host__ __device__ inline uint8_t ksw_target_byte(const Seq &target, const Seq &query, int qlen, int tlen, int T, int t)
{
	if (t < tlen) return target[t];
	if (t < T) return 0;
	return t - T < qlen ? query[qlen - 1 - (t - T)] : 0;
}
// ... and at query position r - t (again zeros behind the reversed query's end)
template <class Seq>
__host__ __device__ inline uint8_t ksw_query_byte(const Seq &query, int qlen, int r, int t)
{
	const int j = r - t;
	return j >= 0 && j < qlen ? query[j] : 0;
}
// mat: the batch's matrix (KswConst::mat, or the kernel's copy of it in LDS: an indexed look-up into a kernel argument would go through scratch)
__host__ __device__ inline int8_t ksw_score(const KswConst &c, const int8_t *mat, bool generic, uint8_t tb, uint8_t qb)
{
	if (generic) return mat[tb * c.m + qb];
	const uint8_t wild = (uint8_t)(c.m - 1);
	return tb == wild || qb == wild ? c.sc_N : tb == qb ? c.sc_mch : c.sc_mis;
}

struct KswCell { int8_t u, v, x, y, x2, y2; uint8_t d; };

// One cell of anti-diagonal r from anti-diagonal r - 1: z the score byte, x1 / v1 / x21 the left neighbour's x, v, x2, and the cell's own
// u, y, y2.  Every sum wraps in 8 bits.  d: bits 0-2 which of the five candidates won, bits 3-6 whether each gap state goes on.
// Left and right gap alignment differ in both (trap 6): `>` against `not <` for the winner, `> 0` against `>= 0` for going on.
__host__ __device__ inline KswCell ksw_cell(const KswConst &c, bool right, int8_t z, int8_t x1, int8_t v1, int8_t x21, int8_t u, int8_t y, int8_t y2)
{
	int8_t a = ksw_i8(x1 + v1), b = ksw_i8(y + u), a2 = ksw_i8(x21 + v1), b2 = ksw_i8(y2 + u);
	uint8_t d;
	if (!right) {
		d = a > z ? 1 : 0;  z = a > z ? a : z;
		if (b > z)  { d = 2; z = b; }
		if (a2 > z) { d = 3; z = a2; }
		if (b2 > z) { d = 4; z = b2; }
	} else {
		d = z > a ? 0 : 1;  z = z > a ? z : a;
		if (!(z > b))  { d = 2; z = b; }
		if (!(z > a2)) { d = 3; z = a2; }
		if (!(z > b2)) { d = 4; z = b2; }
	}
	if (c.sc_mch < z) z = c.sc_mch;
	KswCell o;
	o.u = ksw_i8(z - v1); o.v = ksw_i8(z - u);
	int8_t tmp = ksw_i8(z - c.q8);
	a = ksw_i8(a - tmp); b = ksw_i8(b - tmp);
	tmp = ksw_i8(z - c.q28);
	a2 = ksw_i8(a2 - tmp); b2 = ksw_i8(b2 - tmp);
	o.x  = ksw_i8((a  > 0 ? a  : 0) - c.qe8);
	o.y  = ksw_i8((b  > 0 ? b  : 0) - c.qe8);
	o.x2 = ksw_i8((a2 > 0 ? a2 : 0) - c.qe28);
	o.y2 = ksw_i8((b2 > 0 ? b2 : 0) - c.qe28);
	if (!right) d |= (a > 0 ? 0x08 : 0) | (b > 0 ? 0x10 : 0) | (a2 > 0 ? 0x20 : 0) | (b2 > 0 ? 0x40 : 0);
	else        d |= (a >= 0 ? 0x08 : 0) | (b >= 0 ? 0x10 : 0) | (a2 >= 0 ? 0x20 : 0) | (b2 >= 0 ? 0x40 : 0);
	o.d = d;
	return o;
}

// The exact maximum of a row and its ties (trap 5) as one key to maximise: H in the upper half; below it the complement of the cell's rank in
// the order the ties are settled -- cell en0 first, then the cells of [st0, en1) as four interleaved classes (class, then position), then
// [en1, en0) in order; en1 = st0 + (en0 - st0) / 4 * 4.
__host__ __device__ inline uint64_t ksw_max_key(int32_t H, int t, int st0, int en0)
{
	const int en1 = st0 + (en0 - st0) / 4 * 4;
	uint32_t rank;
	if (t == en0) rank = 0;
	else if (t < en1) rank = 1u + ((uint32_t)((t - st0) & 3) << 27) + (uint32_t)((t - st0) >> 2);
	else rank = (1u << 29) + (uint32_t)(t - en1);
	return (uint64_t)((uint32_t)H ^ 0x80000000u) << 32 | (0xffffffffu - rank);
}
__host__ __device__ inline int32_t ksw_key_H(uint64_t key) { return (int32_t)((uint32_t)(key >> 32) ^ 0x80000000u); }
__host__ __device__ inline int ksw_key_t(uint64_t key, int st0, int en0)
{
	const uint32_t rank = 0xffffffffu - (uint32_t)key;
	if (rank == 0) return en0;
	if (rank < (1u << 29)) return st0 + (int)((rank - 1) & ((1u << 27) - 1)) * 4 + (int)((rank - 1) >> 27);
	return st0 + (en0 - st0) / 4 * 4 + (int)(rank - (1u << 29));
}

struct KswEz { int32_t max, zdropped, max_q, max_t, mqe, mqe_t, mte, mte_q, score, reach_end; };

__host__ __device__ inline void ksw_ez_reset(KswEz &z)
{
	z.max_q = z.max_t = z.mqe_t = z.mte_q = -1;
	z.max = 0; z.score = z.mqe = z.mte = MM2GB_KSW_NEG_INF;
	z.zdropped = 0; z.reach_end = 0;
}

// a job's record from its state (pad_ / cigar_off: 0; the kernel carries the walk's start in them to k_ksw_walk)
__host__ __device__ inline void ksw_store(const KswEz &z, int n_cigar, mm2gb_ksw_res_t *out)
{
	out->max = z.max; out->zdropped = z.zdropped; out->max_q = z.max_q; out->max_t = z.max_t; out->mqe = z.mqe; out->mqe_t = z.mqe_t;
	out->mte = z.mte; out->mte_q = z.mte_q; out->score = z.score; out->reach_end = z.reach_end; out->n_cigar = n_cigar; out->pad_ = 0; out->cigar_off = 0;
}

// a new best, or, diagonally behind the best by more than zdrop + e * (distance off its diagonal), the end of the job
__host__ __device__ inline bool ksw_zdrop(KswEz &z, int32_t H, int r, int t, int zdrop, int e)
{
	if (H > z.max) { z.max = H; z.max_t = t; z.max_q = r - t; }
	else if (t >= z.max_t && r - t >= z.max_q) {
		const int tl = t - z.max_t, ql = (r - t) - z.max_q, l = tl > ql ? tl - ql : ql - tl;
		if (zdrop >= 0 && z.max - H > zdrop + l * e) { z.zdropped = 1; return true; }
	}
	return false;
}

// After a row in exact mode: H_en0 / H_st0 are H of the band's two end cells, en the band's end rounded to a group (trap 3).  True: stop.
__host__ __device__ inline bool ksw_row_exact(KswEz &z, const KswConst &c, int qlen, int tlen, int zdrop, int r, int st0, int en0, int en,
                                              int32_t max_H, int max_t, int32_t H_en0, int32_t H_st0)
{
	if (en0 == tlen - 1 && H_en0 > z.mte) { z.mte = H_en0; z.mte_q = r - en; }
	if (r - st0 == qlen - 1 && H_st0 > z.mqe) { z.mqe = H_st0; z.mqe_t = st0; }
	if (ksw_zdrop(z, max_H, r, max_t, zdrop, c.e2)) return true;
	if (r == qlen + tlen - 2 && en0 == tlen - 1) z.score = H_en0;
	return false;
}

// After a row in approximate mode: one cell's H is followed down or right, whichever difference is larger.  V(t) / U(t): what this row's
// v, u add to H (ksw_diff).  The single-affine form does not test the drop at the first cell (6d-c 10).
template <int FORM = KSW_DUAL, class FV, class FU>
__host__ __device__ inline bool ksw_row_approx(KswEz &z, const KswConst &c, int qlen, int tlen, int zdrop, int flag, int r, int st0, int en0,
                                               int32_t &H0, int &H0_t, FV V, FU U)
{
	if (r > 0) {
		if (H0_t >= st0 && H0_t <= en0 && H0_t + 1 >= st0 && H0_t + 1 <= en0) {
			const int32_t d0 = V(H0_t), d1 = U(H0_t + 1);
			if (d0 > d1) H0 += d0;
			else { H0 += d1; ++H0_t; }
		} else if (H0_t >= st0 && H0_t <= en0) H0 += V(H0_t);
		else { ++H0_t; H0 += U(H0_t); }
	} else { H0 = V(0) - c.qe0; H0_t = 0; }
	if ((flag & MM2GB_KSW_APPROX_DROP) && (FORM != KSW_SINGLE || r > 0) && ksw_zdrop(z, H0, r, H0_t, zdrop, c.e2)) return true;
	if (r == qlen + tlen - 2 && en0 == tlen - 1) z.score = H0;
	return false;
}

// Where the backtrack starts once the rows are done; false: no CIGAR.  A dropped job still walks back from its best cell (trap 9).
// The splice-aware form has no end bonus and not its branch either (mqe > max can hold there): reach_end stays 0.
__host__ __device__ inline bool ksw_walk_from(KswEz &z, bool splice, int qlen, int tlen, int end_bonus, int flag, int *i0, int *j0)
{
	if (flag & MM2GB_KSW_SCORE_ONLY) return false;
	if (!z.zdropped && !(flag & MM2GB_KSW_EXTZ_ONLY)) { *i0 = tlen - 1; *j0 = qlen - 1; return true; }
	if (!splice && !z.zdropped && (flag & MM2GB_KSW_EXTZ_ONLY) && z.mqe + end_bonus > z.max) { z.reach_end = 1; *i0 = z.mqe_t; *j0 = qlen - 1; return true; }
	if (z.max_t >= 0 && z.max_q >= 0) { *i0 = z.max_t; *j0 = z.max_q; return true; }
	return false;
}

// The walk back over the direction bytes, P(row r, column) with columns counted from the row's rounded start.  Outside a row's rounded
// bounds the move is forced (trap 4).  Moves of one kind in a row make one word, handed to out(position, word) when the kind changes; words
// come out last operation first, and the caller reverses them unless REV_CIGAR is set.  At most qlen + tlen + 2 words; returns their number.
// min_intron: ksw_backtrack's min_intron_len -- 0 for the dual-affine form; the splice-aware form's long_thres, above 0 of which the long
// gap state is written N (3) and so is a leftover leading deletion at least that long.
template <class FP, class FO>
__host__ __device__ inline int ksw_walk(int qlen, int tlen, int w, int min_intron, int i, int j, FP P, FO out)
{
	int n = 0, state = 0, run_op = -1;
	uint32_t run_len = 0;
	auto push = [&](int op, int len) {
		if (op == run_op) { run_len += (uint32_t)len; return; }
		if (run_op >= 0) out(n++, run_len << 4 | (uint32_t)run_op);
		run_op = op; run_len = (uint32_t)len;
	};
	while (i >= 0 && j >= 0) {
		const int r = i + j;
		int st0, en0, force = -1;
		ksw_band(r, qlen, tlen, w, &st0, &en0);
		const int st = st0 / 16 * 16, en = (en0 + 16) / 16 * 16 - 1;
		if (i < st) force = 2;
		if (i > en) force = 1;
		const uint32_t tmp = force < 0 ? P(r, i - st) : 0;
		if (state == 0) state = tmp & 7;
		else if (!(tmp >> (state + 2) & 1)) state = 0;
		if (state == 0) state = tmp & 7;
		if (force >= 0) state = force;
		if (state == 0) { push(0, 1); --i; --j; }
		else if (state == 1 || state == 3) { push(state == 3 && min_intron > 0 ? 3 : 2, 1); --i; }
		else { push(1, 1); --j; }
	}
	if (i >= 0) push(min_intron > 0 && i >= min_intron ? 3 : 2, i + 1);
	if (j >= 0) push(1, j + 1);
	if (run_op >= 0) out(n++, run_len << 4 | (uint32_t)run_op);
	return n;
}

// ---- the splice-aware form (ksw2's ksw_exts2_sse).  It has the short gap (x, y with q, e) and ONE long gap, on the target side
// only (x2 with q2 and no extension cost), opened at donor[t] and closed at acceptor[t]; no band, no end bonus, no cap at the match score.
// Its constants (ksw_derive_splice) have e2 = 0, so that the edge values, the z-drop (no l * e term) and the first cell come out of the
// helpers above unchanged. ----
constexpr int KSW_SPLICE_BITS = MM2GB_KSW_SPLICE_FOR | MM2GB_KSW_SPLICE_REV | MM2GB_KSW_SPLICE_FLANK;

// donor[t] and acceptor[t] of a job (ksw2_exts2_sse.c:120-170, loop bounds as written there): 0 without SPLICE_FOR / SPLICE_REV; with either,
// -noncan everywhere up to the rounded target length, 0 at a full signal (GTr / yAG, CTr / yAC for the reverse strand; residues are the
// literal codes 0..3 whatever m is), -noncan / 2 with SPLICE_FLANK or else 0 at a bare GT / AG, and junc_bonus more where junc says so.
// REV_CIGAR means the target is a reversed left extension: the signals and the junc bits are the mirrored ones.
// tg(i): the target's residue i, asked only for 0 <= i < tlen; junc: the job's annotation bytes or null.
template <class FT>
__host__ __device__ inline void ksw_splice_sites(const KswConst &c, int flag, FT tg, const uint8_t *junc, int tlen, int t, int8_t *donor, int8_t *acceptor)
{
	*donor = *acceptor = 0;
	if (!(flag & (MM2GB_KSW_SPLICE_FOR | MM2GB_KSW_SPLICE_REV))) return;
	const bool fwd = (flag & MM2GB_KSW_SPLICE_FOR) != 0, rev = (flag & MM2GB_KSW_SPLICE_REV) != 0, mirror = (flag & MM2GB_KSW_REV_CIGAR) != 0;
	const int8_t none = ksw_i8(-c.noncan), semi = (flag & MM2GB_KSW_SPLICE_FLANK) ? ksw_i8(-c.noncan / 2) : (int8_t)0;
	int8_t d = none, a = none;
	if (t < tlen - 4) {
		const uint8_t b1 = tg(t + 1), b2 = tg(t + 2), b3 = tg(t + 3), second = mirror ? 0 : 3;
		int type = (fwd && b1 == 2 && b2 == second) || (rev && b1 == 1 && b2 == second);
		if (type && (mirror ? (b3 == 1 || b3 == 3) : (b3 == 0 || b3 == 2))) type = 2;
		if (type) d = type == 2 ? 0 : semi;
	}
	if (junc && t < tlen - 1 && ((fwd && (junc[t + 1] & (mirror ? 2 : 1))) || (rev && (junc[t + 1] & (mirror ? 4 : 8))))) d = ksw_i8(d + c.junc_bonus);
	if (t >= 2 && t < tlen) {
		const uint8_t b0 = tg(t), b1 = tg(t - 1), b2 = tg(t - 2), before = mirror ? 3 : 0;
		int type = (fwd && b1 == before && b0 == 2) || (rev && b1 == before && b0 == 1);
		if (type && (mirror ? (b2 == 0 || b2 == 2) : (b2 == 1 || b2 == 3))) type = 2;
		if (type) a = type == 2 ? 0 : semi;
	}
	if (junc && t < tlen && ((fwd && (junc[t] & (mirror ? 1 : 2))) || (rev && (junc[t] & (mirror ? 8 : 4))))) a = ksw_i8(a + c.junc_bonus);
	*donor = d; *acceptor = a;
}

// One cell: as ksw_cell, with a, b and a2 + acceptor the candidates beside the score byte, no cap at the match score, and the long gap going
// on where a2 beats donor (not 0): x2 = max(a2, donor) - q2.  The SSE2 build's score-only loop stores (a2 > donor ? a2 : 0) - q2 instead;
// the definition here is the max form for every flag.
__host__ __device__ inline KswCell ksw_cell_splice(const KswConst &c, bool right, int8_t z, int8_t x1, int8_t v1, int8_t x21, int8_t u, int8_t y, int8_t donor, int8_t acceptor)
{
	int8_t a = ksw_i8(x1 + v1), b = ksw_i8(y + u), a2 = ksw_i8(x21 + v1);
	const int8_t a2a = ksw_i8(a2 + acceptor);
	uint8_t d;
	if (!right) {
		d = a > z ? 1 : 0;  z = a > z ? a : z;
		if (b > z)   { d = 2; z = b; }
		if (a2a > z) { d = 3; z = a2a; }
	} else {
		d = z > a ? 0 : 1;  z = z > a ? z : a;
		if (!(z > b))   { d = 2; z = b; }
		if (!(z > a2a)) { d = 3; z = a2a; }
	}
	KswCell o;
	o.u = ksw_i8(z - v1); o.v = ksw_i8(z - u);
	const int8_t tmp = ksw_i8(z - c.q8);
	a = ksw_i8(a - tmp); b = ksw_i8(b - tmp);
	a2 = ksw_i8(a2 - ksw_i8(z - c.q28));
	o.x  = ksw_i8((a > 0 ? a : 0) - c.qe8);
	o.y  = ksw_i8((b > 0 ? b : 0) - c.qe8);
	o.x2 = ksw_i8((a2 > donor ? a2 : donor) - c.q28);
	o.y2 = 0;
	if (!right) d |= (a > 0 ? 0x08 : 0) | (b > 0 ? 0x10 : 0) | (a2 > donor ? 0x20 : 0);
	else        d |= (a >= 0 ? 0x08 : 0) | (b >= 0 ? 0x10 : 0) | (a2 >= donor ? 0x20 : 0);
	o.d = d;
	return o;
}

// ---- the single-affine form (ksw2's ksw_extz2_sse in its SSE2 build).  One gap cost, and the bytes in a domain of their own:
// non-negative and shifted, z = s + 2(q + e) capped at mat[0] + 2(q + e), x and y clamped at 0 with nothing subtracted, every array 0 at the
// start.  Sums and differences wrap, maximum and minimum are unsigned, and the compares that choose d and clamp are signed: that mix is the
// reference's, and it decides the cells outside the band that flow into real ones when the band moves. ----

// The first cell of a row takes x1 / v1 from a signed byte that the reference widens to 32 bits before it goes into the vector, so a byte
// with its top bit set fills the next three lanes too: the left neighbours of cells st + 1 .. st + 3 read as 0xff (6d-c 9).  Only v can
// have that bit (x is clamped to 0..127), and only where the cap is above 127.  first: the row's boundary v1; k: the cell's distance from
// st; b: the neighbour's v as stored.
__host__ __device__ inline int8_t ksw_smear(int8_t first, int k, int8_t b) { return first < 0 && k >= 1 && k <= 3 ? (int8_t)-1 : b; }

// One cell: s the score byte, x1 / v1 the left neighbour's x, v, and the cell's own u, y.  d: bits 0-1 which candidate won, 0x08 / 0x10
// whether each gap state goes on.  The three code paths of the reference (score only, left, right) compute the same bytes; only d differs.
__host__ __device__ inline KswCell ksw_cell_single(const KswConst &c, bool right, int8_t s, int8_t x1, int8_t v1, int8_t u, int8_t y)
{
	uint8_t z = (uint8_t)(s + c.shift), a = (uint8_t)(x1 + v1), b = (uint8_t)(y + u);
	uint8_t d = right ? ((int8_t)z > (int8_t)a ? 0 : 1) : ((int8_t)a > (int8_t)z ? 1 : 0);      // on the unclamped z
	z = (int8_t)z > 0 ? z : 0;
	z = z > a ? z : a;
	if (right ? !((int8_t)z > (int8_t)b) : (int8_t)b > (int8_t)z) d = 2;
	z = z > b ? z : b;
	z = z < (uint8_t)c.cap ? z : (uint8_t)c.cap;
	KswCell o;
	o.u = ksw_i8(z - (uint8_t)v1); o.v = ksw_i8(z - (uint8_t)u);
	z = (uint8_t)(z - c.q8);
	const int8_t a8 = ksw_i8(a - z), b8 = ksw_i8(b - z);
	o.x = a8 > 0 ? a8 : 0; o.y = b8 > 0 ? b8 : 0;
	o.x2 = o.y2 = 0;
	if (!right) d |= (a8 > 0 ? 0x08 : 0) | (b8 > 0 ? 0x10 : 0);
	else        d |= (a8 >= 0 ? 0x08 : 0) | (b8 >= 0 ? 0x10 : 0);
	o.d = d;
	return o;
}

} // namespace mm2gb
