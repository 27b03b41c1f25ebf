// align_cell.h -- internal: what the host and the device form of mm2gb_align_regs_* share: how a DP job names its two
// stretches inside the resident sequences, the residue a job finds at a position, and the walk of mm_test_zdrop (align.c:32-68).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mm2gb {

// One DP job of a round.  The query stretch is [q0, q0 + qlen) of the read's strand `rev` (0: as given, 1: reverse complement), the target
// stretch [t0, t0 + tlen) of reference sequence rid.  flip: both stretches are read backwards (the left extension, mm_seq_rev at
// align.c:709-711).  q_at / t_at: where the read / the reference sequence begins in the batch's residue arrays; qn the read's length.
struct AlJob {
	int64_t q_at, t_at;
	int32_t qn, tn, q0, qlen, t0, tlen;     // qn, tn: the lengths of the read and of the reference sequence
	int32_t rev, flip, kind;          // kind: 0 left extension, 1 gap fill, 2 right extension, 3 the alignment of an inversion
};

// residue k of a job's query / target; reads and refs: one residue (0..4) per base
__host__ __device__ inline uint8_t al_query(const uint8_t *reads, const AlJob &j, int k)
{
	const int p = j.q0 + (j.flip ? j.qlen - 1 - k : k);
	if (!j.rev) return reads[j.q_at + p];
	const uint8_t c = reads[j.q_at + (j.qn - 1 - p)];
	return c < 4 ? 3 - c : 4;
}
__host__ __device__ inline uint8_t al_target(const uint8_t *refs, const AlJob &j, int k)
{
	return refs[j.t_at + j.t0 + (j.flip ? j.tlen - 1 - k : k)];
}

// ksw_gen_simple_mat's entry for a target and a query residue (align.c:9-22) with a, b, sc_ambi already made positive
__host__ __device__ inline int al_score(int a, int b, int ambi, int t, int q) { return t >= 4 || q >= 4 ? -ambi : t == q ? a : -b; }

// a column of the short-read form's ungapped first pass (align.c:748-749): + e2 where either base is ambiguous, as the reference writes it (not -sc_ambi)
__host__ __device__ inline int al_ungapped_score(int a, int b, int e2, int t, int q) { return t >= 4 || q >= 4 ? e2 : t == q ? a : -b; }

// what the walk along a CIGAR leaves: the largest drop and where it lies (pos[0]: target from / to, pos[1]: query from / to)
struct AlDrop { int32_t max_zdrop, t_from, t_to, q_from, q_to, pad_; };

struct AlDropState { int32_t score, max, max_i, max_j; AlDrop d; };

__host__ __device__ inline void al_drop_update(AlDropState &s, int i, int j, int e)      // update_max_zdrop, align.c:32-45
{
	if (s.score < s.max) {
		const int li = i - s.max_i, lj = j - s.max_j, diff = li > lj ? li - lj : lj - li, z = s.max - s.score - diff * e;
		if (z > s.d.max_zdrop) { s.d.max_zdrop = z; s.d.t_from = s.max_i; s.d.t_to = i; s.d.q_from = s.max_j; s.d.q_to = j; }
	} else { s.max = s.score; s.max_i = i; s.max_j = j; }
}

// the first half of mm_test_zdrop (align.c:49-68): Q(j) / T(i) the job's residues, W(k) its CIGAR words
template <class FQ, class FT, class FW>
__host__ __device__ inline AlDrop al_drop_walk(int n_cigar, FW W, FQ Q, FT T, int a, int b, int ambi, int q, int e)
{
	AlDropState s;
	s.score = 0; s.max = INT32_MIN; s.max_i = s.max_j = -1;
	s.d.max_zdrop = 0; s.d.t_from = s.d.t_to = s.d.q_from = s.d.q_to = -1; s.d.pad_ = 0;
	int i = 0, j = 0;
	for (int k = 0; k < n_cigar; ++k) {
		const uint32_t w = W(k), op = w & 0xf;
		const int len = (int)(w >> 4);
		if (op == 0) {
			for (int l = 0; l < len; ++l) {
				s.score += al_score(a, b, ambi, T(i + l), Q(j + l));
				al_drop_update(s, i + l, j + l, e);
			}
			i += len; j += len;
		} else if (op == 1 || op == 2 || op == 3) {
			s.score -= q + e * len;
			if (op == 1) j += len; else i += len;
			al_drop_update(s, i, j, e);
		}
	}
	return s.d;
}

} // namespace mm2gb
