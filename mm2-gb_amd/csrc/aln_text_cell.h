// aln_text_cell.h -- internal: what the host and the device form of mm2gb_aln_text_* share: what one column of an alignment
// emits into cs:Z / MD:Z (write_cs_core and write_MD_core, format.c:141-218), restated per column so that columns can be taken in any order.
//
// A column is one base of a CIGAR word: a target and a query residue (M), a query residue (I) or a target residue (D).  Both tags are a
// sequence of a column's own bytes and of run lengths.  A column either counts one towards the open run (`m`), or is an event (`ev`) that
// closes the run before it and prints its length, or neither.  The first column of an M word under cs is both: it closes the run of the
// word before and opens the next with itself.  The length an event prints is the number of counting columns since the event before it,
// that event included where it counts.  The record's end closes the last run.
//   cs short   match: counts; the first column of every word and every other column: event.  A length prints as ":%d" when positive.
//   cs long    no run lengths: a match prints its base, with "=" in front where the column before it in the word is no match.
//   MD         match: counts; mismatch and the first column of a D word: event, the length prints as "%d", zero too; insertions and the
//              other columns of a D word neither.  At the record's end a length prints only when positive.
// The spliced calls (mm2gb_aln_text_splice_*) know a fourth word, N (an intron): ONE column whatever its length, which advances the target
// by the word's length.  cs, short and long: an event (short form) whose own bytes are "~", the intron's first two target bases, its
// length, its last two (format.c:179-184; tx_intron_*).  MD: neither event nor count nor bytes (format.c:212-213).  tx_col is not asked.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mm2gb {

enum { TX_CS = 0, TX_CS_LONG = 1, TX_MD = 2 };          // a call's mode (with both CS and MD asked for it is MD, format.c:329)

struct TxCol {
	uint8_t ev, m, n_own;        // event, counts towards the run, bytes of its own
	char own[3];
};

// op: 0 M, 1 I, 2 D; first: the word's first column; t / q: the residues (0..4) the word consumes (the other is ignored);
// prev_match (cs long, M, not first): the column before is a match
__host__ __device__ inline TxCol tx_col(int mode, int op, bool first, int t, int q, bool prev_match)
{
	const char *lo = "acgtn", *up = "ACGTN";
	TxCol c;
	c.ev = c.m = c.n_own = 0; c.own[0] = c.own[1] = c.own[2] = 0;
	const bool match = op == 0 && t == q;
	// (own[] is only ever indexed by constants: it stays in registers)
	if (mode == TX_MD) {
		if (match) c.m = 1;
		else if (op == 0) { c.ev = 1; c.own[0] = up[t]; c.n_own = 1; }
		else if (op == 2 && first) { c.ev = 1; c.own[0] = '^'; c.own[1] = up[t]; c.n_own = 2; }
		else if (op == 2) { c.own[0] = up[t]; c.n_own = 1; }
		return c;
	}
	if (match) {
		if (mode == TX_CS) { c.m = 1; c.ev = first; }
		else if (first || !prev_match) { c.own[0] = '='; c.own[1] = up[q]; c.n_own = 2; }
		else { c.own[0] = up[q]; c.n_own = 1; }
	} else {
		c.ev = mode == TX_CS;
		const char base = lo[op == 1 ? q : t];
		if (op == 0) { c.own[0] = '*'; c.own[1] = lo[t]; c.own[2] = lo[q]; c.n_own = 3; }
		else if (first) { c.own[0] = op == 1 ? '+' : '-'; c.own[1] = base; c.n_own = 2; }
		else { c.own[0] = base; c.n_own = 1; }
	}
	return c;
}

__host__ __device__ inline int tx_digits(uint32_t v) { int n = 1; while (v >= 10) { v /= 10; ++n; } return n; }

// bytes of the run length an event (at_end: the record's end) prints for a run of `len`
__host__ __device__ inline int tx_len_bytes(int mode, bool at_end, int len)
{
	if (mode == TX_CS) return len > 0 ? 1 + tx_digits((uint32_t)len) : 0;
	if (mode == TX_MD) return len > 0 || !at_end ? tx_digits((uint32_t)len) : 0;
	return 0;
}
// writes them at p; P(i, ch) stores one byte
template <class Put> __host__ __device__ inline void tx_put_len(int mode, bool at_end, int len, int64_t p, Put P)
{
	const int n = tx_len_bytes(mode, at_end, len);
	if (n == 0) return;
	int d = n;
	if (mode == TX_CS) { P(p, ':'); ++p; --d; }
	uint32_t v = (uint32_t)len;
	for (int i = d - 1; i >= 0; --i) { P(p + i, (char)('0' + v % 10)); v /= 10; }
}
// a CIGAR word in cg:Z, "%d%c"
__host__ __device__ inline int tx_word_bytes(uint32_t w) { return tx_digits(w >> 4) + 1; }
template <class Put> __host__ __device__ inline void tx_put_word(uint32_t w, int64_t p, Put P)
{
	const int d = tx_digits(w >> 4);
	uint32_t v = w >> 4;
	for (int i = d - 1; i >= 0; --i) { P(p + i, (char)('0' + v % 10)); v /= 10; }
	P(p + d, "MIDN"[w & 0xf]);
}
// an N word's own bytes in cs:Z: t0 t1 / t2 t3 the first and the last two target residues of the intron (len >= 2: they may be the same two)
__host__ __device__ inline int tx_intron_bytes(uint32_t len) { return 5 + tx_digits(len); }
template <class Put> __host__ __device__ inline void tx_put_intron(uint32_t len, int t0, int t1, int t2, int t3, int64_t p, Put P)
{
	const char *lo = "acgtn";
	const int d = tx_digits(len);
	P(p, '~'); P(p + 1, lo[t0]); P(p + 2, lo[t1]);
	uint32_t v = len;
	for (int i = d - 1; i >= 0; --i) { P(p + 3 + i, (char)('0' + v % 10)); v /= 10; }
	P(p + 3 + d, lo[t2]); P(p + 4 + d, lo[t3]);
}

// the query residue of column position k of a record: forward reads[q_at + k]; reverse strand: the complement of reads[q_at - k], q_at the
// residue at qe - 1 (format.c:236-244)
__host__ __device__ inline int tx_query(const uint8_t *reads, int64_t q_at, int rev, int k)
{
	if (!rev) return reads[q_at + k];
	const int c = reads[q_at - k];
	return c < 4 ? 3 - c : 4;
}

} // namespace mm2gb
