// seed_dev.h -- internal: device-side data of the kernels that come before the anchors (seed_kernels.hip): the minimizer sketch, the
// index look-up and the selection of seed matches -- seeding.cpp's sketch / collect_matches_refs for a whole batch of reads.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "post_dev.h"

namespace mm2gb {

// the index as SeedIndex holds it, copied to one device (seeding.cpp: index_on_device)
struct DevIndexView {
	const unsigned long long *keys;     // distinct minimizers, ascending
	const long long          *first;    // n_keys + 1
	const unsigned long long *where;    // occurrences
	const uint32_t           *bucket;   // n_bucket entries
	unsigned long long        n_bucket;
	int                       bucket_shift, k, w;
	int                       flag;     // MM2GB_I_*: reads are sketched the way the index was
};

// the kernels of seed_kernels.hip and index_kernels.hip: a thread per element, TB threads to a workgroup
constexpr int TB = 256;
inline unsigned blocks(int64_t n) { return (unsigned)std::max<int64_t>(1, (n + TB - 1) / TB); }

// carves arrays out of one arena; base == nullptr: only adds up what is needed
struct Carver {
	char *base; size_t at = 0;
	explicit Carver(void *b) : base((char*)b) {}
	template <class T> T *take(size_t n)
	{
		at = (at + 255) & ~(size_t)255;
		T *p = base ? (T*)(base + at) : nullptr;
		at += n * sizeof(T);
		return p;
	}
};

// The sketch by POSITION: sequences laid end to end, n bases in all (< 2^31).  Positions are global; a COUNTED position is
// one the serial loop gives a ring slot to (everything but the k-mers equal to their reverse complement).
// hpc != 0: homopolymer-compressed.  The loop's steps are the BOUNDARIES -- the first base of every run of equal bases and every ambiguous
// base; a run ends with its sequence --, the other positions count as skipped; a step's position is its run's last base.
struct SketchBatch {
	const unsigned char *seqs;         // n + 1 bytes, the last one 'N'
	const int64_t  *seq_off;           // n_seqs + 1
	const uint32_t *rid;               // per sequence, or null (0)
	int64_t         n_seqs, n;
	int             w, k, hpc;
	// scratch (n + 1 entries each)
	uint32_t *n_valid;                 // A/C/G/T before each position (hpc: run starts before each position)
	uint32_t *n_skip;                  // skipped positions before each position
	uint32_t *last_n;                  // 1 + the last ambiguous position at or before each position (0: none)
	unsigned char *comp;               // the sequences without their ambiguous bases, each at its own offset (hpc: a base per run)
	unsigned char *flags;              // 1 valid | 2 skipped | 4 strand (hpc, before the words: 1 run start | 2 ambiguous)
	unsigned long long *hx;            // hash << 8 | span of the canonical k-mer ending here (hpc: ~0 where the span is 256 or more)
	unsigned long long *vx;            // by counted position: the step's value (~0: none)
	uint32_t *vy;                      // by counted position: position in the sequence << 1 | strand
	uint32_t *vrun;                    // by counted position: min(run, w + k)
	int64_t  *cstart;                  // n_seqs + 1: where each sequence's counted positions begin
	uint32_t *emit_cnt;                // by counted position: pairs the step emits
	int64_t  *emit_off;                // their exclusive scan
	uint32_t *n_bnd;                   // hpc only: boundaries before each position
	uint32_t *bnd_pos;                 // hpc only (n + 2 entries): the boundaries' positions; position n is the last one
	void     *tmp; size_t tmp_bytes;   // the library scans' work space
	// out
	int64_t  *mini_off;                // n_seqs + 1
	ulonglong2 *mini;                  // the pairs (set before launch_sketch_write)
	int32_t  *mini_read;               // their sequence
};
// The layout functions size the library calls' work space by running the launch's own list of steps without launching (seed_kernels.hip:
// Pass), so a step under a condition is sized under that condition: everything above "scratch" -- hpc here, the options and the counts of
// MatchBatch -- is set BEFORE the layout is asked for and stays as it is until the launch.
size_t sketch_layout(SketchBatch &b, void *base);            // sets the scratch pointers inside base; returns the bytes needed
int    launch_sketch_count(const SketchBatch &b, hipStream_t s);   // through mini_off; -1: a library scan refused
void   launch_sketch_write(const SketchBatch &b, hipStream_t s);

// mm_collect_matches for every read of a batch, from its minimizers (launch_sketch_*) to the arrays launch_collect_seeds reads
struct MatchBatch {
	DevIndexView ix;
	int32_t mid_occ, max_max_occ, occ_dist; float q_occ_frac;
	int64_t n_reads, n_mini;
	const int64_t *seq_off;            // n_reads + 1 (read lengths)
	const ulonglong2 *mini; const int32_t *mini_read; const int64_t *mini_off;
	const int32_t *len0;               // fragments (launch_frag_view ran; then "read" means fragment everywhere here): n_reads, the first mate's length -- a seed at or past it
	                                   // is the second mate's (segment id 1); INT32_MAX for a fragment of one read.  Null: single reads, segment id 0
	// scratch by minimizer (n_mini + 1 entries unless said)
	unsigned long long *skey_in, *skey;    // the reads' x, unsorted / sorted within each read (q-occurrence filter)
	unsigned char *keepq;
	uint32_t *fpos;                    // exclusive scan of keepq
	unsigned long long *fx; uint32_t *fy; int32_t *fread;      // the filtered list
	uint32_t *l_n; long long *l_first; unsigned char *l_tan;   // its look-up
	uint32_t *mpos;                    // exclusive scan of l_n > 0
	uint32_t *m_n, *m_q, *m_span; long long *m_first; int32_t *m_read;   // the matches (m_span: span | tandem << 31)
	int64_t  *moff;                    // n_reads + 1
	uint32_t *low_before, *low_after;  // 1 + the last match at or before with n <= mid_occ; the first one at or after (stored reversed)
	int4     *streaks; int32_t *n_streaks;   // streaks that need a selection: first match, length, K
	unsigned long long *thr;           // by first match of a streak: the K-th smallest (n << 32 | index in the streak)
	unsigned char *flt;
	uint32_t *spos; int64_t *hpos;     // exclusive scans of the kept matches and of their hits
	int64_t  *tot;                     // [0] filtered [1] matches [2] seeds [3] hits
	void     *tmp; size_t tmp_bytes;
	// out
	SeedRecord *seeds; int64_t *seed_off, *hit_off; unsigned long long *hits;
	long long *src_first;              // by seed: where its occurrences begin in ix.where
	unsigned long long *mini_pos; int32_t *rep_len, *qlen;
};
// The mates of a fragment as ONE read of the match selection (map.c:186-200): after the sketch of the batch's sequences, a fragment is the run of sequences
// frag_off[f] .. frag_off[f + 1] (one or two).  A second mate's minimizers get the first mate's length added to their position (y += len0 << 1) and segment id 1
// in y >> 32, every minimizer's owner becomes its fragment, and the per-fragment offsets the match kernels take (bases, minimizers) are read off the per-sequence ones.
struct FragView {
	int64_t n_frag, n_seqs, n_mini;
	const int64_t *frag_off;           // n_frag + 1: first sequence of each fragment; frag_off[n_frag] = n_seqs
	const int64_t *seq_off, *mini_off; // n_seqs + 1, the sketch's
	ulonglong2 *mini; int32_t *mini_read;   // n_mini, rewritten in place
	int64_t *f_seq_off, *f_mini_off;   // out, n_frag + 1
	int32_t *len0;                     // out, n_frag (MatchBatch::len0)
};
void launch_frag_view(const FragView &v, hipStream_t s);

size_t match_layout(MatchBatch &b, void *base);
int    launch_matches_select(const MatchBatch &b, hipStream_t s);  // everything but the hits; tot is final when it is through.  -1: a library call refused
void   launch_matches_gather(const MatchBatch &b, hipStream_t s);  // hits (b.hits sized by tot[3])

} // namespace mm2gb
