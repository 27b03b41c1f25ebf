// align_host.h -- internal: what align_host.cpp offers the device form (align_kernels.hip): the batch's context, the jobs of a round and
// the host half of mm_test_zdrop.  Planning, stitching and the per-read steps are the host's in both forms.
#pragma once
#include <vector>
#include "align_cell.h"
#include "ksw_cell.h"

namespace mm2gb {

struct AlCtx {
	mm2gb_align_opt_t opt;
	int k = 0, idx_flag = 0, a = 0, b = 0, ambi = 0, bw = 0, bw_long = 0;      // a, b, ambi: positive; bw, bw_long: mm_align1's (align.c:588-590)
	int8_t mat[25];
	KswConst kc;
	bool sr = false;                           // the short-read form: plan_chain_sr, ungapped first-pass fills, no log-gap term, no update_dp_max
	bool splice = false;                       // the spliced form: kc is ksw_exts2's, and the four numbers below are read
	int noncan = 0, junc_bonus = 0, anchor_ext_len = 0, anchor_ext_shift = 0;
	int32_t n_ref = 0;
	int64_t n_reads = 0;
	std::vector<int64_t> ref_at, read_at;      // n + 1 each: where a sequence's residues begin
	std::vector<uint8_t> refs, reads;          // one residue per base (seq_nt4_table); reads as given, the reverse strand is computed
};

// What a long-read or assembly preset sets on top of mm_mapopt_init (options.c:95-131): one row per name, read by mm2gb_align_opt_init
// (the scores, drops, min_dp_max, max_gap and the two bands) and by mm2gb_map_opt_init_preset (max_gap, the bands, flag, the mid_occ bounds, best_n)
struct PresetRow {
	const char *name;
	int32_t a, b, q, e, q2, e2, zdrop, zdrop_inv, min_dp_max, max_gap, bw, bw_long;
	int64_t map_flag;
	int32_t min_mid_occ, max_mid_occ, best_n;
};
const PresetRow *preset_row(const char *name);     // nullptr: not a name of the table
extern const char *const preset_names;             // the table's names, for error texts

// a base as text -> its residue
inline uint8_t nt4(char ch)
{
	switch (ch) { case 0: case 1: case 2: case 3: return (uint8_t)ch;          // seq_nt4_table (sketch.c) leaves bytes 0..3 as they are
	              case 'A': case 'a': return 0; case 'C': case 'c': return 1; case 'G': case 'g': return 2; case 'T': case 't': case 'U': case 'u': return 3; default: return 4; }
}

// the sequences of a call as residues end to end (ref_at / read_at: n + 1 each, where a sequence's begin), packed on nt host threads
void pack_residues(int32_t n_ref, const char *const *ref_seqs, const int32_t *ref_lens, int64_t n_reads, const char *const *read_seqs, const int32_t *read_lens, int nt,
                   std::vector<int64_t> &ref_at, std::vector<int64_t> &read_at, std::vector<uint8_t> &refs, std::vector<uint8_t> &reads);

// a job of a round with its DP parameters (first pass), and what came of it
struct AlRun {
	AlJob j;
	int32_t w, zdrop, end_bonus, flag;
	int32_t twin;                      // above 0: the job `twin` places before this one IN THE ROUND'S ARRAY has the same two stretches (a chain's second trial) and the
	                                   // device backend uses its bytes.  Holds because a read's jobs enter the round's array contiguous and in plan_chain's order (drive());
	                                   // whoever reorders a round's jobs (a sort by size, say) must carry the link along or the second trial reads another job's bytes
	int32_t ungapped;                  // the short-read form's fill: the first pass is the one-word ungapped alignment (align.c:744-751), not a DP; w, zdrop and flag are the second pass's
	int32_t code;                      // gap fills: mm_test_zdrop's answer for the first pass (0, 1, 2); a second pass ran when it is not 0
	mm2gb_ksw_res_t res;               // of the pass that counts; res.cigar_off: where its words lie in the round's pool
};

// what runs the DP of a round: every job's first pass, mm_test_zdrop for the gap fills, the second pass where it says so
struct AlBackend {
	virtual ~AlBackend() {}
	virtual int run(const AlCtx &ctx, std::vector<AlRun> &runs, std::vector<uint32_t> &pool) = 0;
	double seconds[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
};

// mm_align_pair's rule (align.c:326-328): a stretch over max_sw_mat cells is not run
inline bool al_too_big(const AlCtx &ctx, const AlJob &j) { return (int64_t)j.tlen * j.qlen > ctx.opt.max_sw_mat; }
// the flag, and the drop, of a gap fill's second pass (align.c:757)
inline int al_second_flag(int flag) { return flag & ~MM2GB_KSW_APPROX_MAX; }
inline int al_second_zdrop(const AlCtx &ctx, int code) { return code == 2 ? ctx.opt.zdrop_inv : ctx.opt.zdrop; }
// the second half of mm_test_zdrop (align.c:70-88): the inversion probe where the drop is deep enough, then the code
int  al_zdrop_code(const AlCtx &ctx, const AlJob &j, const AlDrop &d);

// the call behind the public forms: whole_batch: every read in one sequence of rounds (the device form) instead of read by read on n_threads
// threads (the host form).  spl: the spliced calls' options (opt is then &spl->base) with splice_counts (or null); null: the calls that refuse splice.
// single: the _extz calls, which take q == q2 && e == e2 and nothing else, and run the single-affine DP
int  al_align_regs(const char *who, const mm2gb_align_opt_t *opt, const mm2gb_align_splice_opt_t *spl, int k, int idx_flag, int32_t n_ref, const char *const *ref_seqs, const int32_t *ref_lens,
                   int64_t n_reads, const char *const *read_seqs, const int32_t *read_lens, const int64_t *reg_off, const mm2gb_reg_t *regs,
                   const int64_t *anchor_off, const mm2gb_anchor_t *anchors, int n_threads, AlBackend *whole_batch, mm2gb_align_out_t *out, int64_t *splice_counts, bool single = false,
                   int64_t *sr_counts = nullptr, bool sr = false);          // sr: the _sr calls (MM_F_SR), with their counts
// MM2GB_ALIGN_ROUNDS=batch (read at every call): the host forms run the device form's schedule with the host DP behind it
int  al_align_regs_host(const char *who, const mm2gb_align_opt_t *opt, const mm2gb_align_splice_opt_t *spl, int k, int idx_flag, int32_t n_ref, const char *const *ref_seqs,
                        const int32_t *ref_lens, int64_t n_reads, const char *const *read_seqs, const int32_t *read_lens, const int64_t *reg_off, const mm2gb_reg_t *regs,
                        const int64_t *anchor_off, const mm2gb_anchor_t *anchors, int n_threads, mm2gb_align_out_t *out, int64_t *splice_counts, bool single = false,
                        int64_t *sr_counts = nullptr, bool sr = false);

} // namespace mm2gb
