// engine.h -- internal: the chaining engine (device arenas, streams, micro-batch pipeline).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <functional>
#include <string>
#include <vector>
#include "../../include/mm2gb_chain.h"
#include "chain_dev.h"
#include "post_dev.h"
#include "seed_dev.h"

namespace mm2gb {

void set_error(const std::string &msg);
// the index's copy on a device, made on first use (seeding.cpp); a device buffer given up without waiting for the device (engine.hip)
int  index_on_device(const mm2gb_index_t *ix, int device, DevIndexView *out);
void retire_device_buffer(void *ptr, size_t bytes);
int  fail(const std::string &msg);            // sets the error text, returns -1

#define MM2GB_HIP(call)                                                                                        \
	do {                                                                                                       \
		hipError_t e_ = (call);                                                                                \
		if (e_ != hipSuccess)                                                                                  \
			return ::mm2gb::fail(std::string(#call) + ": " + hipGetErrorString(e_));                           \
	} while (0)

// One device buffer that only ever grows.
struct DevBuf {
	void  *ptr = nullptr;
	size_t bytes = 0;
	int ensure(size_t need);
	void release();
};

// Buffers replaced by a growth are retired, not freed (engine.hip: hipFree waits for the whole device): this frees them now.
void flush_retired_buffers();

// Page-locked host buffer that only ever grows.
struct PinnedBuf {
	void  *ptr = nullptr;
	size_t bytes = 0;
	int ensure(size_t need);
	void release();
};

// Device-side staging of one host micro-batch: raw anchors + offsets in, f/p out.  Two sets alternate so that the H2D of
// micro-batch k+1, the kernels of k and the D2H of k-1 run at the same time on three streams.
struct IoSet {
	DevBuf raw, offsets, f, p;
	hipEvent_t in_start = nullptr, in_done = nullptr, comp_done = nullptr, out_start = nullptr, out_done = nullptr;
	bool used = false;
};

// Timing + result counters of one enqueued micro-batch (a host call may enqueue several).
struct BatchSlot { hipEvent_t prep0 = nullptr, prep1 = nullptr, score1 = nullptr; };
constexpr int MAX_SLOTS = 256;

struct Engine {
	int device = 0;
	mm2gb_config_t cfg;
	mm2gb_misc_t   misc;
	DevParams      params;
	LaunchCfg      launch;
	hipStream_t    stream = nullptr;       // kernels (== work[0].stream)
	hipStream_t    s_in = nullptr, s_out = nullptr;   // H2D / D2H of the host-buffer paths
	bool           lean_streams = false;   // two HIP streams instead of four: kernels and H2D share one (Engine::init: every engine but the first on its device)
	bool           counted_on_device = false;
	int            n_cu = 256;

	// Work arenas of the kernels of one micro-batch (sized by cap_n / cap_blocks, grow-only).  Two sets, each with its own
	// compute stream: consecutive micro-batches of the host-buffer paths alternate between them, so the tail of micro-batch k
	// (a persistent kernel ends at the pace of its last few chunks) overlaps the body of micro-batch k+1 instead of idling the GPU.
	// Device-pointer calls (mm2gb_score_device) always use set 0 = `stream`.
	struct WorkSet {
		hipStream_t stream = nullptr;
		int64_t cap_n = 0, cap_reads = 0, cap_blocks = 0;
		DevBuf st;
		DevBuf blk_firstcut, blk_pairs, blk_clamped, blk_wmax, blk_read;
		DevBuf chunk_start, chunk_end, chunk_cost, chunk_track, order, long_list, mid_list;
		DevBuf chunk_pp, chunk_kk, chunk_blk, tile_sums, tile_base, bins;
		DevBuf counters, totals, flags;
		DevBuf gang_slots;                    // one chunk on several workgroups (gangs, k_score's phase 0): GANG_MAX_CHUNKS slots
		DevBuf skip_mark;                     // k_skip_fill's marks (lchain.c:175 t[]): 4 B per anchor, allocated when first used
		DevBuf skip_stats;                    // k_skip_fill's counters (SKIP_STAT_WORDS), only with MM2GB_SKIP_STATS=1
		DevBuf band_diag, band_res;           // k_score's band pass (params.band_slab > 0): x - y per anchor 4 B, its result 8 B, allocated when first used
		DevBuf band_ord, band_hdr;            // ... and what a team's slab publishes for its other parts: the targets' order 2 B per anchor, a header word per 128 anchors
		void  *band_hdr_zeroed = nullptr;     // the band_hdr allocation that has been cleared (a grown one is a new, uninitialised buffer)
		size_t band_hdr_zeroed_bytes = 0;
		int    band_epoch = 0;                // the last launch's tag in the header words: a word of an earlier launch never reads as published
		std::vector<DevBuf*> all() { return { &st, &blk_firstcut, &blk_pairs, &blk_clamped, &blk_wmax, &blk_read, &chunk_start, &chunk_end, &chunk_cost,
		                                      &chunk_track, &order, &long_list, &mid_list, &chunk_pp, &chunk_kk, &chunk_blk, &tile_sums, &tile_base, &bins, &counters, &totals, &flags, &gang_slots, &skip_mark, &skip_stats, &band_diag, &band_res, &band_ord, &band_hdr }; }
	};
	WorkSet work[2];
	DevBuf lut, dbg;
	// device post-pass (post_kernels.hip), allocated on first use: 41 B/anchor of work arrays (candidates 8, walk records 8, picked 4, two lifting tables 8, the sort's bytes / permutation / way station 13), + chains' arrays, + outputs
	int64_t cap_post_n = 0, cap_post_reads = 0;
	DevBuf post_dbg_tasks, post_dbg_stasks, rmq_dbg_reads, rmq_skey_in, rmq_skey, rmq_sa, rmq_srange, rmq_sort_tmp, post_z, post_fp, post_picked, post_utmp, post_heads, post_nu, post_nkept, post_misc, post_bins, post_order, post_up4, post_up16, post_sort_s, post_sort_perm, post_sort_tmp, post_cls, post_cls_cnt, post_cls_nz, post_read_nz, post_uloc, post_wtask, post_stask, rmq_tied, rmq_sum, rmq_by_y, rmq_ord, rmq_meta, rmq_win, rmq_tree, reg_out;
	DevBuf sd_seeds, sd_seed_off, sd_hit_off, sd_hits, sd_qlen, sd_q_rank, sd_ref_len, sd_ref_rank, sd_seed_read, sd_tmp, sd_n_kept, sd_a_off, sd_out;   // mm2gb_collect_seeds_gpu
	DevBuf sh_ord, sh_keys, sh_long, sh_sort_tmp, sh_tied;   // mm2gb_collect_seeds_heap_gpu (seed_heap_kernels.hip): the sorted order, the long reads' keys, ranges and sort space, the tie flags
	// sequence bytes -> matches on the device (seed_kernels.hip; mm2gb_sketch_gpu, mm2gb_collect_matches_gpu): the sequences, their offsets and
	// ids, the minimizers with their reads and offsets, one arena for the work arrays of either stage, what the host's mapq / divergence code wants
	DevBuf sk_seqs, sk_seq_off, sk_rid, sk_mini, sk_mini_read, sk_mini_off, sk_work, sd_src_first, sd_mini_pos, sd_rep_len, sk_frag;   // sk_frag: fragments' first sequences, their offsets, first mates' lengths
	// mm_est_err's walk (est_err_kernels.hip; mm2gb_est_err_gpu and the mapper's resident path): the call's arrays as the host gives them (the resident path reads
	// the engine's own instead: reg_out, post_out[0], sd_qlen, sd_seed_off, sd_mini_pos), the reads' hashes of the resident path's hit records, scratch, results
	DevBuf ee_reg_off, ee_a_off, ee_a, ee_qlen, ee_mini_off, ee_mini, ee_ref_len, ee_hash, ee_reg_read, ee_literal, ee_out, ee_sum_k;
	// the extension DP (ksw_kernels.hip; mm2gb_ksw_extd2_gpu): job records, both sequence arrays, result records, the direction bytes of the jobs
	// of one launch, every job's CIGAR words before and after packing, state images too large for LDS, the launches' job counters, the words' offsets
	// kw_junc: the splice-aware DP's annotation bytes, laid out like kw_t (mm2gb_ksw_exts2_gpu)
	DevBuf kw_jobs, kw_q, kw_t, kw_res, kw_slab, kw_cig, kw_img, kw_cnt, kw_off, kw_pack, kw_junc;
	int64_t kw_class_jobs[2] = { 0, 0 };   // since the engine was made: DP jobs launched with their image in LDS / in global memory
	double kw_ms[2] = { 0, 0 };            // of the last call: fill + backtrack kernels, packing kernel
	// the alignment of hits (align_kernels.hip; mm2gb_align_regs_gpu): the batch's resident residues (references, reads), a round's job
	// descriptors, gather slices, the list of gap fills to test and the test's results
	DevBuf al_refs, al_reads, al_jobs, al_slices, al_list, al_drop;
	// the text of the alignment tags (aln_text_kernels.hip; mm2gb_aln_text_gpu): records, words, slices, the slices' counts and carries, their
	// byte counts and destinations, the scan's work space, the text
	DevBuf tx_recs, tx_words, tx_slices, tx_cnt, tx_run, tx_bytes, tx_dest, tx_tmp, tx_text;
	double tx_s[4] = { 0, 0, 0, 0 };       // of the last call: residues up, the host's pass over the words (checks, slices), words up + kernels, text back
	// residues of al_refs / al_reads that the LAST alignment call (mm2gb_align_regs_gpu) or text call uploaded, laid end to end in the call's order:
	// their numbers of bytes, -1 when that call uploaded nothing.  What lets a later step of the same batch use them without uploading again.
	int64_t al_resident[2] = { -1, -1 };
	// what the post-pass leaves for the host, two sets: the boundary keeps two batches in flight (the results of batch k are
	// fetched after batch k+1 has been launched)
	struct PostOut {
		DevBuf u_off, a_off, u_out, a_out;
		int64_t *h_totals = nullptr;       // pinned: [0] chains [1] anchors kept
		hipEvent_t done = nullptr;         // post kernels of the batch that owns this set have finished, totals are in h_totals
	} post_out[2];
	DevBuf &post_uoff = post_out[0].u_off, &post_aoff = post_out[0].a_off, &post_uout = post_out[0].u_out, &post_aout = post_out[0].a_out;
	int64_t *&h_post_totals = post_out[0].h_totals;
	hipEvent_t post0 = nullptr, post1 = nullptr;
	hipEvent_t post_fork = nullptr, post_join = nullptr;   // the classes' pass on the second compute stream beside the lifting tables' (engines with streams of their own)
	IoSet io[2];
	uint64_t io_seq = 0;
	PinnedBuf h_slice_off;                 // per-slice read offsets of mm2gb_score_host
	std::vector<hipEvent_t> slice_in;      // sliced mm2gb_chain_gpu: slice k's anchors have arrived
	PinnedBuf h_res_f, h_res_p;            // scores of whole-batch chaining calls (pool.cpp): page-locked, reused, grow-only
	// per-slot read-back (pinned)
	char    *h_small = nullptr;            // one page-locked block: h_counters, h_totals, both post sets' totals
	int32_t *h_counters = nullptr;         // MAX_SLOTS x CNT_WORDS
	int64_t *h_totals = nullptr;           // MAX_SLOTS x 2
	BatchSlot slots[MAX_SLOTS];
	int n_slots = 0;

	mm2gb_stats_t last = {};
	bool misc_valid = false, coop_disabled = false, debug_phases = false, one_compute_stream = false;
	int64_t sparse_min_n = 0;       // micro-batches from this many anchors on get the planner's sparse list (launch.sparse_max_window)
	int64_t team4_min_n = 0;        // micro-batches from this many anchors on send wide-window heavy chunks to 4-wave teams (launch.team4_share_pct)
	int64_t gang_max_n = 0;         // micro-batches up to this many anchors run the instantiation of k_score with the gang phase
	int64_t last_gang_chunks = 0, last_gang_wgs = 0;        // of the last call: chunks scored by a gang of workgroups, workgroups that started in one
	bool rmq_tiles_last = false;    // which form the last RMQ call ran (for the debug print)
	std::function<void(const int32_t*)> rmq_tied_ready;   // the NEXT device re-chaining call only: called on the calling thread as soon as the fill's tie counts are on the host, while the call's post-pass and copies still run
	hipEvent_t rmq_fill_done = nullptr;
	int  rmq_team_reads = 0;        // tile form, the NEXT device call only: its first reads that get a whole workgroup each (mm2gb_rmq_chain puts the costliest first); MM2GB_RMQ_TEAM_READS overrides
	bool rmq_abandon_tied = false;  // the NEXT device re-chaining call only: give a read up at its first tie (mm2gb_rmq_chain redoes tied reads on the host whatever the device made of them)
	bool rmq_calibrate = false;     // mm2gb_rmq_chain on this engine scales its cost model by the measured / estimated times of earlier calls (rmq_hybrid.cpp)
	int  rmq_kernel = 0;            // device form of the RMQ fill: 0 tiles (k_rmq_fill_tiles), 1 one anchor per step (k_rmq_fill); MM2GB_RMQ_KERNEL=steps|tiles overrides
	bool lds_contract_ok = false;   // this device reads 0 beyond a workgroup's LDS and saturates v_sad_u32 ... clamp (probed in init)
	int64_t dual_stream_max_n = 16 * 1000 * 1000;   // micro-batches up to this many anchors alternate between the two compute streams
	bool chain_skip = false;        // the DP keeps misc.max_skip (k_skip_fill) where the limit can be reached; false: exhaustive (k_score), the default.  MM2GB_CHAIN_SKIP=keep at creation
	int64_t last_sparse_chunks = 0;           // chunks of the planner's sparse list that k_score scored, since the last reset of the stats
	int64_t last_band_groups[2] = { 0, 0 };   // groups of targets k_score's band pass swept in the wave path / the team paths, since the last reset of the stats
	int  last_score_form = 0;       // form of the DP the last enqueued micro-batch ran: 0 exhaustive (k_score), 1 the skip-limited walk (k_skip_fill)
	int  last_score_set = 0, last_score_host_mode = 0;   // work set (whose flag word the device combined with it) and launch.host_mode of the last enqueued micro-batch (mm2gb_engine_last_score_mode)
	bool skip_stats = false;        // MM2GB_SKIP_STATS=1: k_skip_fill counts rounds, targets and its slowest chunk (mm2gb_engine_skip_stats; profiles/skip_rate.py)
	int  last_skip_set = 0;         // work set of the last micro-batch the walk ran on

	int  init(const mm2gb_config_t *cfg, const mm2gb_misc_t *misc, int device);
	void shutdown();
	int  set_misc(const mm2gb_misc_t *m);
	int  configure_score();
	int  reserve(int64_t n_anchors, int64_t n_reads, int set = 0);
	int  begin_call();                     // start of a host-level call: resets slots and `last`
	// host buffers (pinned for true asynchrony): H2D, kernels, D2H enqueued on three streams; returns without waiting
	// want_stats = false: no timing events / counter read-back for this micro-batch (the drop-in boundary keeps two host
	// batches in flight and never asks for statistics)
	int  enqueue_host(int64_t n_reads, const int64_t *h_offsets, const mm2gb_anchor_t *h_anchors, int64_t n, int32_t *h_f, int32_t *h_p, bool want_stats = true);
	int  enqueue(int64_t n_reads, const int64_t *d_offsets, const mm2gb_anchor_t *d_anchors, int64_t n, int32_t *d_f, int32_t *d_p, bool want_stats = true, int set = 0);
	int  score_host(int64_t n_reads, const int64_t *offsets, const mm2gb_anchor_t *anchors, int32_t *f, int32_t *p,
	                const std::function<void(int64_t, int64_t)> *slice_done);   // sliced + overlapped, waits for the end
	// backtrack + compaction of a scored micro-batch on the device (all pointers device pointers; d_f / d_p as enqueue() left
	// them); enqueued on the compute stream.  Results stay in post_uoff / post_aoff / post_uout / post_aout; totals land in
	// h_post_totals once the stream has been synchronised.
	int  reserve_post(int64_t n_anchors, int64_t n_reads);                 // work arrays of the post kernels (shared by both result sets)
	int  reserve_post_out(int set, int64_t n_anchors, int64_t n_reads);    // result buffers of one set; never touches the other
	void print_post_debug(int64_t n_reads);   // MM2GB_DEBUG_PHASES: the last post-pass kernel's records, to stderr
	int  enqueue_post(int64_t n_reads, const int64_t *d_offsets, const mm2gb_anchor_t *d_anchors, int64_t n, const int32_t *d_f, const int32_t *d_p,
	                  const mm2gb_rmq_param_t *rmq = nullptr, int out_set = 0);   // rmq given: thresholds of the re-chaining call (lchain.c:355) instead of misc's
	// the boundary's device post-pass: host anchors in (page-locked), H2D + score kernels + post kernels enqueued, nothing waited
	// for; fetch_chains() waits for that batch and copies its chains out (exact sizes)
	int  enqueue_host_chains(int64_t n_reads, const int64_t *h_offsets, const mm2gb_anchor_t *h_anchors, int64_t n, int out_set, bool want_stats = false);
	int  fetch_chains(int out_set, int64_t n_reads, mm2gb_chains_t *out);
	// whole batch on host buffers, chains back, nothing but the chains crosses the link on the way back
	// rmq given: the score fill is mg_lchain_rmq's (k_rmq_fill) instead of the chaining DP; n_tied (optional, n_reads entries)
	// receives, per read, the number of anchors whose range-minimum was tied (results for such a read are not the reference's)
	int  chain_gpu(int64_t n_reads, const int64_t *offsets, const mm2gb_anchor_t *anchors, mm2gb_chains_t *out,
	               const mm2gb_rmq_param_t *rmq = nullptr, int32_t *n_tied = nullptr);
	int  chain_gpu_sliced(int64_t n_reads, const int64_t *offsets, const mm2gb_anchor_t *anchors, mm2gb_chains_t *out, int64_t slice);
	int  collect_seeds(int64_t opt_flag, int64_t n_reads, const int64_t *seed_off, const mm2gb_seed_t *seeds, const int64_t *hit_off, const uint64_t *hits,
	                   const int32_t *qlen, const int32_t *q_rank, int32_t n_ref, const int32_t *ref_len, const int32_t *ref_rank, int64_t *anchor_off, mm2gb_anchor_t *anchors);
	// collect_seed_hits_heap (seed_heap_kernels.hip): as collect_seeds in the heap's order; reads with two equal cr are done again by the host form
	int  collect_seeds_heap(int64_t opt_flag, int64_t n_reads, const int64_t *seed_off, const mm2gb_seed_t *seeds, const int64_t *hit_off, const uint64_t *hits,
	                        const int32_t *qlen, const int32_t *q_rank, int32_t n_ref, const int32_t *ref_len, const int32_t *ref_rank, int64_t *anchor_off, mm2gb_anchor_t *anchors, int64_t *n_tied_reads);
	// the minimizers of sequences laid end to end, left in sk_mini / sk_mini_read / sk_mini_off (arguments checked by the callers)
	int  sketch_device(int w, int k, int flag, int64_t n_seqs, const int64_t *seq_off, const char *seqs, const uint32_t *rid, int64_t *n_mini);
	// collect_seeds_heap on the matches collect_matches_device left resident (the short-read mapper seeded on the device)
	int  heap_order_on_device(const char *who, int64_t opt_flag, int64_t n_reads, int64_t n_seeds, int64_t n_hits, const int64_t *seed_off, const mm2gb_seed_t *seeds, const int64_t *hit_off,
	                          const uint64_t *hits, const int32_t *qlen, bool names, const int32_t *q_rank, const int32_t *ref_len, const int32_t *ref_rank, int64_t *anchor_off,
	                          mm2gb_anchor_t *anchors, int64_t *n_tied_reads);      // what the two share, on matches that lie on the device
	int  collect_seeds_heap_resident(int64_t opt_flag, int64_t n_reads, int64_t n_seeds, int64_t n_hits, int64_t *anchor_off, mm2gb_anchor_t *anchors, int64_t *n_tied_reads);
	// mm_collect_matches for a batch, left in sd_seeds / sd_seed_off / sd_hit_off / sd_hits (+ sd_qlen, sd_mini_pos, sd_rep_len)
	// frag_off (n_frag + 1, host; null: every sequence a read of its own): the sequences frag_off[f] .. frag_off[f + 1], one or two, are the mates of fragment f, seeded as
	// one list (launch_frag_view); everything left behind is then per fragment -- sd_seed_off, sd_rep_len and sd_qlen have n_frag entries, sd_qlen the mates' summed length
	int  collect_matches_device(const DevIndexView &ix, const mm2gb_seed_opt_t &opt, int64_t n_reads, const int64_t *seq_off, const char *seqs, int64_t *n_seeds, int64_t *n_hits,
	                            int64_t n_frag = 0, const int64_t *frag_off = nullptr);
	// launch_collect_seeds on what collect_matches_device left; q_rank / ref_rank / ref_len as for collect_seeds (null: no name tests).  anchors null: the anchors
	// stay in sd_out / sd_a_off and only the offsets come down (the mapper's resident path)
	int  collect_seeds_resident(int64_t opt_flag, int64_t n_reads, int64_t n_seeds, int64_t n_hits, const int32_t *q_rank, int32_t n_ref, const int32_t *ref_len, const int32_t *ref_rank,
	                            int64_t *anchor_off, mm2gb_anchor_t *anchors);
	// the mapper's resident path on what collect_seeds_resident left: chaining DP, backtrack and compaction on device pointers -- the chains stay in
	// post_out[0]; only their totals come down ...
	int  resident_chain(int64_t n_reads, int64_t n_anchors, int64_t *n_chains, int64_t *n_kept);
	// ... then k_gen_regs and k_est_err on them: hit records, their offsets, the walk's counts and sum_k come down
	int  resident_regs(int64_t n_reads, int64_t n_chains, const uint32_t *hash, int32_t n_ref, const int32_t *ref_len, int64_t *u_off, mm2gb_reg_t *regs, mm2gb_est_err_t *est, uint64_t *sum_k);
	int  est_err(int64_t n_reads, const int64_t *reg_off, const mm2gb_reg_t *regs, const int64_t *anchor_off, const mm2gb_anchor_t *anchors, const int32_t *qlen,
	             const int64_t *mini_off, const uint64_t *mini_pos, int32_t n_ref, const int32_t *ref_len, mm2gb_est_err_t *out, uint64_t *sum_k);
	int  sort_seeds(int64_t n_reads, const int64_t *offsets, mm2gb_anchor_t *anchors);
	int  gen_regs(int64_t n_reads, const mm2gb_chains_t *chains, const int32_t *qlen, const uint32_t *hash, int is_qstrand, mm2gb_reg_t *regs);
	int  record_outputs_done(hipEvent_t ev);   // fires when every D2H enqueued so far has landed
	int  sync();
	int  collect_stats();
};

} // namespace mm2gb

// host_scratch: what the engine's host-side callers keep from call to call (the mapper's and the re-chaining call's large arrays, host_chain.h
// HostScratch): an engine serves one thread at a time, so its scratch needs no lock, and it outlives the threads that use it
struct mm2gb_engine { mm2gb::Engine e; void *host_scratch = nullptr; void (*host_scratch_free)(void*) = nullptr; };

namespace mm2gb {
// pool.cpp: one engine, host buffers in, chains out, post-pass on n_threads host threads overlapped with the device
int chain_batch_on_engine(mm2gb_engine_t *eng, int64_t n_reads, const int64_t *offsets, const mm2gb_anchor_t *anchors, int n_threads, mm2gb_chains_t *out, mm2gb_stats_t *stats);
}
