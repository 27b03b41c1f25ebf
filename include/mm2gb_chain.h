/*
 * mm2gb_chain.h -- C ABI of the MI355X-native chaining library (libmm2gb_chain.so).
 *
 * Two layers are exported:
 *   1. the host-independent core declared here (anchors in, per-anchor score/predecessor or finished chains out);
 *   2. the reference's own drop-in boundary (init/chain/finish/free_stream_gpu) declared in mm2gb_plutils.h.
 *
 * Plain C types only: pointers, sizes, PODs.  "Reference" citations are file:line in the mm2-gb checkout.
 */
#ifndef MM2GB_CHAIN_H
#define MM2GB_CHAIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MM2GB_VERSION "0.1-mi355x"

/* One anchor; bit-identical to mm128_t (minimap.h:44):
 *   x = rev<<63 | rid<<32 | ref_pos     y = seg_id<<48 | flags<<40 | q_span<<32 | query_pos   (lchain.c:140-143) */
typedef struct { uint64_t x, y; } mm2gb_anchor_t;

/* Chaining parameter block; field order and types are those of `Misc` (gpu/plutils.h:33-37) so a Misc can be
 * passed by pointer cast.  Values are what build_misc() (map.c:393-426) produces. */
typedef struct {
	int max_iter, max_dist_x, max_dist_y, max_skip, bw, min_cnt, min_score, is_cdna, n_seg;
	float chn_pen_gap, chn_pen_skip;
} mm2gb_misc_t;

/* gpu_config.json, same schema as the reference's presets (gpu/gpu_config.json; parsed at plmem.cu:416-540).
 * Keys that start with "//" are comments.  Unknown keys are ignored.  Fields absent from a file keep their default. */
typedef struct {
	int     num_streams;            /* top level */
	int     min_n;
	int64_t long_seg_buffer_size;
	int64_t max_total_n;            /* may exceed INT32_MAX (plmem.cu:491 reads it as a double) */
	int     max_read;
	int     avg_read_n;             /* optional in the reference schema (plmem.cu:497-539) */
	int     has_max_total_n, has_max_read, has_avg_read_n;
	struct { int blockdim, cut_check_anchors, anchor_per_block; } range_kernel;
	struct { int micro_batch, mid_blockdim, short_griddim, long_griddim, mid_griddim,
	             long_seg_cutoff, mid_seg_cutoff; } score_kernel;
} mm2gb_config_t;

/* Per-call measurements (device times from HIP events on the engine's stream). */
typedef struct {
	int64_t n_anchors, n_reads;
	int64_t n_pairs;            /* sum of predecessor-window sizes == the reference's "anchor pairs" (planalyze.cu:69-83) */
	int64_t n_chunks;           /* independent DP work items found by the planner */
	int64_t n_long_chunks;      /* of those, pipelined over a big team: 8 waves, or a whole workgroup (LDS score ring) */
	int64_t n_mid_chunks;       /* of those, pipelined over a 4-wave team */
	int64_t n_tracked_chunks;   /* of those, run with the max_ii rescue state machine (lchain.c:190-205) */
	int64_t n_clamped_blocks;   /* planner blocks containing a window cut by max_iter (lchain.c:173) */
	float   ms_h2d, ms_prep, ms_score, ms_d2h, ms_total;
	float   ms_post;            /* device post-pass kernels (mm2gb_chain_gpu), 0 when the post-pass ran on the host */
} mm2gb_stats_t;

typedef struct mm2gb_engine mm2gb_engine_t;

/* ---- errors: every int-returning call gives 0 on success, negative on failure; text via mm2gb_last_error() ---- */
const char *mm2gb_last_error(void);
const char *mm2gb_version(void);

/* ---- configuration (replaces plmem_parse_gpu_config / plmem_config_kernels / plmem_config_batch, plmem.cu:373-540) ---- */
void mm2gb_config_defaults(mm2gb_config_t *cfg);                       /* tuned for MI355X, see mm2-gb_amd/mi355x_config.json */
int  mm2gb_config_parse(const char *json_text, mm2gb_config_t *cfg);   /* starts from defaults */
int  mm2gb_config_load(const char *path, mm2gb_config_t *cfg);

/* ---- engine: one per (process, device); owns streams and device arenas (replaces plmem_stream_initialize,
 *      plmem.cu:558-624, and the constant uploads plrange.cu:225-239 / plscore.cu:491-502) ---- */
int  mm2gb_device_count(void);
/* Node awareness (the reference uses device 0 and pins nothing, gpu/plmem.cu:426,462,499).  The NUMA node of a device's PCIe root
 * (/sys/bus/pci/devices/<bdf>/numa_node; -1 unknown) and a move of the CALLING thread -- and of the threads it starts afterwards -- onto the
 * CPUs of that node which the process may use: 0 when nothing changed (node unknown, none of its CPUs usable, MM2GB_NUMA=0), else the
 * CPUs in the new mask.  Pool workers, batcher workers and bench.py's ranks call it before they allocate page-locked staging (first
 * touch then lands on that node).  mm2gb_numa_cpus_for_bdf is the parsing alone, against a given sysfs root (tests use a made-up tree):
 * returns the number of CPUs of the node (cpus[] filled up to max_cpus), 0 when unknown. */
int  mm2gb_device_numa_node(int device);
int  mm2gb_pin_thread_to_device(int device);
int  mm2gb_numa_cpus_for_bdf(const char *bdf, const char *sysfs_root_dir, int32_t *node_out, int32_t *cpus, int32_t max_cpus);
mm2gb_engine_t *mm2gb_engine_create(const mm2gb_config_t *cfg, const mm2gb_misc_t *misc, int device);
void mm2gb_engine_destroy(mm2gb_engine_t *eng);
int  mm2gb_engine_set_misc(mm2gb_engine_t *eng, const mm2gb_misc_t *misc);
/* The chaining DP's skip limit (misc.max_skip, lchain.c:183-187).  keep = 0 (the default): the DP is exhaustive whatever max_skip says,
 * i.e. results are those of max_skip = INT32_MAX.  keep = 1: every later call on this engine (score, chain, sliced, host-buffer and stream
 * paths, mm2gb_lchain_dp) gives mg_lchain_dp's results at misc.max_skip: a skip-limited walk, one wave per planner chunk, runs in place
 * of the exhaustive kernel unless the limit cannot be reached (max_skip >= max_iter).  MM2GB_CHAIN_SKIP=keep|ignore sets the mode an
 * engine starts with (read when it is created).  mm2gb_engine_last_score_form: the form the engine's last call ran, 0 exhaustive,
 * 1 the skip-limited walk.  Stats keep their meaning (n_pairs: the sum of window sizes, not the candidates met). */
int  mm2gb_engine_set_chain_skip(mm2gb_engine_t *eng, int keep);
int  mm2gb_engine_last_score_form(const mm2gb_engine_t *eng);
/* Which build of the exhaustive score kernel did the work of the engine's last micro-batch: 0 the penalty table in LDS, 1 per-pair float
 * penalties, 2 every branch of comput_sc (cDNA, several segments).  It is the host's choice for the current parameters combined with what
 * the range pass found in the anchors, exactly as the kernel combines them: a segment id anywhere in the micro-batch gives 2, a query
 * position too large for the table turns 0 into 1.  Waits for the engine and reads the micro-batch's flag word back; scoring calls carry
 * no cost for it.  Where the skip-limited walk ran (mm2gb_engine_last_score_form == 1) it is the build the exhaustive kernel would have run. */
int  mm2gb_engine_last_score_mode(mm2gb_engine_t *eng);
/* measurement aid: groups of 64 targets that k_score's band pass (far predecessors by diagonal band; MM2GB_BAND, MM2GB_BAND_SLAB,
 * MM2GB_BAND_LAG when the engine is made) swept in the engine's calls since its stats were last reset: out[0] the wave path, out[1] the teams */
int  mm2gb_engine_band_groups(const mm2gb_engine_t *eng, int64_t *out);
/* measurement aid: chunks of the planner's sparse list (stretches of isolated anchors, no window wider than MM2GB_SPARSE_MAX_WINDOW when the
 * engine is made; 0: no such list) that the score kernel scored in the engine's calls since its stats were last reset: the length of the list */
int  mm2gb_engine_sparse_chunks(const mm2gb_engine_t *eng, int64_t *scored);
/* measurement aid: the band pass's shape as the engine's score kernel is configured now: out[0] the slab (0: the band pass is off), out[1..4] the
 * lag of the wave path, the 4-wave teams, the 8-wave teams and whole-workgroup teams (MM2GB_BAND_LAG_WAVE, _TEAM4, _TEAM8, _WG; MM2GB_BAND_LAG
 * sets all four), out[5] the mean window, in anchors, above which a chunk takes the band pass */
int  mm2gb_engine_band_shape(const mm2gb_engine_t *eng, int *out6);
/* measurement aid: with MM2GB_SKIP_STATS=1 set when the engine was made, the skip-limited walk of its last micro-batch counts, and this waits for
 * the engine and gives: [0] walk rounds of 64 candidates, [1] rounds of the max_ii search, [2] targets, [3] the slowest chunk's time and [4] its
 * anchors, [5] the walk's span from the first chunk's start to the last chunk's end; times in ticks of the 100 MHz s_memrealtime clock */
int  mm2gb_engine_skip_stats(mm2gb_engine_t *eng, int64_t *out6);
int  mm2gb_engine_device(const mm2gb_engine_t *eng);
/* compute units of the engine's device, as the launches that size their grids by it count them (-1: null engine) */
int  mm2gb_engine_cu_count(const mm2gb_engine_t *eng);
/* of the engine's last completed call: chunks that a GANG of workgroups scored -- a chunk whose share of the micro-batch's pairs is worth two
 * workgroups or more is cut into strips that several workgroups take in turn (what plscore.cu's long-segment kernel does with one block per
 * segment, plscore.cu:187-290, cannot: a segment there is one block's) -- and the workgroups that started in a gang.  MM2GB_GANG_MAX (default 8,
 * 0 = off) bounds the workgroups per chunk; micro-batches of more than MM2GB_GANG_MAX_ANCHORS anchors (default 150 M) run the kernel without
 * the gang phase: they fill the machine with whole chunks */
void mm2gb_engine_gang_counts(const mm2gb_engine_t *eng, int64_t *chunks, int64_t *workgroups);
int  mm2gb_has_gang_build(void);    /* 1 (round 3: the gang phase was a build option) */
/* make sure arenas can take a micro-batch of this size (grows, never shrinks) */
int  mm2gb_engine_reserve(mm2gb_engine_t *eng, int64_t n_anchors, int64_t n_reads);

/* ---- score generation: range selection + DP (replaces plrange_async_range_selection, plscore_async_*;
 *      call chain plchain.cu:346-461).  Reads are concatenated: read r owns anchors [offsets[r], offsets[r+1]).
 *      f[i]  = best chain score ending at anchor i (lchain.c:202)
 *      p[i]  = distance back to its predecessor, i - j (0 = no predecessor); int32 because the max_ii rescue
 *              (lchain.c:196-201) can reach further than the reference GPU path's uint16 (plmem.cuh:30). ---- */
int mm2gb_score_host(mm2gb_engine_t *eng, int64_t n_reads, const int64_t *offsets, const mm2gb_anchor_t *anchors,
                     int32_t *f, int32_t *p, mm2gb_stats_t *stats);
/* Same, all pointers are DEVICE pointers in the engine's device; enqueued on the engine's compute stream and
 * returns without synchronising.  Use mm2gb_engine_sync() then mm2gb_engine_stats(). */
int mm2gb_score_device(mm2gb_engine_t *eng, int64_t n_reads, const int64_t *d_offsets, const mm2gb_anchor_t *d_anchors,
                       int64_t n_anchors, int32_t *d_f, int32_t *d_p);
int mm2gb_engine_sync(mm2gb_engine_t *eng);
int mm2gb_engine_stats(mm2gb_engine_t *eng, mm2gb_stats_t *stats);
/* HIP stream handle (hipStream_t) the engine launches on -- for callers that time with their own HIP events. */
void *mm2gb_engine_stream(mm2gb_engine_t *eng);
/* time of the score kernels alone for the last mm2gb_score_device call (ms, valid after mm2gb_engine_sync) */
float mm2gb_engine_last_kernel_ms(mm2gb_engine_t *eng);

/* ---- full chaining of a batch on host buffers: scores on the GPU, then backtrack + compaction
 *      (replaces plchain_cal_score_async + plchain_post_gpu_helper, plchain.cu:201-464).
 *      The post-pass starts on each slice of reads as soon as its scores are back, while later slices are on the device.
 *      Outputs are malloc'd by the library: u_off[n_reads+1] indexes u[], a_off[n_reads+1] indexes a[].
 *      Free with mm2gb_chains_free().  Stats of a multi-device call: counts are summed, times are the slowest device's. ---- */
typedef struct {
	int64_t *u_off;   uint64_t *u;            /* chains per read: score<<32 | n_anchors (lchain.c:145) */
	int64_t *a_off;   mm2gb_anchor_t *a;      /* compacted anchors per read, chain by chain (lchain.c:78-111) */
} mm2gb_chains_t;
int  mm2gb_chain_host(mm2gb_engine_t *eng, int64_t n_reads, const int64_t *offsets, const mm2gb_anchor_t *anchors,
                      int n_threads, mm2gb_chains_t *out, mm2gb_stats_t *stats);
void mm2gb_chains_free(mm2gb_chains_t *out);

/* ---- the same with the post-pass on the device too: backtrack (mg_chain_backtrack, lchain.c:27-76) and
 *      compaction (compact_a, lchain.c:78-111) run as kernels behind the score kernel -- one wave per read, the reference's
 *      sort order (radix_sort_128x, ksort.h:98-151) reproduced element for element -- and only chains and compacted anchors
 *      come back over the link.  Same outputs as mm2gb_chain_host, no host threads.  One micro-batch per call.
 *      mm2gb_post_device: the post-pass alone on device-resident scores (as mm2gb_score_device left them); results stay on the
 *      device, the totals and the kernels' time are reported.  Synchronises the engine's stream. ---- */
int  mm2gb_chain_gpu(mm2gb_engine_t *eng, int64_t n_reads, const int64_t *offsets, const mm2gb_anchor_t *anchors,
                     mm2gb_chains_t *out, mm2gb_stats_t *stats);
int  mm2gb_post_device(mm2gb_engine_t *eng, int64_t n_reads, const int64_t *d_offsets, const mm2gb_anchor_t *d_anchors, int64_t n_anchors,
                       const int32_t *d_f, const int32_t *d_p, int64_t *n_chains, int64_t *n_kept, float *ms);
/* the same, enqueued only (mm2gb_post_device_totals waits and reads the totals): the post-pass of batch k on one engine beside the score kernels of
 * batch k+1 on another -- a stream of micro-batches pays the longer of the two, not their sum, where the kernels can share the chip */
int  mm2gb_post_device_enqueue(mm2gb_engine_t *eng, int64_t n_reads, const int64_t *d_offsets, const mm2gb_anchor_t *d_anchors, int64_t n_anchors,
                               const int32_t *d_f, const int32_t *d_p);
int  mm2gb_post_device_totals(mm2gb_engine_t *eng, int64_t *n_chains, int64_t *n_kept, float *ms);
/* a digest of the chains the last post-pass on this engine left on the device (offsets of chains, offsets of anchors, chains, anchors: four
 * position-dependent sums folded on the host), for comparing two settings or builds on batches too large for the oracle */
int  mm2gb_post_device_digest(mm2gb_engine_t *eng, int64_t n_reads, uint64_t *digest);
/* for tests and debugging: the per-anchor scores f[] and predecessor distances p[] (i - predecessor, 0 = none) that the engine's LAST
 * mm2gb_chain_gpu / mm2gb_rmq_chain_gpu call left on the device (n = that call's anchors) */
int  mm2gb_debug_last_fill(mm2gb_engine_t *eng, int64_t n, int32_t *f, int32_t *p);

/* ---- RMQ re-chaining (mg_lchain_rmq, lchain.c:250-369, called per read from post_chaining_helper, map.c:444-456,
 *      on the anchors the first chaining kept, sorted by x).  Parameters in the order of mg_lchain_rmq's argument list.
 *      mm2gb_rmq_chain_gpu: a batch of reads; score fill, backtrack and compaction all on the device.  The reference resolves
 *      ties between equal range-minimum priorities by the shape of its AVL tree (krmq.h:110-147), which no closed form
 *      reproduces: n_tied[r] (optional) counts the anchors of read r where that happened AND the tied elements do not all leave
 *      the anchor with the same score and predecessor (the tile kernel weighs a tie on the spot; the one-anchor-per-step
 *      kernel and MM2GB_RMQ_TIES=strict count every tie); the chains of a read with n_tied[r] != 0 may differ from the reference's
 *      and are for the caller to discard (mm2gb_lchain_rmq does).
 *      max_chn_skip: at or above cap_rmq_size (or INT32_MAX) the inner walk can never be cut short (lchain.c:329-333) and either kernel
 *      form fills the batch; below it the one-anchor-per-step kernel does, whose inner walk meets the candidates in the reference's
 *      order and keeps the skip counter and its marks (round 6; MM2GB_RMQ_SKIP=ignore: exhaustive whatever the value, as before).
 *      mm2gb_rmq_chain: the batch call that is exact for EVERY read with the device carrying the load (csrc/rmq_hybrid.cpp): reads are
 *      dealt between the kernel form and the host form by estimated cost so that both finish together (a read inside a tandem array is
 *      a hundred times the median and would be one wave's alone), both run at the same time, and reads the kernel reports a tie for
 *      are redone by the host form.  where[r] (optional): 0 device, 1 host threads (cost), 2 host threads (tie).
 *      mm2gb_lchain_rmq: one read, signature and ownership of mg_lchain_rmq; answered by the host form below (exact for every read);
 *      with MM2GB_RMQ=gpu by the kernel, and then a read that met a tie is redone by the host form.  The host PROGRAM's mg_lchain_rmq
 *      is never called: the library does not import it. ---- */
typedef struct {
	int max_dist, max_dist_inner, bw, max_chn_skip, cap_rmq_size, min_cnt, min_sc;
	float chn_pen_gap, chn_pen_skip;
} mm2gb_rmq_param_t;
int  mm2gb_rmq_chain_gpu(mm2gb_engine_t *eng, const mm2gb_rmq_param_t *prm, int64_t n_reads, const int64_t *offsets, const mm2gb_anchor_t *anchors,
                         mm2gb_chains_t *out, int32_t *n_tied, mm2gb_stats_t *stats);
typedef struct { int64_t n_device, n_host_cost, n_host_tie; double est_device_s, est_host_s, device_s, host_s, tie_s, total_s; int32_t device_kernel /* 0 tiles, 1 steps */, n_team /* device reads a whole workgroup filled */; } mm2gb_rmq_deal_t;
/* device form of the fill for this engine's later calls: 0 the tile kernel (64 anchors per step of a wave; best where inner windows hold up to a few hundred
 * anchors), 1 one anchor per step (best where they hold many: its inner scan passes blocks over per anchor).  mm2gb_rmq_chain picks per call. */
int  mm2gb_engine_set_rmq_kernel(mm2gb_engine_t *eng, int kind);
/* tile kernel, this engine's NEXT mm2gb_rmq_chain_gpu call only: its first n reads are filled by a whole workgroup each (the sweeps over a tile's inner
 * window shared by its waves) instead of one wave -- for the few reads of a batch that would otherwise set its pace.  mm2gb_rmq_chain sets it. */
int  mm2gb_engine_set_rmq_team_reads(mm2gb_engine_t *eng, int n);
int  mm2gb_rmq_chain(mm2gb_engine_t *eng, const mm2gb_rmq_param_t *prm, int64_t n_reads, const int64_t *offsets, const mm2gb_anchor_t *anchors,
                     int n_threads, mm2gb_chains_t *out, int32_t *where, mm2gb_rmq_deal_t *deal);
/* The same on host threads, O(log n) per anchor, the reference's answer for EVERY read at any max_chn_skip (csrc/rmq_host.cpp): a read
 * is first done with a tournament tree of fixed shape over its anchors' (y, index) ranks, which gives the reference's answer as long as
 * one anchor in range holds the smallest priority, or all that hold it leave the anchor with the same score and predecessor; at the
 * first tie that decides something (which element the reference returns then follows from its tree's shape; with a skip limit: at the
 * first tie) the read is done again with the reference's own tree -- an AVL tree with krmq.h's insertion, deletion, rotation and
 * subtree-minimum rules, on arrays (MM2GB_RMQ_TREE=avl: that tree for every read).  n_tied[r] (may be NULL) = 1 for a read that was
 * done again, else 0: information only, the chains are exact either way. */
int  mm2gb_rmq_chain_host(const mm2gb_rmq_param_t *prm, int64_t n_reads, const int64_t *offsets, const mm2gb_anchor_t *anchors, int n_threads,
                          mm2gb_chains_t *out, int32_t *n_tied);
/* the same for reads that are known to meet a tie (a device call counted it): the reference's tree for every read at once */
int  mm2gb_rmq_chain_host_tied(const mm2gb_rmq_param_t *prm, int64_t n_reads, const int64_t *offsets, const mm2gb_anchor_t *anchors, int n_threads, mm2gb_chains_t *out);
mm2gb_anchor_t *mm2gb_lchain_rmq(int max_dist, int max_dist_inner, int bw, int max_chn_skip, int cap_rmq_size, int min_cnt, int min_sc,
                                 float chn_pen_gap, float chn_pen_skip, int64_t n, mm2gb_anchor_t *a, int *n_u_, uint64_t **_u, void *km);
void mm2gb_lchain_rmq_counts(int64_t *calls, int64_t *tied_calls);   /* single-read calls so far, and how many of them met a tie */

/* ---- the formats either side of the path, on the device with the reference's exact orders:
 *      mm2gb_sort_seeds_gpu: the seed sort of collect_seed_hits (map.c:329): every read's anchors sorted by x IN PLACE exactly as
 *      radix_sort_128x leaves them (order of equal x included), so unsorted seeds can go straight into the chaining calls;
 *      mm2gb_gen_regs_gpu: mm_gen_regs (hit.c:52-88): one hit record per chain -- best score first, ties by the hash of the first
 *      anchor and the read's hash (map.c:590-592), coordinates and fuzzy lengths of hit.c:8-38.  mm2gb_reg_t is the leading
 *      72 bytes of mm_reg1_t (minimap.h:104-119), i.e. everything but the alignment pointer; regs must hold
 *      chains->u_off[n_reads] records.  qlen / hash: one per read. ---- */
typedef struct {
	int32_t id, cnt, rid, score, qs, qe, rs, re, parent, subsc, as, mlen, blen, n_sub, score0;
	uint32_t flags;          /* mm_reg1_t's bit-field word: rev = bit 10 */
	uint32_t hash;
	float div;
} mm2gb_reg_t;
int  mm2gb_sort_seeds_gpu(mm2gb_engine_t *eng, int64_t n_reads, const int64_t *offsets, mm2gb_anchor_t *anchors);
/*      mm2gb_collect_seeds_gpu: collect_seed_hits (map.c:295-331) with skip_seed (map.c:205-227): the matches mm_collect_matches
 *      (seed.c:98) returned for every read -- seeds[] = the leading 16 bytes of each mm_seed_t (mmpriv.h:40-46), read by read
 *      (seed_off: n_reads + 1), hits[] = the arrays mm_seed_t::cr points at, seed by seed (hit_off: n_seeds + 1) -- become anchors
 *      (map.c:311-324), dropped hits removed, every read's anchors sorted as radix_sort_128x leaves them (map.c:329): the input of the
 *      chaining calls.  opt_flag: the MM_F_* bits of mm_mapopt_t::flag that the function looks at (NO_DIAG, NO_DUAL, FOR_ONLY,
 *      REV_ONLY, QSTRAND; others ignored).  qlen: per read.  Name tests (strcmp(qname, name), map.c:211) are given as ranks in one
 *      common order -- q_rank per read, ref_rank per reference sequence, equal names <=> equal ranks; both may be NULL when neither
 *      NO_DIAG nor NO_DUAL is set.  ref_len (per reference sequence) is needed for NO_DIAG and QSTRAND.  anchors must hold
 *      hit_off[n_seeds] elements; anchor_off (n_reads + 1) receives where each read's anchors begin. ---- */
typedef struct { uint32_t n, q_pos, span_flt, seg_tandem; } mm2gb_seed_t;
int  mm2gb_collect_seeds_gpu(mm2gb_engine_t *eng, int64_t opt_flag, int64_t n_reads, const int64_t *seed_off, const mm2gb_seed_t *seeds,
                             const int64_t *hit_off, const uint64_t *hits, const int32_t *qlen, const int32_t *q_rank,
                             int32_t n_ref, const int32_t *ref_len, const int32_t *ref_rank, int64_t *anchor_off, mm2gb_anchor_t *anchors);
int  mm2gb_gen_regs_gpu(mm2gb_engine_t *eng, int64_t n_reads, const mm2gb_chains_t *chains, const int32_t *qlen, const uint32_t *hash,
                        int is_qstrand, mm2gb_reg_t *regs);

/* ---- from sequence to seed matches on the host (csrc/seeding.cpp), the reference's definitions to the letter:
 *      mm2gb_sketch: mm_sketch (sketch.c:77-143): pairs (hash << 8 | span, rid << 32 | last_pos << 1 | strand).  The *_flag forms take
 *      MM2GB_I_HPC (= MM_I_HPC): homopolymer-compressed minimizers (minimap2 -H, preset map-pb) -- one base per run in the k-mer, the span the
 *      bases it covers, k-mers of 256 bases or more left out; the names without _flag are flag 0;
 *      mm2gb_index_*: every minimizer of the reference sequences -> its occurrences in ascending order, what mm_idx_get returns
 *      (index.c:81-98, 213-262); mid_occ as mm_mapopt_update computes it (options.c:78-84, index.c:186-211);
 *      an index OWNS its flag (mm2gb_index_flag): every function that sketches reads for it -- mm2gb_collect_matches, its device form and
 *      mm2gb_map_reads* on either side -- sketches them the way the index was;
 *      mm2gb_collect_matches: mm_collect_matches (seed.c:98-131, with seed.c:5-96) for one read of one segment: the arrays
 *      mm2gb_collect_seeds_gpu takes, plus rep_len and the minimizer positions the host's mapq / divergence estimates use.
 *      Free a matches record with mm2gb_matches_free, a sketch with mm2gb_free.  Sketch, look-up and match collection have a device
 *      form too (below: mm2gb_sketch_gpu, mm2gb_collect_matches_gpu), and so have building the index and mid_occ (mm2gb_index_build_gpu,
 *      mm2gb_index_mid_occ_gpu); the host functions here stay the definition and the default. ---- */
typedef struct mm2gb_index mm2gb_index_t;
typedef struct { int32_t mid_occ, max_max_occ, occ_dist; float q_occ_frac; } mm2gb_seed_opt_t;   /* mm_mapopt_t: mid_occ, max_max_occ, occ_dist, q_occ_frac */
typedef struct {
	int32_t n_seeds, rep_len, n_mini_pos, pad_;
	int64_t n_hits;
	mm2gb_seed_t *seeds;      /* n_seeds */
	uint64_t *hits;           /* n_hits: seed 0's, seed 1's, ... */
	uint64_t *mini_pos;       /* n_mini_pos: q_span << 32 | position of the minimizer's last base (seed.c:125) */
} mm2gb_matches_t;
#define MM2GB_I_HPC 0x1
int  mm2gb_sketch(const char *seq, int32_t len, int w, int k, uint32_t rid, uint64_t **out_xy, int64_t *n_out);
int  mm2gb_sketch_flag(const char *seq, int32_t len, int w, int k, uint32_t rid, int flag, uint64_t **out_xy, int64_t *n_out);
mm2gb_index_t *mm2gb_index_build(int k, int w, int32_t n_seq, const char *const *seqs, const int32_t *lens, int n_threads);
mm2gb_index_t *mm2gb_index_build_flag(int k, int w, int flag, int32_t n_seq, const char *const *seqs, const int32_t *lens, int n_threads);
int  mm2gb_index_flag(const mm2gb_index_t *ix);                                /* the MM2GB_I_* bits it was built with; negative on error */
void mm2gb_index_destroy(mm2gb_index_t *ix);
int64_t mm2gb_index_size(const mm2gb_index_t *ix, int64_t *n_occurrences);     /* distinct minimizers */
int32_t mm2gb_index_mid_occ(const mm2gb_index_t *ix, float mid_occ_frac, int32_t min_mid_occ, int32_t max_mid_occ);
int  mm2gb_collect_seeds_host(int64_t opt_flag, int64_t n_reads, const int64_t *seed_off, const mm2gb_seed_t *seeds, const int64_t *hit_off,
                              const uint64_t *hits, const int32_t *qlen, const int32_t *q_rank, int32_t n_ref, const int32_t *ref_len,
                              const int32_t *ref_rank, int n_threads, int64_t *anchor_off, mm2gb_anchor_t *anchors);   /* = mm2gb_collect_seeds_gpu, on host threads */
int  mm2gb_collect_matches(const mm2gb_index_t *ix, const char *seq, int32_t len, const mm2gb_seed_opt_t *opt, mm2gb_matches_t *out);
/* mm2gb_collect_matches_frag: the same for a fragment of one or two segments seeded as ONE list (map.c:186-200, 663-666; paired ends): every segment sketched by itself,
 * the second one's minimizers moved behind the first's (position + lens[0]) with segment id 1 (mm2gb_seed_t::seg_tandem), and the q-occurrence filter, the tandem
 * test, the streaks of mm_seed_select, rep_len and mini_pos on the joint list of lens[0] + lens[1] bases.  n_segs = 1 is mm2gb_collect_matches. */
int  mm2gb_collect_matches_frag(const mm2gb_index_t *ix, int32_t n_segs, const char *const *seqs, const int32_t *lens, const mm2gb_seed_opt_t *opt, mm2gb_matches_t *out);
void mm2gb_matches_free(mm2gb_matches_t *m);

/* ---- the same stages on the device (csrc/seed_kernels.hip), byte-identical to the host functions above, for a batch of sequences laid
 *      end to end (seq_off: n + 1 entries, seq_off[0] = 0, fewer than 2^31 bases in all):
 *      mm2gb_sketch_gpu: for sequence r exactly the pairs mm2gb_sketch(seqs + seq_off[r], len_r, w, k, rid ? rid[r] : 0) returns, in its
 *      order; mini_off (n_seqs + 1) says where each sequence's pairs begin in *out_xy (malloc'd, free with mm2gb_free); mm2gb_sketch_gpu_flag
 *      likewise equals mm2gb_sketch_flag (a run of equal bases never continues into the next sequence);
 *      mm2gb_index_to_device: the index's copy in a device's memory (keys, first, where, bucket as they are); made on first use otherwise,
 *      released by mm2gb_index_destroy;
 *      mm2gb_collect_matches_gpu: for read r, seeds[seed_off[r] .. seed_off[r+1]), their hits, mini_pos and rep_len[r] are what
 *      mm2gb_collect_matches(ix, read r, opt) returns.  Free the batch with mm2gb_match_batch_free. ---- */
int  mm2gb_sketch_gpu(mm2gb_engine_t *eng, int w, int k, int64_t n_seqs, const int64_t *seq_off, const char *seqs,
                      const uint32_t *rid, int64_t *mini_off, uint64_t **out_xy);
int  mm2gb_sketch_gpu_flag(mm2gb_engine_t *eng, int w, int k, int flag, int64_t n_seqs, const int64_t *seq_off, const char *seqs,
                           const uint32_t *rid, int64_t *mini_off, uint64_t **out_xy);
int  mm2gb_index_to_device(mm2gb_index_t *ix, int device);
typedef struct {
	int64_t n_seeds, n_hits;
	int64_t *seed_off;        /* n_reads + 1 */
	mm2gb_seed_t *seeds;      /* n_seeds, read by read */
	int64_t *hit_off;         /* n_seeds + 1 */
	uint64_t *hits;           /* n_hits */
	uint64_t *mini_pos;       /* n_seeds: as mm2gb_matches_t::mini_pos */
	int32_t *rep_len;         /* n_reads */
} mm2gb_match_batch_t;
int  mm2gb_collect_matches_gpu(mm2gb_engine_t *eng, const mm2gb_index_t *ix, const mm2gb_seed_opt_t *opt, int64_t n_reads,
                               const int64_t *seq_off, const char *seqs, mm2gb_match_batch_t *out);
/* mm2gb_collect_matches_frag_gpu: the sequences frag_off[f] .. frag_off[f + 1] (one or two; frag_off has n_frag + 1 entries, from 0 to n_seqs) are fragment f, and the
 * result is per FRAGMENT (seed_off and rep_len have n_frag entries): what mm2gb_collect_matches_frag returns for it, record for record.  After the sketch one kernel
 * moves the second mates' minimizers and re-labels every minimizer with its fragment; the match kernels then run on per-fragment offsets. */
int  mm2gb_collect_matches_frag_gpu(mm2gb_engine_t *eng, const mm2gb_index_t *ix, const mm2gb_seed_opt_t *opt, int64_t n_seqs, const int64_t *seq_off, const char *seqs,
                                    int64_t n_frag, const int64_t *frag_off, mm2gb_match_batch_t *out);
void mm2gb_match_batch_free(mm2gb_match_batch_t *m);

/* ---- the index built on the device (csrc/index_kernels.hip): the sequences are sketched there in chunks of whole sequences (at most
 *      MM2GB_INDEX_CHUNK_BASES bases, read at call time, default 256 Mbp; a longer sequence is a chunk of its own, one of 2^31 - 1 bases is
 *      refused), the pairs sorted by (x >> 8, y) and the tables made there.
 *      mm2gb_index_build_gpu(_flag): arguments as mm2gb_index_build(_flag).  The host arrays of the result are byte-identical to mm2gb_index_build's, so
 *      every function that takes an index works on it unchanged; the same arrays stay resident on the engine's device as that device's
 *      copy (nothing is uploaded on first use).  NULL on error (a HIP error or no room on the device included): never a host build instead.
 *      mm2gb_index_mid_occ_gpu: the value mm2gb_index_mid_occ returns, the quantile found on the device by an exact radix select over the
 *      resident first[] (uploaded through mm2gb_index_to_device when the index is not resident there); negative on error.
 *      mm2gb_index_view: sizes, parameters and read-only pointers to the host arrays (valid until mm2gb_index_destroy); built_on is the
 *      device of mm2gb_index_build_gpu or -1, uploads counts the host -> device copies made so far.
 *      mm2gb_index_fetch_device: a device's resident arrays copied into buffers of the view's sizes (keys n_keys, first n_keys + 1,
 *      where n_occ, bucket n_bucket); an error when the index is not resident there.
 *      mm2gb_index_build_split: milliseconds of the device build's stages (H2D, sketch, sort, tables, D2H; H2D overlaps the sketch);
 *      zeros for a host-built index. ---- */
typedef struct {
	int64_t n_keys, n_occ, n_bucket;
	int32_t bucket_shift, k, w, built_on;
	int64_t uploads;
	const uint64_t *keys;     /* n_keys */
	const int64_t  *first;    /* n_keys + 1 */
	const uint64_t *where;    /* n_occ */
	const uint32_t *bucket;   /* n_bucket */
} mm2gb_index_view_t;
mm2gb_index_t *mm2gb_index_build_gpu(mm2gb_engine_t *eng, int k, int w, int32_t n_seq, const char *const *seqs, const int32_t *lens);
mm2gb_index_t *mm2gb_index_build_gpu_flag(mm2gb_engine_t *eng, int k, int w, int flag, int32_t n_seq, const char *const *seqs, const int32_t *lens);
int32_t mm2gb_index_mid_occ_gpu(mm2gb_engine_t *eng, const mm2gb_index_t *ix, float mid_occ_frac, int32_t min_mid_occ, int32_t max_mid_occ);
int  mm2gb_index_view(const mm2gb_index_t *ix, mm2gb_index_view_t *out);
int  mm2gb_index_fetch_device(const mm2gb_index_t *ix, int device, uint64_t *keys, int64_t *first, uint64_t *where, uint32_t *bucket);
int  mm2gb_index_build_split(const mm2gb_index_t *ix, double *ms5);

/* ---- reads in, PAF out (csrc/mapper.cpp): seeding on host threads, anchors / chaining / re-chaining / hit records on the
 *      device, primary-secondary decisions, divergence, mapping quality and the PAF line on the host, written from scratch after
 *      mm_map_frag (map.c:630-790) for single-segment reads without base-level alignment.  Options: the fields of mm_mapopt_t this
 *      path looks at, mm2gb_map_opt_init sets the defaults of mm_mapopt_init (options.c:15-75) except max_chain_skip: chaining runs at
 *      max-chain-skip = infinity (the GPU path's contract) unless max_chain_skip is set below INT32_MAX.  paf: malloc'd text, one line per
 *      hit in read order (free with mm2gb_free). ---- */
typedef struct {
	int64_t flag;              /* MM_F_FOR_ONLY | MM_F_REV_ONLY | MM_F_RMQ (the spliced calls refuse it, options.c:173) | MM_F_NO_LJOIN, and in the calls without base-level
	                            * alignment MM_F_NO_DIAG | MM_F_NO_DUAL | MM_F_ALL_CHAINS (read overlap: below, mm2gb_map_opt_init_ava) */
	int32_t seed, mid_occ, min_mid_occ, max_mid_occ, max_max_occ, occ_dist;
	float   mid_occ_frac, q_occ_frac;
	int32_t min_cnt, min_chain_score, bw, bw_long, max_gap, max_gap_ref, max_chain_iter;
	int32_t rmq_inner_dist, rmq_size_cap, rmq_rescue_size;
	float   rmq_rescue_ratio, chain_gap_scale, chain_skip_scale;
	float   mask_level; int32_t mask_len; float pri_ratio; int32_t best_n;
	int32_t host_threads;      /* 0: every CPU the process may use, at most 32 */
	int32_t seeds_on_device;   /* matches -> sorted anchors: 1 on the device, -1 on host threads, 0 by batch size */
	int32_t rechain_on_device; /* mg_lchain_rmq's fill: 0 (default) mm2gb_rmq_chain -- device and host threads at the same time, reads dealt by cost, ties redone on the host; 1 every read on the device first (ties redone on host threads); -1 host threads only */
	int32_t max_chain_skip;    /* mm_mapopt_t::max_chain_skip; INT32_MAX (the default here): chaining and re-chaining exhaustive.  Below it both keep the limit */
	int32_t seeding_on_device; /* 1: sketch, look-up and match selection on the device (mm2gb_collect_matches_gpu's kernels), anchors from the resident matches; 0 (default), -1: on host threads.
	                            * 2 (MM2GB_SEEDING_RESIDENT): as 1, and in the calls without base-level alignment, where the options have neither a re-chaining stage (MM_F_NO_LJOIN, or
	                            * bw_long <= bw) nor MM_F_RMQ, the resident path: anchors, chains and kept anchors never leave the device -- hit records and the divergence walk's counts
	                            * come down.  Where the options do not allow it, and for a batch with more anchors than one chaining micro-batch holds, 2 is 1 */
} mm2gb_map_opt_t;
typedef struct { int64_t n_reads, n_mapped, n_anchors, n_chains, n_rechained, n_rmq_tied; double s_seed, s_anchors, s_chain, s_rechain, s_regs, s_post; } mm2gb_map_stats_t;   /* s_*: seconds per stage */
void mm2gb_map_opt_init(mm2gb_map_opt_t *opt);
/* mm2gb_map_opt_init, then the mapping fields a preset sets (options.c:95-131): "map-ont" and "map-pb" nothing; "map-hifi" / "map-ccs" max_gap = 10000,
 * min_mid_occ = 50, max_mid_occ = 500; "asm5" / "asm10" / "asm20" those and bw = 1000, bw_long = 100000, best_n = 50, flag |= MM_F_RMQ.  max_chain_skip stays
 * what mm2gb_map_opt_init sets.  The index is the caller's: k = 19, w = 19 (asm20: w = 10) for the new names.  Another name: -1 and the error text.
 * MM_F_RMQ (minimap2 --rmq=yes): stage 3 is not the chaining DP; every read's sorted anchors go through mg_lchain_rmq's fill with bw (map.c:690-692;
 * max_gap_ref and max_chain_iter play no part), in the form rechain_on_device selects, ties redone by the host form, then re-chaining with bw_long as always. */
#define MM2GB_F_RMQ 0x80000000LL
int  mm2gb_map_opt_init_preset(mm2gb_map_opt_t *opt, const char *preset);
/* Read against read (minimap2 -x ava-ont / ava-pb, or -X on any option set): seeding and chaining and nothing else.
 *   MM2GB_F_NO_DIAG     a read's hits on a sequence of its own name and length: those on the diagonal are dropped, the others of the same strand carry MM_SEED_SELF (map.c:212-215)
 *   MM2GB_F_NO_DUAL     hits on a sequence whose name is smaller than the read's are dropped: every pair is reported once (map.c:216)
 *   MM2GB_F_NO_LJOIN    no re-chaining stage (map.c:698); honoured by every mapping call
 *   MM2GB_F_ALL_CHAINS  every chain is reported: no primary / secondary decision, no secondaries dropped (map.c:335); every line is tp:A:S with mapping quality 0
 * Names compare as strcmp does (bytes as unsigned char); the calls with base-level alignment refuse NO_DIAG, NO_DUAL and ALL_CHAINS by name.
 * mm2gb_map_opt_init_ava: mm2gb_map_opt_init, then options.c:96-109 for "ava-ont" (the four bits, min_chain_score = 100, pri_ratio = 0, occ_dist = 0, bw = bw_long = 2000; index k = 15,
 * w = 5) or "ava-pb" (the same with bw_long = bw = 500; index k = 19, w = 5, MM2GB_I_HPC); max_chain_skip stays what mm2gb_map_opt_init sets.  Another name: -1 and the error text. */
#define MM2GB_SEEDING_RESIDENT 2
#define MM2GB_F_NO_DIAG    0x001LL
#define MM2GB_F_NO_DUAL    0x002LL
#define MM2GB_F_NO_LJOIN   0x400LL
#define MM2GB_F_ALL_CHAINS 0x800000LL
int  mm2gb_map_opt_init_ava(mm2gb_map_opt_t *opt, const char *preset);
/* Short single-end reads (minimap2 -x sr).  mm2gb_map_opt_init_sr: mm2gb_map_opt_init, then the mapping fields of
 * options.c:133-150 that mm2gb_map_opt_t has room for -- flag |= MM_F_SR | MM_F_FRAG_MODE | MM_F_NO_PRINT_2ND | MM_F_HEAP_SORT, max_gap = 100, bw = bw_long = 100,
 * pri_ratio = 0.5, min_cnt = 2, min_chain_score = 25, best_n = 20, mid_occ = 1000 (fixed: not recomputed from the index); max_chain_skip stays what mm2gb_map_opt_init
 * sets, which is what main.c:316-318 forces under MM_F_SR.  The index is the caller's: k = 21, w = 11, no HPC.  max_occ = 5000 and max_frag_len = 800 have no field here.
 * They go to mm2gb_map_reads_sr (below); mm2gb_map_reads* and the alignment calls refuse the four bits as they always have.
 *   MM2GB_F_HEAP_SORT   anchors in the order collect_seed_hits_heap leaves them (map.c:229-293): mm2gb_collect_seeds_heap_host / _gpu below
 * mm2gb_collect_seeds_heap_host / _gpu: the arguments of mm2gb_collect_seeds_host / _gpu, and the anchors not sorted by x but as the reference's heap merge of the
 * seeds' hit lists leaves them: the forward-strand anchors in ascending cr (the hit as the index holds it), then the reverse-strand ones in ascending cr.  Among EQUAL cr
 * -- one minimizer value at two places of a read: both seeds carry the same list -- the order is the heap's own (ks_heapdown, ksort.h:43-53, moves a child with an equal
 * key up: not seed order).  The host form restates the heap and is the definition.  The device form (csrc/seed_heap_kernels.hip) sorts a read's hits by (cr, seed, k) --
 * one wave in LDS up to 1024 hits, rocprim's segmented radix sort beyond --, which is the heap's order for every read without two equal cr; a read with two is flagged
 * and done again by the host form inside the call, so both forms return the same anchors element for element.  *n_tied_reads (may be NULL): the reads with two equal cr,
 * the same number from both forms.  MM_F_QSTRAND is refused by name (the reference's heap form has no such branch). */
#define MM2GB_F_FRAG_MODE    0x2000LL
#define MM2GB_F_NO_PRINT_2ND 0x4000LL
#define MM2GB_F_HEAP_SORT    0x400000LL
void mm2gb_map_opt_init_sr(mm2gb_map_opt_t *opt);
int  mm2gb_collect_seeds_heap_host(int64_t opt_flag, int64_t n_reads, const int64_t *seed_off, const mm2gb_seed_t *seeds, const int64_t *hit_off,
                                   const uint64_t *hits, const int32_t *qlen, const int32_t *q_rank, int32_t n_ref, const int32_t *ref_len,
                                   const int32_t *ref_rank, int n_threads, int64_t *anchor_off, mm2gb_anchor_t *anchors, int64_t *n_tied_reads);
int  mm2gb_collect_seeds_heap_gpu(mm2gb_engine_t *eng, int64_t opt_flag, int64_t n_reads, const int64_t *seed_off, const mm2gb_seed_t *seeds,
                                  const int64_t *hit_off, const uint64_t *hits, const int32_t *qlen, const int32_t *q_rank,
                                  int32_t n_ref, const int32_t *ref_len, const int32_t *ref_rank, int64_t *anchor_off, mm2gb_anchor_t *anchors, int64_t *n_tied_reads);
/* mm_est_err's walk (esterr.c:30-61) for every hit record of a batch, on host threads (the definition) and on the device (est_err_kernels.hip; equal results):
 * read r owns regs[reg_off[r] .. reg_off[r+1]) -- looked at: as (an index into the read's anchors, which begin at anchor_off[r]), cnt, rid, qs, rs, re and the rev bit --
 * and the minimizer positions mini_pos[mini_off[r] .. mini_off[r+1]) (mm2gb_matches_t::mini_pos).  out[j]: n_match and n_tot after both end increments (esterr.c:60-61), or
 * n_tot = -1 where the walk does not start (no anchors, no minimizers, or the first anchor's position is no minimizer's: esterr.c:36, 45-51) and div stays -1.
 * sum_k[r]: esterr.c:37-38.  The pow of esterr.c:62 stays on the host in both forms: mm2gb_est_err_div(n_match, n_tot, sum_k, n_mini) finishes it. */
typedef struct { int32_t n_match, n_tot; } mm2gb_est_err_t;
int  mm2gb_est_err_host(int64_t n_reads, const int64_t *reg_off, const mm2gb_reg_t *regs, const int64_t *anchor_off, const mm2gb_anchor_t *anchors, const int32_t *qlen,
                        const int64_t *mini_off, const uint64_t *mini_pos, int32_t n_ref, const int32_t *ref_len, int n_threads, mm2gb_est_err_t *out, uint64_t *sum_k);
int  mm2gb_est_err_gpu(mm2gb_engine_t *eng, int64_t n_reads, const int64_t *reg_off, const mm2gb_reg_t *regs, const int64_t *anchor_off, const mm2gb_anchor_t *anchors, const int32_t *qlen,
                       const int64_t *mini_off, const uint64_t *mini_pos, int32_t n_ref, const int32_t *ref_len, mm2gb_est_err_t *out, uint64_t *sum_k);
float mm2gb_est_err_div(int32_t n_match, int32_t n_tot, uint64_t sum_k, int32_t n_mini);
int  mm2gb_map_reads(mm2gb_engine_t *eng, const mm2gb_index_t *ix, int k, const char *const *ref_names, const int32_t *ref_lens, int32_t n_ref,
                     const mm2gb_map_opt_t *opt, int32_t n_reads, const char *const *names, const char *const *seqs, const int32_t *lens,
                     char **paf_out, int64_t *paf_len, mm2gb_map_stats_t *stats);

/* the same over several engines (one per device; reads shard, no exchange): contiguous runs of reads balanced by bases, one host thread per
 * engine, PAF in read order; counts are summed, stage times are the slowest engine's */
int  mm2gb_map_reads_multi(mm2gb_engine_t *const *engines, int n_engines, const mm2gb_index_t *ix, int k, const char *const *ref_names, const int32_t *ref_lens,
                           int32_t n_ref, const mm2gb_map_opt_t *opt, int32_t n_reads, const char *const *names, const char *const *seqs, const int32_t *lens,
                           char **paf_out, int64_t *paf_len, mm2gb_map_stats_t *stats);
/* A run of any size as a stream of batches (role of worker_for's batch rotation, map.c:924-1153): reads cut into chunks of about
 * chunk_bases bases (<= 0: 96 Mbp), every engine's host thread takes the next chunk and maps it from seeding to PAF.  Several engines
 * per device overlap one chunk's host stages with another's kernels; engines on several devices shard the reads.  PAF in read order;
 * stats->s_*: seconds per stage summed over chunks (stages overlap: not wall time). */
int  mm2gb_map_reads_stream(mm2gb_engine_t *const *engines, int n_engines, const mm2gb_index_t *ix, int k, const char *const *ref_names, const int32_t *ref_lens,
                            int32_t n_ref, const mm2gb_map_opt_t *opt, int32_t n_reads, const char *const *names, const char *const *seqs, const int32_t *lens,
                            int64_t chunk_bases, char **paf_out, int64_t *paf_len, mm2gb_map_stats_t *stats);
/* An engine that maps (or re-chains: mm2gb_rmq_chain) keeps the largest host arrays of those calls -- matches, anchors, the re-chaining
 * gathers and the spliced chains, about 70 bytes per anchor of its largest batch so far, several gigabytes at 100 M anchors -- from call to
 * call, because touching fresh pages costs more than filling them.  They go with the engine; this gives the memory back at once. */
int  mm2gb_engine_release_host_scratch(mm2gb_engine_t *eng);

/* ---- several devices in one process: reads are independent, so a batch is dealt to the devices as contiguous
 *      runs of reads with about the same number of anchors; each device has its own engine (arenas, three streams) and host
 *      thread, nothing is exchanged between devices, results come back in read order.  devices == NULL: 0..n_devices-1;
 *      n_devices <= 0: every visible device.  A device id may repeat (two engines sharing one GPU).
 *      mm2gb_pool_score_host: first_read_of_device (optional, n_devices+1 entries) reports how the reads were dealt.
 *      Replaces the reference's one-GPU stream_setup (plmem.cu:370, plchain.cu:299) for hosts that own whole batches. ---- */
typedef struct mm2gb_pool mm2gb_pool_t;
mm2gb_pool_t *mm2gb_pool_create(const mm2gb_config_t *cfg, const mm2gb_misc_t *misc, int n_devices, const int *devices);
void mm2gb_pool_destroy(mm2gb_pool_t *pool);
int  mm2gb_pool_size(const mm2gb_pool_t *pool);
int  mm2gb_pool_device(const mm2gb_pool_t *pool, int k);              /* HIP device of engine k, -1 if out of range */
int  mm2gb_pool_set_misc(mm2gb_pool_t *pool, const mm2gb_misc_t *misc);
int  mm2gb_pool_score_host(mm2gb_pool_t *pool, int64_t n_reads, const int64_t *offsets, const mm2gb_anchor_t *anchors,
                           int32_t *f, int32_t *p, mm2gb_stats_t *stats, int64_t *first_read_of_device);
int  mm2gb_pool_chain_host(mm2gb_pool_t *pool, int64_t n_reads, const int64_t *offsets, const mm2gb_anchor_t *anchors,
                           int n_threads, mm2gb_chains_t *out, mm2gb_stats_t *stats);

/* ---- batch accumulator + dispatcher (role of mm_trbuf_t, mm_trbuf_is_full and the batch rotation of worker_for,
 *      map.c:23-157, 886-922, 1026-1075): feed reads one at a time from any number of host threads; they are grouped into batches
 *      of at most max_total_n x micro_batch anchors / max_read x micro_batch reads (a read that would overflow the batch starts
 *      the next one, as in map.c:887-920; a read larger than the limit is a batch of its own), closed batches are dealt to the
 *      devices' workers as they become free (one engine + one host thread per device, nothing moves between devices), and every
 *      read's chains come back through `done` (called on worker threads, reads of one batch in the order they were added).
 *      min_n (gpu_config.json) routes reads with fewer anchors to a lane of their own -- batched separately, still on the GPU;
 *      there is no CPU fallback.  post_threads > 0: host threads per device for backtrack + compaction, overlapped with the
 *      device; 0: the device post-pass (mm2gb_chain_gpu).  mm2gb_batcher_add blocks while every batch buffer is in flight.
 *      mm2gb_plan_batches: the grouping rule alone, for a sequence of reads added in order by one thread (no GPU needed):
 *      writes the batch id (in order of creation) and lane (0 big, 1 small) of every read, returns the number of batches. ---- */
typedef struct mm2gb_batcher mm2gb_batcher_t;
typedef void (*mm2gb_read_done_fn)(void *user, int64_t read_id, int n_u, const uint64_t *u, int64_t n_a, const mm2gb_anchor_t *a);
#define MM2GB_BATCHER_MAX_ENGINES 16
typedef struct {
	int64_t reads, anchors;
	int64_t reads_per_lane[2], batches[2];                         /* [0] reads of at least min_n anchors, [1] smaller ones */
	int64_t batches_per_engine[MM2GB_BATCHER_MAX_ENGINES];
	int     n_engines;
} mm2gb_batcher_stats_t;
mm2gb_batcher_t *mm2gb_batcher_create(const mm2gb_config_t *cfg, const mm2gb_misc_t *misc, int n_devices, const int *devices,
                                      int post_threads, mm2gb_read_done_fn done, void *user);
int  mm2gb_batcher_add(mm2gb_batcher_t *b, int64_t read_id, const mm2gb_anchor_t *a, int64_t n);
/* the reads of a packed batch added one at a time by n_producers threads of the library (read r gets the id first_id + r) */
int  mm2gb_batcher_feed(mm2gb_batcher_t *b, int64_t n_reads, int64_t first_id, const int64_t *offsets, const mm2gb_anchor_t *anchors, int n_producers);
int  mm2gb_batcher_flush(mm2gb_batcher_t *b);                     /* close the partial batches, wait until every read is delivered */
int  mm2gb_batcher_stats(mm2gb_batcher_t *b, mm2gb_batcher_stats_t *out);
void mm2gb_batcher_destroy(mm2gb_batcher_t *b);
int64_t mm2gb_plan_batches(int64_t n_reads, const int64_t *n_anchors, int64_t max_total_n, int max_read, int min_n,
                           int32_t *batch_of_read, int32_t *lane_of_read);

/* ---- host post-pass on given f / relative p for ONE read (restates mg_chain_backtrack + compact_a,
 *      lchain.c:27-111, including the radix_sort_128x order, ksort.h:98-151).  Returns number of chains;
 *      *u_out / *a_out are malloc'd (NULL when 0).  Exposed for tests and for hosts that keep their own loop. ---- */
int  mm2gb_backtrack_host(const mm2gb_misc_t *misc, int64_t n, const mm2gb_anchor_t *a, const int32_t *f, const int32_t *p_rel,
                          uint64_t **u_out, mm2gb_anchor_t **a_out);
void mm2gb_free(void *ptr);

/* ---- synchronous single-read entry with the signature of mg_lchain_dp (mmpriv.h:84-85, lchain.c:148-149):
 *      consumes a[] (freed with the host's kfree when linked into minimap2, free() otherwise), returns the compacted
 *      anchors and *_u allocated the same way.  max_skip is ignored (the DP is exhaustive, == INT32_MAX) unless the engines were
 *      created with MM2GB_CHAIN_SKIP=keep: then it is kept as mg_lchain_dp keeps it. ---- */
mm2gb_anchor_t *mm2gb_lchain_dp(int max_dist_x, int max_dist_y, int bw, int max_skip, int max_iter, int min_cnt, int min_sc,
                                float chn_pen_gap, float chn_pen_skip, int is_cdna, int n_seg, int64_t n, mm2gb_anchor_t *a,
                                int *n_u_, uint64_t **_u, void *km);

/* ---- deterministic synthetic reads for benchmarks (SURVEY 8d recipe; xorshift64* seeded per read id).
 *      Two-call protocol: count, then fill.  len_lo/len_hi in bases. ---- */
int64_t mm2gb_synth_count(uint64_t seed, int64_t first_read, int64_t n_reads, int len_lo, int len_hi, int64_t *offsets /* n_reads+1 */);
int     mm2gb_synth_fill(uint64_t seed, int64_t first_read, int64_t n_reads, int len_lo, int len_hi, const int64_t *offsets,
                         mm2gb_anchor_t *anchors, int n_threads);

/* ---- base-level DP, batched: the dual-affine banded extension alignment align.c calls for every stretch between and beyond
 *      anchors at the long-read presets (ksw2's ksw_extd2_sse, ksw2_extd2_sse.c), field for field and CIGAR word for CIGAR word.
 *      A job aligns queries[q_off .. q_off+qlen) against targets[t_off .. t_off+tlen), residues 0..m-1 (m-1 the wildcard); w < 0: no band,
 *      zdrop < 0: no drop.  flag: the MM2GB_KSW_* bits below (= KSW_EZ_*); any other bit is refused by name.  Refused, with the error
 *      text set and nothing run: a flag outside the list, a residue >= m, a job with qlen * tlen > MM2GB_KSW_MAX_CELLS (mm_align_pair's
 *      max_sw_mat).  A job the reference returns from at once (m <= 1, an empty side, -min(mat) > 2(q+e)) gives the reset record.
 *      res[j].cigar_off / n_cigar say where job j's words (len << 4 | op; 0 M, 1 I, 2 D) lie in *cigar (malloc'd, free with mm2gb_free,
 *      NULL when the batch has none).  The host form is the definition; the device form (csrc/ksw_kernels.hip) equals it. ---- */
#define MM2GB_KSW_SCORE_ONLY   0x01
#define MM2GB_KSW_RIGHT        0x02
#define MM2GB_KSW_GENERIC_SC   0x04
#define MM2GB_KSW_APPROX_MAX   0x08
#define MM2GB_KSW_APPROX_DROP  0x10
#define MM2GB_KSW_EXTZ_ONLY    0x40
#define MM2GB_KSW_REV_CIGAR    0x80
#define MM2GB_KSW_NEG_INF      (-0x40000000)
#define MM2GB_KSW_MAX_CELLS    100000000LL
typedef struct { int8_t m, mat[25], q, e, q2, e2; } mm2gb_ksw_param_t;                      /* 0 <= m <= 5; mat: m x m, row = target residue */
typedef struct { int64_t q_off, t_off; int32_t qlen, tlen, w, zdrop, end_bonus, flag; } mm2gb_ksw_job_t;
typedef struct { int32_t max, zdropped, max_q, max_t, mqe, mqe_t, mte, mte_q, score, reach_end, n_cigar, pad_; int64_t cigar_off; } mm2gb_ksw_res_t;
int  mm2gb_ksw_extd2_host(const mm2gb_ksw_param_t *param, int64_t n_jobs, const mm2gb_ksw_job_t *jobs, const uint8_t *queries, const uint8_t *targets,
                          int n_threads, mm2gb_ksw_res_t *res, uint32_t **cigar, int64_t *n_cigar_total);
int  mm2gb_ksw_extd2_gpu(mm2gb_engine_t *eng, const mm2gb_ksw_param_t *param, int64_t n_jobs, const mm2gb_ksw_job_t *jobs, const uint8_t *queries,
                         const uint8_t *targets, mm2gb_ksw_res_t *res, uint32_t **cigar, int64_t *n_cigar_total);
/* the device form's seams, for tests: [0..2] threads of a workgroup per band class, [3..4] the widest band (rounded, in cells) of the first
 * two classes, [5] the largest state image (bytes) kept in LDS -- a larger one lives in global memory; ms2 (optional): the last call's
 * kernel time, [0] fill + backtrack, [1] CIGAR packing */
int  mm2gb_ksw_gpu_info(mm2gb_engine_t *eng, int64_t *consts6, double *ms2);
/* jobs2: the DP jobs the engine has launched since it was made (by either form of the DP, through any call) with their state image
 * [0] in LDS, [1] in global memory (the class of a job whose image, proportional to its target, does not fit) */
int  mm2gb_ksw_gpu_class_jobs(mm2gb_engine_t *eng, int64_t *jobs2);

/* ---- single-affine DP, batched: ksw2's ksw_extz2_sse (ksw2_extz2_sse.c, its SSE2 build), the DP mm_align_pair runs when
 *      q == q2 && e == e2 (align.c:331) -- one gap cost, the same band, z-drop, end bonus and flags -- field for field and CIGAR word for
 *      CIGAR word.  Jobs, results, flags and word array are those of the extd2 calls above.  Of the parameter record only m, mat, q and e
 *      are read; q2 and e2 are IGNORED.  Refused, error text set and nothing run, by both forms: what the extd2 calls refuse (the splice
 *      flag bits by name), q <= 0, e <= 0, 2(q + e) > 127 (options.c:205, 215), and with m == 1 a residue other than 0.  The reset record
 *      and no words: m <= 0, an empty side, -min(mat) > 2(q + e), the minimum taken from mat[1] on whatever m is.  m == 1 is NOT an early
 *      return here.  The host form is the definition; the device form (csrc/ksw_kernels.hip, the same fill kernel in a third form) equals it. ---- */
int  mm2gb_ksw_extz2_host(const mm2gb_ksw_param_t *param, int64_t n_jobs, const mm2gb_ksw_job_t *jobs, const uint8_t *queries, const uint8_t *targets,
                          int n_threads, mm2gb_ksw_res_t *res, uint32_t **cigar, int64_t *n_cigar_total);
int  mm2gb_ksw_extz2_gpu(mm2gb_engine_t *eng, const mm2gb_ksw_param_t *param, int64_t n_jobs, const mm2gb_ksw_job_t *jobs, const uint8_t *queries,
                         const uint8_t *targets, mm2gb_ksw_res_t *res, uint32_t **cigar, int64_t *n_cigar_total);

/* ---- splice-aware DP, batched: ksw2's ksw_exts2_sse (ksw2_exts2_sse.c), the alignment of a cDNA / RNA read's stretches across
 *      introns -- one short gap (q, e), one long gap on the target side only (q2, no extension cost) that opens at donor[] and closes at
 *      acceptor[] -- field for field and CIGAR word for CIGAR word.  Jobs and results are those of the extd2 calls above; the reference's
 *      function has no band and no end bonus, so a job's w and end_bonus are NOT read, and reach_end is always 0.  Words may carry
 *      operation 3 (N).  flag: the seven bits above plus the three below; any other bit is refused by name or value.  junc (may be NULL):
 *      one byte per target residue, indexed like targets (t_off + position), bits 1 / 2 / 4 / 8 = annotated donor / acceptor on the forward
 *      strand, acceptor / donor on the reverse, each worth junc_bonus.  The signal codes are the literal residues 0..3 = A C G T whatever m is.
 *      Refused, error text set and nothing run, by both forms: null arguments, m outside 0..5, a residue >= m, qlen * tlen >
 *      MM2GB_KSW_MAX_CELLS, negative lengths or offsets, e <= 0 (the reference divides by e; checked BEFORE the early return q2 <= q + e),
 *      q < 0, q2 < 0, q + e > 127, noncan or junc_bonus outside 0..127 (then each of -noncan, -noncan / 2 and 0, with or without
 *      junc_bonus added, is an int8_t without wrapping).  The reset record and no words: m <= 1, an empty side, q2 <= q + e,
 *      -min(mat) > 2(q + e).  The host form is the definition; the device form (csrc/ksw_kernels.hip) equals it. ---- */
#define MM2GB_KSW_SPLICE_FOR   0x100
#define MM2GB_KSW_SPLICE_REV   0x200
#define MM2GB_KSW_SPLICE_FLANK 0x400
typedef struct { int8_t m, mat[25], q, e, q2, noncan, junc_bonus; } mm2gb_ksw_splice_param_t;
int  mm2gb_ksw_exts2_host(const mm2gb_ksw_splice_param_t *param, int64_t n_jobs, const mm2gb_ksw_job_t *jobs, const uint8_t *queries, const uint8_t *targets,
                          const uint8_t *junc, int n_threads, mm2gb_ksw_res_t *res, uint32_t **cigar, int64_t *n_cigar_total);
int  mm2gb_ksw_exts2_gpu(mm2gb_engine_t *eng, const mm2gb_ksw_splice_param_t *param, int64_t n_jobs, const mm2gb_ksw_job_t *jobs, const uint8_t *queries,
                         const uint8_t *targets, const uint8_t *junc, mm2gb_ksw_res_t *res, uint32_t **cigar, int64_t *n_cigar_total);

/* ---- base-level alignment of hits, batched: mm_align_skeleton (align.c:960-1020) for every read of a batch -- which stretches
 *      between and beyond a chain's anchors are aligned, how ends are extended, when a hit is split at a z-drop and when an inversion is
 *      tried, then mm_filter_regs, mm_update_dp_max and mm_hit_sort -- record for record and CIGAR word for CIGAR word.
 *      Options: the fields of mm_mapopt_t those functions read; mm2gb_align_opt_init sets options.c's values for "map-ont", "map-pb",
 *      "map-hifi" (= "map-ccs"), "asm5", "asm10" or "asm20".
 *      Input per read: the sequence as text, the hit records as map.c has them when it calls align_regs (regs[reg_off[r] .. reg_off[r+1]),
 *      `as` counted within the read's anchors) and the read's anchors, not yet squeezed (mm_squeeze_a is part of the call).  k and
 *      idx_flag (MM2GB_I_HPC) are the index's, for mm_adjust_minier.  Reference sequences as text.
 *      Output (malloc'd, free with mm2gb_align_out_free): the records after the call with their own reg_off, one mm2gb_aln_t per record
 *      (mm_extra_t without the words; cigar_off = -1 and zeros for a record without one) and the batch's CIGAR words.
 *      Refused, with the error text set, nothing run and *out zeroed: MM_F_SPLICE, MM_F_SR, MM_F_QSTRAND, MM_F_EQX; q == q2 && e == e2
 *      (that path is ksw_extz2_sse: the _extz pair below takes it); max_sw_mat <= 0 or above MM2GB_KSW_MAX_CELLS; a record whose as + cnt
 *      leaves its read's anchors; multi-segment reads (a record marked seg_split or an anchor of a segment other than 0).
 *      The host form is the definition; the device form (csrc/align_kernels.hip) equals it.  counts (information): see MM2GB_ALN_N_* .
 *      mm2gb_align_regs_extz_host / _gpu: the same call for an option set with q == q2 && e == e2 (minimap2 -O4 -E2: one number to -O
 *      and one to -E; main.c:304-309), where mm_align_pair runs ksw_extz2_sse (align.c:331) -- every stretch goes through the
 *      single-affine DP above, and nothing else differs: the region arithmetic, mm_update_extra's gap score and the inversion test read
 *      q and e.  They refuse q != q2 || e != e2 (that is the pair without _extz), 2(q + e) > 127, and whatever the pair above refuses. ---- */
#define MM2GB_F_SPLICE      0x080LL
#define MM2GB_F_SR          0x1000LL
#define MM2GB_F_FOR_ONLY    0x100000LL
#define MM2GB_F_REV_ONLY    0x200000LL
#define MM2GB_F_EQX         0x4000000LL
#define MM2GB_F_NO_END_FLT  0x10000000LL
#define MM2GB_F_QSTRAND     0x100000000LL
#define MM2GB_F_NO_INV      0x200000000LL
/* flag: mm_mapopt_t's one flag word.  mm2gb_align_opt_init leaves the asm presets' MM2GB_F_RMQ (0x80000000) in it, as mm_set_opt does; the alignment
 * calls ignore that bit, but the spliced option set must not carry it into a mapping call (the _splice mapper calls refuse MM_F_RMQ). */
typedef struct {
	int64_t flag, max_sw_mat;
	int32_t a, b, q, e, q2, e2, sc_ambi, zdrop, zdrop_inv, end_bonus;
	int32_t min_dp_max, min_ksw_len, bw, bw_long, max_gap, min_cnt, min_chain_score, rank_min_len;
	float   max_clip_ratio, rank_frac;
} mm2gb_align_opt_t;
typedef struct { int32_t dp_score, dp_max, dp_max2, n_ambi, trans_strand, n_cigar; int64_t cigar_off; } mm2gb_aln_t;
/* counts[]: what the call met, summed over the batch */
enum { MM2GB_ALN_N_GAP_SKIPPED, MM2GB_ALN_N_FILL_ONE_PASS, MM2GB_ALN_N_FILL_TWO_PASS, MM2GB_ALN_N_SPLIT, MM2GB_ALN_N_READS_3_ROUNDS, MM2GB_ALN_N_SPLIT_REFUSED,
       MM2GB_ALN_N_INV, MM2GB_ALN_N_LEFT_END, MM2GB_ALN_N_LEFT_SHORT, MM2GB_ALN_N_RIGHT_END, MM2GB_ALN_N_RIGHT_SHORT, MM2GB_ALN_N_LEFT_AT_0,
       MM2GB_ALN_N_REV_CHAIN, MM2GB_ALN_N_SEAM_MERGED, MM2GB_ALN_N_LEAD_GAP_CUT, MM2GB_ALN_N_FILTERED, MM2GB_ALN_N_DP_MAX_REWRITTEN, MM2GB_ALN_N_OVER_SW_MAT,
       MM2GB_ALN_N_ROUNDS, MM2GB_ALN_N_HPC_MOVED, MM2GB_ALN_N_INV_PROBE_HIT, MM2GB_ALN_N_JOBS, MM2GB_ALN_N_CELLS, MM2GB_ALN_N_CELLS_DISCARDED, MM2GB_ALN_N_COUNTS };
typedef struct {
	int64_t n_regs, n_cigar;
	int64_t *reg_off;          /* n_reads + 1 */
	mm2gb_reg_t *regs;         /* n_regs */
	mm2gb_aln_t *aln;          /* n_regs */
	uint32_t *cigar;           /* n_cigar */
	int64_t counts[MM2GB_ALN_N_COUNTS];
	double  seconds[8];        /* device form: upload, planning, gather, first pass, test, second pass, copies back, stitching and extras */
} mm2gb_align_out_t;
int  mm2gb_align_opt_init(mm2gb_align_opt_t *opt, const char *preset);
int  mm2gb_align_regs_host(const mm2gb_align_opt_t *opt, int k, int idx_flag, int32_t n_ref, const char *const *ref_seqs, const int32_t *ref_lens,
                           int64_t n_reads, const char *const *read_seqs, const int32_t *read_lens, const int64_t *reg_off, const mm2gb_reg_t *regs,
                           const int64_t *anchor_off, const mm2gb_anchor_t *anchors, int n_threads, mm2gb_align_out_t *out);
int  mm2gb_align_regs_gpu(mm2gb_engine_t *eng, const mm2gb_align_opt_t *opt, int k, int idx_flag, int32_t n_ref, const char *const *ref_seqs, const int32_t *ref_lens,
                          int64_t n_reads, const char *const *read_seqs, const int32_t *read_lens, const int64_t *reg_off, const mm2gb_reg_t *regs,
                          const int64_t *anchor_off, const mm2gb_anchor_t *anchors, mm2gb_align_out_t *out);
int  mm2gb_align_regs_extz_host(const mm2gb_align_opt_t *opt, int k, int idx_flag, int32_t n_ref, const char *const *ref_seqs, const int32_t *ref_lens,
                                int64_t n_reads, const char *const *read_seqs, const int32_t *read_lens, const int64_t *reg_off, const mm2gb_reg_t *regs,
                                const int64_t *anchor_off, const mm2gb_anchor_t *anchors, int n_threads, mm2gb_align_out_t *out);
int  mm2gb_align_regs_extz_gpu(mm2gb_engine_t *eng, const mm2gb_align_opt_t *opt, int k, int idx_flag, int32_t n_ref, const char *const *ref_seqs, const int32_t *ref_lens,
                               int64_t n_reads, const char *const *read_seqs, const int32_t *read_lens, const int64_t *reg_off, const mm2gb_reg_t *regs,
                               const int64_t *anchor_off, const mm2gb_anchor_t *anchors, mm2gb_align_out_t *out);
void mm2gb_align_out_free(mm2gb_align_out_t *out);

/* ---- spliced alignment of hits, batched: mm_align_skeleton under MM_F_SPLICE -- the end filter of
 *      mm_fix_bad_ends_splice, every stretch through ksw_exts2 (above), no inversions, and with MM_F_SPLICE_FOR and MM_F_SPLICE_REV both
 *      set every chain aligned once per transcript strand, the larger dp_score kept (trans_strand 1 / 2; 3 on a tie, where the trial
 *      (qlen + dp_score) & 1 is kept).  A second set of calls on the records of the calls above, which keep refusing MM_F_SPLICE.
 *      mm2gb_align_splice_opt_init sets options.c's values for "splice", "cdna" (the same) or "splice:hq", with ONE departure: the preset's
 *      max_sw_mat = 0 (no limit) is MM2GB_KSW_MAX_CELLS here, mm_mapopt_init's own default.  max_sw_mat outside 1 .. MM2GB_KSW_MAX_CELLS is
 *      refused as above and a stretch over it gives the reset record with zdropped = 1 (mm_align_pair's rule); the reference equals these
 *      calls when it runs with the same value (--cap-sw-mem=100000000 after -x splice).
 *      Flags honoured: MM_F_SPLICE_FOR alone, MM_F_SPLICE_REV alone (one trial, align.c:997-1000), both, MM_F_SPLICE_FLANK, MM_F_NO_END_FLT,
 *      MM_F_FOR_ONLY, MM_F_REV_ONLY; FOR or REV implies SPLICE (options.c:70-71).  Junction annotation is absent (no --junc-bed), which
 *      equals the zero bytes mm_idx_bed_junc gives without one.
 *      Refused by name, error text set, nothing run and *out zeroed: a flag word without MM_F_SPLICE, MM_F_SR, MM_F_QSTRAND, MM_F_EQX;
 *      e <= 0; an index with MM2GB_I_HPC; gap penalties, noncan or junc_bonus that mm2gb_ksw_exts2_* refuses; and what the calls above
 *      refuse about max_sw_mat, records, anchors and segments.  splice_counts (may be NULL): the paths met, see MM2GB_SPL_N_*; the
 *      MM2GB_ALN_N_* counts in *out are those of the trials kept, except jobs, cells and cells_discarded, which count every trial.
 *      The host form is the definition; the device form equals it: the two trials of a chain are two DP jobs on the same gathered bytes. ---- */
#define MM2GB_F_SPLICE_FOR   0x100LL
#define MM2GB_F_SPLICE_REV   0x200LL
#define MM2GB_F_SPLICE_FLANK 0x40000LL
typedef struct { mm2gb_align_opt_t base; int32_t noncan, junc_bonus, anchor_ext_len, anchor_ext_shift; } mm2gb_align_splice_opt_t;
/* trial_*: which trial a chain's record came from (for = trial 0); end_flt_*: an anchor dropped at the head / tail, or the probe run and the
 * anchor kept; *_intron: an N in the words of a left extension, a right extension, a gap fill (trials kept); tail_other_strand: a split-off
 * tail whose trans_strand differs from the record before it; n_seam_merged: two N words merged where two stretches meet;
 * noncanonical_intron: an N of a finished record whose ends are neither GT..AG nor CT..AC; single_trial: chains aligned once */
enum { MM2GB_SPL_N_TRIAL_FOR_WON, MM2GB_SPL_N_TRIAL_REV_WON, MM2GB_SPL_N_TRIAL_TIE_KEPT_0, MM2GB_SPL_N_TRIAL_TIE_KEPT_1, MM2GB_SPL_N_END_FLT_HEAD, MM2GB_SPL_N_END_FLT_TAIL,
       MM2GB_SPL_N_END_FLT_PROBE_KEPT, MM2GB_SPL_N_LEFT_EXT_INTRON, MM2GB_SPL_N_RIGHT_EXT_INTRON, MM2GB_SPL_N_FILL_INTRON, MM2GB_SPL_N_FILL_TWO_PASS, MM2GB_SPL_N_SPLIT,
       MM2GB_SPL_N_TAIL_OTHER_STRAND, MM2GB_SPL_N_N_SEAM_MERGED, MM2GB_SPL_N_NONCANONICAL_INTRON, MM2GB_SPL_N_SINGLE_TRIAL, MM2GB_SPL_N_REV_CHAIN, MM2GB_SPL_N_OVER_SW_MAT,
       MM2GB_SPL_N_COUNTS };
int  mm2gb_align_splice_opt_init(mm2gb_align_splice_opt_t *opt, const char *preset);
int  mm2gb_align_regs_splice_host(const mm2gb_align_splice_opt_t *opt, int k, int idx_flag, int32_t n_ref, const char *const *ref_seqs, const int32_t *ref_lens,
                                  int64_t n_reads, const char *const *read_seqs, const int32_t *read_lens, const int64_t *reg_off, const mm2gb_reg_t *regs,
                                  const int64_t *anchor_off, const mm2gb_anchor_t *anchors, int n_threads, mm2gb_align_out_t *out, int64_t *splice_counts);
int  mm2gb_align_regs_splice_gpu(mm2gb_engine_t *eng, const mm2gb_align_splice_opt_t *opt, int k, int idx_flag, int32_t n_ref, const char *const *ref_seqs,
                                 const int32_t *ref_lens, int64_t n_reads, const char *const *read_seqs, const int32_t *read_lens, const int64_t *reg_off,
                                 const mm2gb_reg_t *regs, const int64_t *anchor_off, const mm2gb_anchor_t *anchors, mm2gb_align_out_t *out, int64_t *splice_counts);

/* ---- the text of a PAF line's alignment tags, batched: for record i the bytes text[text_off[i] .. text_off[i+1]) are what
 *      mm_write_paf3 appends after rl:i (format.c:322-329): "\tcg:Z:" and "%d%c" per CIGAR word with MM2GB_TEXT_CG, then "\tcs:Z:..." with
 *      MM2GB_TEXT_CS (the long form, =ACGT instead of :n, with MM2GB_TEXT_CS_LONG as well) or "\tMD:Z:..." with MM2GB_TEXT_MD (write_cs_core,
 *      write_MD_core, format.c:141-218); with both CS and MD it is MD, as there.  regs / aln / cigar: as mm2gb_align_out_t holds them
 *      (aln[i].cigar_off counted in cigar[]); read_of_reg[i]: the read of record i.  Sequences as text; residues compare as seq_nt4_table
 *      codes (N against N is a match); a reverse-strand record reads its query reverse-complemented.  A record with cigar_off < 0 gets
 *      no bytes.  *text_off (n_regs + 1) and *text are malloc'd, free with mm2gb_free.
 *      Refused, with the error text set and nothing run: a bit outside MM2GB_TEXT_*; a CIGAR operation other than M, I, D (the alignment
 *      call refuses splice and EQX); a word of length 0; a record whose words do not sum to qe - qs and re - rs; a record outside its sequences.
 *      The host form is the definition; the device form (csrc/aln_text_kernels.hip) equals it byte for byte. ---- */
#define MM2GB_TEXT_CG       0x1
#define MM2GB_TEXT_CS       0x2
#define MM2GB_TEXT_CS_LONG  0x4
#define MM2GB_TEXT_MD       0x8
int  mm2gb_aln_text_host(int what, int32_t n_ref, const char *const *ref_seqs, const int32_t *ref_lens, int64_t n_reads, const char *const *read_seqs, const int32_t *read_lens,
                         int64_t n_regs, const mm2gb_reg_t *regs, const int32_t *read_of_reg, const mm2gb_aln_t *aln, const uint32_t *cigar, int n_threads,
                         int64_t **text_off, char **text);
int  mm2gb_aln_text_gpu(mm2gb_engine_t *eng, int what, int32_t n_ref, const char *const *ref_seqs, const int32_t *ref_lens, int64_t n_reads, const char *const *read_seqs,
                        const int32_t *read_lens, int64_t n_regs, const mm2gb_reg_t *regs, const int32_t *read_of_reg, const mm2gb_aln_t *aln, const uint32_t *cigar,
                        int64_t **text_off, char **text);
/* the device form's seams, for tests: consts2 [0] columns (words, for cg:Z) per slice, [1] threads of a workgroup; s4 (optional): the last
 * call's seconds: [0] residues to the device (0 where they were resident), [1] the host's pass over the words (checks, word starts, slices),
 * [2] words and slices up, kernels, [3] the text back */
int  mm2gb_aln_text_gpu_info(mm2gb_engine_t *eng, int64_t *consts2, double *s4);
/* The same two calls for records of the spliced alignment calls: operation 3 (N) is accepted beside M, I and D.  cg:Z: the letter N.  cs:Z, short
 * and long: "~", the intron's first two target bases in lower case, its length, its last two (format.c:179-184); a run of matches is closed
 * before it as before any event.  MD:Z: the target moves on, nothing is printed and the run stays open (format.c:212-213).  Refused as
 * above, and an N word shorter than 2 (format.c:180 asserts it).  The device form takes an N word as ONE column. */
int  mm2gb_aln_text_splice_host(int what, int32_t n_ref, const char *const *ref_seqs, const int32_t *ref_lens, int64_t n_reads, const char *const *read_seqs,
                                const int32_t *read_lens, int64_t n_regs, const mm2gb_reg_t *regs, const int32_t *read_of_reg, const mm2gb_aln_t *aln, const uint32_t *cigar,
                                int n_threads, int64_t **text_off, char **text);
int  mm2gb_aln_text_splice_gpu(mm2gb_engine_t *eng, int what, int32_t n_ref, const char *const *ref_seqs, const int32_t *ref_lens, int64_t n_reads, const char *const *read_seqs,
                               const int32_t *read_lens, int64_t n_regs, const mm2gb_reg_t *regs, const int32_t *read_of_reg, const mm2gb_aln_t *aln, const uint32_t *cigar,
                               int64_t **text_off, char **text);

/* ---- = / X CIGARs (minimap2 --eqx), batched: mm_update_cigar_eqx (align.c:169-238) as a call of its own on the records the
 *      alignment calls return.  Every M word becomes runs of = (operation 7) and X (operation 8): residues compare as seq_nt4_table codes (N
 *      against N is =), a reverse-strand record reads its query reverse-complemented, a run never crosses a word; I, D and N words are copied.
 *      Arguments as mm2gb_aln_text_*.  *aln_out (n_regs records; malloc'd, free with mm2gb_free) is aln with cigar_off / n_cigar of the new
 *      words, which lie in *cigar_out (malloc'd, free with mm2gb_free); a record with cigar_off < 0 stays as it is.  The input is untouched.
 *      Refused, with the error text set and nothing run: what mm2gb_aln_text_splice_* refuse (an operation other than M, I, D, N; a word of
 *      length 0; words that do not sum to the record's spans; a record outside its sequences), and a = or X word: the rewrite has been done.
 *      The host form is the definition; the device form (csrc/eqx_kernels.hip) equals it word for word.  mm2gb_cigar_eqx_gpu_info: as
 *      mm2gb_aln_text_gpu_info (columns per slice, threads of a workgroup; the last call's seconds). ---- */
int  mm2gb_cigar_eqx_host(int32_t n_ref, const char *const *ref_seqs, const int32_t *ref_lens, int64_t n_reads, const char *const *read_seqs, const int32_t *read_lens,
                          int64_t n_regs, const mm2gb_reg_t *regs, const int32_t *read_of_reg, const mm2gb_aln_t *aln, const uint32_t *cigar, int n_threads,
                          mm2gb_aln_t **aln_out, uint32_t **cigar_out);
int  mm2gb_cigar_eqx_gpu(mm2gb_engine_t *eng, int32_t n_ref, const char *const *ref_seqs, const int32_t *ref_lens, int64_t n_reads, const char *const *read_seqs,
                         const int32_t *read_lens, int64_t n_regs, const mm2gb_reg_t *regs, const int32_t *read_of_reg, const mm2gb_aln_t *aln, const uint32_t *cigar,
                         mm2gb_aln_t **aln_out, uint32_t **cigar_out);
int  mm2gb_cigar_eqx_gpu_info(mm2gb_engine_t *eng, int64_t *consts2, double *s4);

/* ---- the mapper with base-level alignment (minimap2 -c, --cs, --MD; csrc/mapper.cpp): mm2gb_map_reads / mm2gb_map_reads_stream with a
 *      mm2gb_map_aln_t.  After mm_filter_strand_retained the batch's surviving records go through mm2gb_align_regs_* in one call (map.c:342-352;
 *      k and the HPC flag are the index's; what that call refuses fails the mapping call with the same text; with opt.q == opt.q2 &&
 *      opt.e == opt.e2 -- minimap2 -O4 -E2 -- the call is mm2gb_align_regs_extz_*, the single-affine DP), then per read mm_set_parent,
 *      mm_select_sub and mm_set_mapq in their forms with an alignment, and every PAF line is format.c:274-329's: columns 10 and 11 from the
 *      alignment, NM ms AS nn tp cm s1 s2 de zd rl, then the text mm2gb_aln_text_* gives for `what` (one call for the batch's lines).
 *      s_extra (optional): seconds for the alignment call, the steps after it and the text; stats->s_post holds the rest of the host's share. ---- */
typedef struct {
	const char *const *ref_seqs;      /* the reference sequences as text, n_ref of them */
	mm2gb_align_opt_t  opt;
	int32_t what;                     /* MM2GB_TEXT_*; 0: the tags without cg / cs / MD (minimap2 has no such form; allowed here) */
	int32_t align_on_device;          /* 1: the device form of the alignment call, and so is 0, the value a zeroed structure has (the default); -1: host threads */
	int32_t text_on_device;           /* 1: the device form of the text call; -1: host threads; 0 (default): host threads, by profiles/aln_text_rate.json */
} mm2gb_map_aln_t;
int  mm2gb_map_reads_aln(mm2gb_engine_t *eng, const mm2gb_index_t *ix, int k, const char *const *ref_names, const int32_t *ref_lens, int32_t n_ref,
                         const mm2gb_map_opt_t *opt, const mm2gb_map_aln_t *aln, int32_t n_reads, const char *const *names, const char *const *seqs, const int32_t *lens,
                         char **paf_out, int64_t *paf_len, mm2gb_map_stats_t *stats, double *s_extra /* 3, optional */);
int  mm2gb_map_reads_stream_aln(mm2gb_engine_t *const *engines, int n_engines, const mm2gb_index_t *ix, int k, const char *const *ref_names, const int32_t *ref_lens,
                                int32_t n_ref, const mm2gb_map_opt_t *opt, const mm2gb_map_aln_t *aln, int32_t n_reads, const char *const *names, const char *const *seqs,
                                const int32_t *lens, int64_t chunk_bases, char **paf_out, int64_t *paf_len, mm2gb_map_stats_t *stats, double *s_extra /* 3, optional; summed over chunks */);

/* ---- the mapper for spliced reads (minimap2 -x splice -c, --cs, --MD): the two calls above with a mm2gb_map_splice_t.  The stages are the
 *      same but for: is_cdna = 1 in the chaining DP (map.c:419, 695; max_dist_x = max_gap_ref as always), no re-chaining stage (map.c:698),
 *      the spliced alignment and text calls, and "ts:A:+" / "ts:A:-" after nn:i for trans_strand 1 / 2 (nothing for 0 and 3; format.c:281-282).
 *      mm2gb_map_opt_init_splice: mm2gb_map_opt_init, then the preset's bw = bw_long = max_gap_ref = 200000 and max_gap = 2000.  The index is
 *      built with k = 15, w = 5.  The calls always align; junction annotation is not taken.  Equal to
 *      minimap2 -x splice --cap-sw-mem=100000000 --max-chain-skip=2147483647 (the max_sw_mat departure of mm2gb_align_splice_opt_init). ---- */
typedef struct {
	const char *const *ref_seqs;      /* the reference sequences as text, in the index's order */
	mm2gb_align_splice_opt_t opt;
	int32_t what;                     /* MM2GB_TEXT_* */
	int32_t align_on_device;          /* as in mm2gb_map_aln_t */
	int32_t text_on_device;
} mm2gb_map_splice_t;
void mm2gb_map_opt_init_splice(mm2gb_map_opt_t *opt);
int  mm2gb_map_reads_splice(mm2gb_engine_t *eng, const mm2gb_index_t *ix, int k, const char *const *ref_names, const int32_t *ref_lens, int32_t n_ref,
                            const mm2gb_map_opt_t *opt, const mm2gb_map_splice_t *spl, int32_t n_reads, const char *const *names, const char *const *seqs, const int32_t *lens,
                            char **paf_out, int64_t *paf_len, mm2gb_map_stats_t *stats, double *s_extra /* 3, optional */);
int  mm2gb_map_reads_stream_splice(mm2gb_engine_t *const *engines, int n_engines, const mm2gb_index_t *ix, int k, const char *const *ref_names, const int32_t *ref_lens,
                                   int32_t n_ref, const mm2gb_map_opt_t *opt, const mm2gb_map_splice_t *spl, int32_t n_reads, const char *const *names, const char *const *seqs,
                                   const int32_t *lens, int64_t chunk_bases, char **paf_out, int64_t *paf_len, mm2gb_map_stats_t *stats, double *s_extra /* 3, optional; summed over chunks */);

/* ---- alignment of hits under MM_F_SR, batched: mm_align_skeleton with mm_align1's is_sr branches.  A third set of calls on the records of
 *      mm2gb_align_regs_*, which keep refusing MM_F_SR.  Per chain: mm_max_stretch (align.c:498-524) picks the best run of anchors on one diagonal, no end filter and
 *      no bad-seed filters, qs0 = 0 and qe0 = qlen, rs0 / re0 from align.c:625-630, the two extensions ordinary ksw_extd2 jobs with end_bonus, and ONE gap fill over the
 *      whole stretch whose first pass is not a DP (align.c:744-751): one M word of qe - qs columns, score = sum of a / -b per column and + e2 where either base is
 *      ambiguous (as the reference writes it; not sc_ambi).  mm_test_zdrop walks that word with the real matrix and makes no inversion trial; a fill that drops by more
 *      than zdrop runs again as a ksw_extd2 job (band bw_long * 1.5 + 1, exact maximum), may split the chain, and the tail is planned in the same form next round.
 *      mm_update_extra leaves out its log-gap term (a gap costs q + e), mm_update_dp_max is not run.  mm2gb_align_sr_opt_init: options.c:133-150.
 *      Refused by name, nothing run and *out zeroed: a flag word without MM_F_SR, MM_F_SPLICE, MM_F_QSTRAND, MM_F_EQX, an index with MM2GB_I_HPC (align.c:583),
 *      q == q2 && e == e2, a stretch whose two sides differ in length (anchors that are not the chainer's), and what mm2gb_align_regs_* refuse about max_sw_mat, records,
 *      anchors and segments.  sr_counts (may be NULL): see MM2GB_SR_N_*.  In *out, fill_one_pass counts the fills left ungapped and fill_two_pass those run again.
 *      The host form is the definition; the device form equals it: k_al_ungapped (csrc/align_kernels.hip) takes a wave per first-pass fill over the gathered bytes --
 *      score by reduction, mm_test_zdrop's walk as a scan -- and no DP launch is made for them. ---- */
enum { MM2GB_SR_N_FILL_UNGAPPED,     /* fills whose ungapped first pass stood */
       MM2GB_SR_N_FILL_RERUN,        /* fills that dropped and ran again as a DP */
       MM2GB_SR_N_STRETCH_SHORT,     /* chains whose best stretch holds fewer anchors than the chain */
       MM2GB_SR_N_COUNTS };
void mm2gb_align_sr_opt_init(mm2gb_align_opt_t *opt);
int  mm2gb_align_regs_sr_host(const mm2gb_align_opt_t *opt, int k, int idx_flag, int32_t n_ref, const char *const *ref_seqs, const int32_t *ref_lens,
                              int64_t n_reads, const char *const *read_seqs, const int32_t *read_lens, const int64_t *reg_off, const mm2gb_reg_t *regs,
                              const int64_t *anchor_off, const mm2gb_anchor_t *anchors, int n_threads, mm2gb_align_out_t *out, int64_t *sr_counts);
int  mm2gb_align_regs_sr_gpu(mm2gb_engine_t *eng, const mm2gb_align_opt_t *opt, int k, int idx_flag, int32_t n_ref, const char *const *ref_seqs, const int32_t *ref_lens,
                             int64_t n_reads, const char *const *read_seqs, const int32_t *read_lens, const int64_t *reg_off, const mm2gb_reg_t *regs,
                             const int64_t *anchor_off, const mm2gb_anchor_t *anchors, mm2gb_align_out_t *out, int64_t *sr_counts);

/* mm2gb_map_reads_sr / mm2gb_map_reads_stream_sr: minimap2 -x sr [-c | -c --cs | --cs=long --MD -c] on single-end reads, to the PAF (the arguments of mm2gb_map_reads /
 * mm2gb_map_reads_stream and a mm2gb_map_sr_t): anchors in heap order (under MM_F_HEAP_SORT), the chaining DP with the gaps of map.c:678-686 -- max_dist_y = max(qlen,
 * max_gap), max_dist_x = max(max_frag_len - qlen, max_gap) or max_gap_ref where set: one chaining call per distinct max_dist_x among a batch's reads (reads of one length
 * share it, and so do all reads of max_frag_len - max_gap bases or more) --, the rescue of map.c:708-731 (max_occ > mid_occ: reads with rep_len > 0 and no chain are
 * seeded, collected and chained again with max_occ in mid_occ's place, as one more batch; that round's rep_len stands in the line), no re-chaining stage, mm_gen_regs,
 * mm_set_parent, mm_select_sub, no mm_est_err (without an alignment no dv:f), then with align != 0 mm2gb_align_regs_sr_* and the steps after it in their forms with an
 * alignment, mm_set_mapq with is_sr = 1, the text calls for `what`, and under MM_F_NO_PRINT_2ND no line for a secondary hit.
 * seeding_on_device: 0 seeds on host threads; 1 on the device, the matches left resident for the heap-order collection (mm2gb_collect_seeds_heap_gpu's kernels read them
 * where they lie) and copied back once for the rescue's test and the lines' rl:i; 2 is treated as 1: the resident path skips nothing that the rescue needs.
 * sr_out (optional): the call's own counts and the seconds of the alignment call, the steps after it and the text; stats->s_chain holds stages 2 and 3 together, and
 * n_rechained / n_rmq_tied stay 0 (there is no re-chaining stage and no RMQ here).  The stream form sums them over chunks.
 * Refused by name: an HPC index (align.c:583), MM_F_RMQ (options.c:173), MM_F_QSTRAND, MM_F_EQX, MM_F_SPLICE, the read-overlap bits, options without MM_F_SR, align != 0
 * without ref_seqs, what != 0 with align == 0; mates of a pair come through mm2gb_map_frags_sr (below).  mm2gb_map_sr_init: max_occ = 5000, max_frag_len = 800, align = 0 and
 * mm2gb_align_sr_opt_init's values in opt. */
typedef struct {
	const char *const *ref_seqs;      /* the reference sequences as text, in the index's order (not read while align is 0; may then be NULL) */
	mm2gb_align_opt_t opt;            /* the alignment's option set (not read while align is 0) */
	int32_t align;                    /* 0: no base-level alignment, PAF from the chains; 1: minimap2 -c */
	int32_t what;                     /* MM2GB_TEXT_*; 0 while align is 0 */
	int32_t align_on_device, text_on_device;      /* as in mm2gb_map_aln_t */
	int32_t max_occ, max_frag_len;    /* mm_mapopt_t::max_occ, max_frag_len: the two fields mm2gb_map_opt_t has no room for */
} mm2gb_map_sr_t;
typedef struct {
	int64_t n_chain_calls;            /* chaining calls made (one per distinct max_dist_x -- with fragments: per distinct (n_seg, max_dist_x, max_dist_y) --, both rounds) */
	int64_t n_rescued;                /* reads (fragments) that went through the max_occ round */
	int64_t n_tied_reads;             /* reads whose anchors the host's heap ordered (two equal index entries) */
	int64_t sr_counts[MM2GB_SR_N_COUNTS];
	double  s_extra[3];               /* seconds: the alignment call, the steps after it, the text */
} mm2gb_map_sr_out_t;
void mm2gb_map_sr_init(mm2gb_map_sr_t *sr);
int  mm2gb_map_reads_sr(mm2gb_engine_t *eng, const mm2gb_index_t *ix, int k, const char *const *ref_names, const int32_t *ref_lens, int32_t n_ref, const mm2gb_map_opt_t *opt,
                        const mm2gb_map_sr_t *sr, int32_t n_reads, const char *const *names, const char *const *seqs, const int32_t *lens, char **paf_out, int64_t *paf_len,
                        mm2gb_map_stats_t *stats, mm2gb_map_sr_out_t *sr_out);
int  mm2gb_map_reads_stream_sr(mm2gb_engine_t *const *engines, int n_engines, const mm2gb_index_t *ix, int k, const char *const *ref_names, const int32_t *ref_lens,
                               int32_t n_ref, const mm2gb_map_opt_t *opt, const mm2gb_map_sr_t *sr, int32_t n_reads, const char *const *names, const char *const *seqs,
                               const int32_t *lens, int64_t chunk_bases, char **paf_out, int64_t *paf_len, mm2gb_map_stats_t *stats, mm2gb_map_sr_out_t *sr_out);

/* ---- SAM output and = / X CIGARs from the mapper (minimap2 -a, --eqx, -Y, --sam-hit-only): the calls above that align, with a mm2gb_map_out_t as their
 *      last argument.  NULL, or a zeroed record: the bytes of the call without it.
 *      format 1: every line is mm_write_sam3's at n_seg = 1 (format.c:389-546): FLAG 0x10 on the reverse strand, 0x100 for a hit that is not its own
 *      parent, 0x800 for every primary hit of a read but its first (mm_set_sam_pri, hit.c:220-229); RNAME, POS + 1, MAPQ; the CIGAR with clips (H on 0x800
 *      lines, S elsewhere and everywhere under MM2GB_F_SOFTCLIP; swapped on the reverse strand); "*\t0\t0"; SEQ: the whole read on the first line and
 *      under MM2GB_F_SOFTCLIP, qs .. qe on 0x800 lines, "*" on 0x100 lines, reverse-complemented on the reverse strand with IUPAC codes and case kept;
 *      QUAL "*"; the PAF line's tags; SA:Z on a primary line of a read with other aligned primaries; cs:Z / MD:Z as `what` asks (MM2GB_TEXT_CG means
 *      nothing here); rl:i.  A read without a hit gets "name 4 * 0 0 * * 0 0 SEQ * rl:i" unless MM2GB_F_SAM_HIT_ONLY; stats->n_mapped counts reads with a
 *      hit, not lines.  mm2gb_sam_header gives the @SQ lines and a @PG line of this project (malloc'd, free with mm2gb_free); paf_out holds no header.
 *      MM2GB_F_EQX in flag, either format: the CIGAR column / cg:Z show mm2gb_cigar_eqx_*'s words, made in one call per batch after the text call, which
 *      reads the M words (format.c prints the same cs:Z / MD:Z for either).  eqx_on_device: 1 the device form -- on the residues the alignment call left
 *      on the device where they are this batch's, uploaded otherwise --, -1 host threads, 0 the default: host threads (profiles/eqx_rate.json).
 *      Refused by name: a format other than 0 / 1, a flag bit other than the three, SAM or MM2GB_F_EQX on a call that does not align
 *      (mm2gb_map_reads_sr_out with align = 0: -a implies -c); the read-overlap bits are refused with any alignment as before.  Every refusal of the
 *      calls above stays, MM_F_EQX in the mapping options' and the alignment options' flag included: the bit belongs to mm2gb_map_out_t alone.
 *      Not taken: -L (the CIGAR in CG:B:I), qualities (reads are as from FASTA), -R, -y, --paf-no-hit, --secondary-seq, SAM for paired ends (the pair fields of
 *      mm_write_sam3's n_seg > 1 branches). ---- */
#define MM2GB_F_SOFTCLIP     0x80000LL
#define MM2GB_F_SAM_HIT_ONLY 0x40000000LL
typedef struct {
	int32_t format;                   /* 0 PAF, 1 SAM */
	int32_t eqx_on_device;            /* 1 the device form of the = / X rewrite; -1 host threads; 0 (default): host threads */
	int64_t flag;                     /* MM2GB_F_EQX, MM2GB_F_SOFTCLIP, MM2GB_F_SAM_HIT_ONLY: the reference's values */
} mm2gb_map_out_t;
void mm2gb_map_out_init(mm2gb_map_out_t *out);
int  mm2gb_sam_header(int32_t n_ref, const char *const *ref_names, const int32_t *ref_lens, char **out, int64_t *len);
int  mm2gb_map_reads_aln_out(mm2gb_engine_t *eng, const mm2gb_index_t *ix, int k, const char *const *ref_names, const int32_t *ref_lens, int32_t n_ref,
                             const mm2gb_map_opt_t *opt, const mm2gb_map_aln_t *aln, int32_t n_reads, const char *const *names, const char *const *seqs, const int32_t *lens,
                             char **paf_out, int64_t *paf_len, mm2gb_map_stats_t *stats, double *s_extra, const mm2gb_map_out_t *out);
int  mm2gb_map_reads_stream_aln_out(mm2gb_engine_t *const *engines, int n_engines, const mm2gb_index_t *ix, int k, const char *const *ref_names, const int32_t *ref_lens,
                                    int32_t n_ref, const mm2gb_map_opt_t *opt, const mm2gb_map_aln_t *aln, int32_t n_reads, const char *const *names, const char *const *seqs,
                                    const int32_t *lens, int64_t chunk_bases, char **paf_out, int64_t *paf_len, mm2gb_map_stats_t *stats, double *s_extra, const mm2gb_map_out_t *out);
int  mm2gb_map_reads_splice_out(mm2gb_engine_t *eng, const mm2gb_index_t *ix, int k, const char *const *ref_names, const int32_t *ref_lens, int32_t n_ref,
                                const mm2gb_map_opt_t *opt, const mm2gb_map_splice_t *spl, int32_t n_reads, const char *const *names, const char *const *seqs, const int32_t *lens,
                                char **paf_out, int64_t *paf_len, mm2gb_map_stats_t *stats, double *s_extra, const mm2gb_map_out_t *out);
int  mm2gb_map_reads_stream_splice_out(mm2gb_engine_t *const *engines, int n_engines, const mm2gb_index_t *ix, int k, const char *const *ref_names, const int32_t *ref_lens,
                                       int32_t n_ref, const mm2gb_map_opt_t *opt, const mm2gb_map_splice_t *spl, int32_t n_reads, const char *const *names, const char *const *seqs,
                                       const int32_t *lens, int64_t chunk_bases, char **paf_out, int64_t *paf_len, mm2gb_map_stats_t *stats, double *s_extra, const mm2gb_map_out_t *out);
int  mm2gb_map_reads_sr_out(mm2gb_engine_t *eng, const mm2gb_index_t *ix, int k, const char *const *ref_names, const int32_t *ref_lens, int32_t n_ref, const mm2gb_map_opt_t *opt,
                            const mm2gb_map_sr_t *sr, int32_t n_reads, const char *const *names, const char *const *seqs, const int32_t *lens, char **paf_out, int64_t *paf_len,
                            mm2gb_map_stats_t *stats, mm2gb_map_sr_out_t *sr_out, const mm2gb_map_out_t *out);
int  mm2gb_map_reads_stream_sr_out(mm2gb_engine_t *const *engines, int n_engines, const mm2gb_index_t *ix, int k, const char *const *ref_names, const int32_t *ref_lens,
                                   int32_t n_ref, const mm2gb_map_opt_t *opt, const mm2gb_map_sr_t *sr, int32_t n_reads, const char *const *names, const char *const *seqs,
                                   const int32_t *lens, int64_t chunk_bases, char **paf_out, int64_t *paf_len, mm2gb_map_stats_t *stats, mm2gb_map_sr_out_t *sr_out,
                                   const mm2gb_map_out_t *out);

/* ---- paired-end short reads (minimap2 -x sr r1.fq r2.fq, without -c), to the PAF: fragments of two mates seeded and chained as one query.
 *      mm2gb_frag_offsets: fragments as map.c:1297-1304 forms them under MM_F_FRAG_MODE -- a run of consecutive reads with the same name, a trailing "/" + one digit
 *      not being part of the name (mm_qname_same, bseq.h:31-44).  frag_off: room for n_reads + 1 entries; *n_frag fragments, frag_off[*n_frag] = n_reads.  Two input
 *      files are the same thing interleaved.
 *      mm2gb_map_frags_sr / mm2gb_map_frags_stream_sr: the arguments of mm2gb_map_reads_sr / _stream_sr plus the fragments, pe_ori (mm_mapopt_t::pe_ori, 0..3; -x sr: 1) and
 *      an optional mm2gb_map_out_t.  A fragment of one read goes the single-end way, with the bytes of mm2gb_map_reads_sr.  For a fragment of two: mate j is
 *      reverse-complemented before mapping when (j == 0 && pe_ori >> 1 & 1) || (j == 1 && pe_ori & 1) and its hits' qs / qe / strand are flipped back afterwards
 *      (map.c:1169-1199); the mates are seeded as one list (mm2gb_collect_matches_frag, or its device form with seeding_on_device = 1, the matches left resident for
 *      the heap-order collection), anchors collected with qlen = qlen_sum, one chaining DP at n_seg = 2 with max_dist_x = max(max_frag_len - qlen_sum, max_gap) (or
 *      max_gap_ref) and max_dist_y = max(qlen_sum, max_gap) -- at n_seg > 1 max_dist_y also bounds the reference gap between anchors of different mates, so a chaining
 *      call is made per distinct (n_seg, max_dist_x, max_dist_y) of the batch: n_chain_calls --; the rescue of map.c:708-731 for a fragment with rep_len > 0 that has no
 *      chain or whose best-scoring chain lacks a mate; mm_gen_regs with qlen_sum and the hash of the FIRST mate's name, mm_set_parent, mm_select_sub_multi (pe.c:6-43),
 *      mm_seg_gen (hit.c:331-385) into per-mate hits, per mate mm_set_parent and mm_set_mapq with the fragment's rep_len, and the PAF lines of mate 0, then mate 1,
 *      each under its own name and length.  The stream form cuts chunks only between fragments.  stats->n_mapped counts fragments with a line.
 *      Refused by name: sr->align != 0 with a two-mate fragment in the batch ("paired ends with base-level alignment": -c, mm_pair and mm_set_pe_thru are not built), a
 *      mm2gb_map_out_t with SAM or MM_F_EQX, a fragment of more than two reads (MM_MAX_SEG > 2), pe_ori outside 0..3, and everything mm2gb_map_reads_sr refuses.
 *      Not built: MM_F_INDEPEND_SEG.
 *      mm2gb_select_sub_multi_host / mm2gb_seg_gen_host: the two steps by themselves, batched over fragments on the host (there is no device form: at that stage the
 *      records and kept anchors lie on the host).  qlens: two entries per fragment (the second ignored where n_segs[f] is 1).
 *      select_sub_multi: fragment f's records regs[reg_off[f] .. reg_off[f + 1]) (after mm_set_parent) are squeezed in place to their first n_kept[f], ids and parents
 *      re-synchronised (mm_sync_regs).  seg_gen: unit 2 f + s of *out is fragment f's segment s: its records (seg_split and seg_id set in flags: bits 15, 16-23) and its
 *      anchors with y in the mate's own coordinates; records' `as` count from the unit's first anchor.  Free with mm2gb_seg_out_free. ---- */
int  mm2gb_frag_offsets(int32_t n_reads, const char *const *names, int32_t *frag_off, int32_t *n_frag);
int  mm2gb_map_frags_sr(mm2gb_engine_t *eng, const mm2gb_index_t *ix, int k, const char *const *ref_names, const int32_t *ref_lens, int32_t n_ref, const mm2gb_map_opt_t *opt,
                        const mm2gb_map_sr_t *sr, int32_t n_reads, const char *const *names, const char *const *seqs, const int32_t *lens, char **paf_out, int64_t *paf_len,
                        mm2gb_map_stats_t *stats, mm2gb_map_sr_out_t *sr_out, int32_t n_frag, const int32_t *frag_off, int32_t pe_ori, const mm2gb_map_out_t *out);
int  mm2gb_map_frags_stream_sr(mm2gb_engine_t *const *engines, int n_engines, const mm2gb_index_t *ix, int k, const char *const *ref_names, const int32_t *ref_lens,
                               int32_t n_ref, const mm2gb_map_opt_t *opt, const mm2gb_map_sr_t *sr, int32_t n_reads, const char *const *names, const char *const *seqs,
                               const int32_t *lens, int64_t chunk_bases, char **paf_out, int64_t *paf_len, mm2gb_map_stats_t *stats, mm2gb_map_sr_out_t *sr_out,
                               int32_t n_frag, const int32_t *frag_off, int32_t pe_ori, const mm2gb_map_out_t *out);
typedef struct {
	int64_t *reg_off;                 /* 2 * n_frag + 1 */
	mm2gb_reg_t *regs;
	int64_t *anchor_off;              /* 2 * n_frag + 1 */
	mm2gb_anchor_t *anchors;
} mm2gb_seg_out_t;
int  mm2gb_select_sub_multi_host(float pri_ratio, float pri1, float pri2, int32_t min_diff, int32_t best_n, int64_t n_frag, const int32_t *n_segs, const int32_t *qlens,
                                 const int32_t *max_gap_ref, const int64_t *reg_off, mm2gb_reg_t *regs, int32_t *n_kept);
int  mm2gb_seg_gen_host(int64_t n_frag, const int32_t *n_segs, const int32_t *qlens, const uint32_t *hash, const int64_t *reg_off, const mm2gb_reg_t *regs,
                        const int64_t *anchor_off, const mm2gb_anchor_t *anchors, mm2gb_seg_out_t *out);
void mm2gb_seg_out_free(mm2gb_seg_out_t *out);

#ifdef __cplusplus
}
#endif
#endif
