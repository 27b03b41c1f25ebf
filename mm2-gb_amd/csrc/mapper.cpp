// mapper.cpp -- reads in, PAF out, without the reference's sources: the host side around the device path, written
// from scratch to give the reference's output for single-segment reads mapped without base-level alignment (no -a / -c).
//
//   per batch of reads (map_reads_body: one function per step):   1 matches (seeding.cpp on host threads, or seed_kernels.hip)  ->  2 anchors, sorted (collect_seed_hits: device for large batches, host threads otherwise)  ->  3 chains (device:
//   chaining DP + backtrack)  ->  4 re-chaining of reads whose chains look broken (host threads: mg_lchain_rmq with the reference's tree, csrc/rmq_host.cpp, map.c:697-708)
//   ->  5 hit records (device: mm_gen_regs)  ->  6 per read on the host: primary / secondary (mm_set_parent, hit.c:125-198), which
//   secondaries stay (mm_select_sub, hit.c:272-295, mm_sync_regs hit.c:247-270), divergence estimate (mm_est_err, esterr.c:31-64),
//   mm_filter_strand_retained (hit.c:297-309), mapping quality (mm_set_mapq, hit.c:420-466), PAF line (format.c:274-321).
//
//   With a mm2gb_map_aln_t (mm2gb_map_reads_aln; minimap2 -c): 6a after mm_filter_strand_retained the batch's surviving records go through
//   mm2gb_align_regs_* in one call (map.c:342-352), 6b then per read mm_set_parent, mm_select_sub and mm_set_mapq in their forms with an
//   alignment, 6c and the PAF line gets NM/ms/AS/nn/de and cg:Z / cs:Z / MD:Z (the text of the whole batch from one mm2gb_aln_text_* call).
//
//   With a mm2gb_map_splice_t (mm2gb_map_reads_splice; minimap2 -x splice -c): the same stages with is_cdna = 1 in the chaining DP
//   (map.c:419, 695), no re-chaining stage (map.c:698 leaves MM_F_SPLICE out), the spliced alignment and text calls in 6a / 6c, and ts:A in the line.
//
//   With MM_F_RMQ in the options' flag (the asm5 / asm10 / asm20 presets, mm2gb_map_opt_init_preset; minimap2 --rmq=yes): stage 3 is not the chaining
//   DP -- every read's sorted anchors go through mg_lchain_rmq's fill with bw (map.c:690-692), the same call as stage 4's with bw_long (device and host
//   threads as rechain_on_device says, ties redone by the host form).  Stage 4 follows as always.  The spliced calls refuse the flag (options.c:173).
//
//   Read against read (mm2gb_map_opt_init_ava, or the four bits of minimap2 -X on any option set; the calls without base-level alignment only): with
//   MM_F_NO_DIAG / MM_F_NO_DUAL step 2's name tests run (map.c:208-219) on the names' ranks in strcmp order over reads and references together (name_ranks, once
//   per call); MM_F_NO_LJOIN leaves stage 4 out (map.c:698); MM_F_ALL_CHAINS leaves mm_set_parent / mm_select_sub out of stage 6 (map.c:335), so every
//   record keeps parent = MM_PARENT_UNSET: mapping quality 0 (hit.c:436, 463), tp:A:S and no s2 (format.c:301-304).
//
//   The resident path (seeding_on_device = 2, no re-chaining stage, no MM_F_RMQ, no alignment; chain_resident, hit_records_resident): steps 2, 3 and 5 run on
//   device pointers and mm_est_err's walk runs there too (est_err_kernels.hip), so no anchor crosses the link in either direction: what comes down is the
//   offsets, the hit records, the walk's counts, sum_k and rep_len.
//   Short single-end reads (mm2gb_map_reads_sr / _stream_sr with the options of mm2gb_map_opt_init_sr; minimap2 -x sr [-c]): stage 2 in the heap's order
//   (collect_seed_hits_heap, map.c:229-293: seed_heap_host.cpp / seed_heap_kernels.hip; seeded on the device, from the matches resident there), stage 3 as one chaining
//   call per distinct max_dist_x of the batch (the gaps depend on the read's length, map.c:678-686), the max_occ rescue of map.c:708-731 as one more batch, no stage 4,
//   and in stage 6 no mm_est_err, the alignment call in its MM_F_SR form (mm2gb_align_regs_sr_*: ungapped fills), mm_set_mapq with is_sr = 1, no line
//   for a secondary hit under MM_F_NO_PRINT_2ND (anchors_and_chains_sr, finish_reads_sr).
//   With a mm2gb_map_out_t (the calls named _out, on the three families that align; minimap2 -a, --eqx, -Y, --sam-hit-only): after 6c the kept records' M words go
//   through mm2gb_cigar_eqx_* in one call under MM_F_EQX (eqx_words; mm_update_cigar_eqx is the last statement of mm_update_extra and nothing after it tells M from = / X,
//   DESIGN 6g), and a line is mm_write_sam3's at n_seg = 1 (write_sam, format.c:389-546) with mm_set_sam_pri's choice of the primary line, or the PAF line with cg:Z from
//   the new words.  cs:Z / MD:Z are always asked of the text calls with the M words (format.c treats 0, 7 and 8 alike).  Left out of SAM: -L (CG:B:I), qualities (QUAL is
//   *), -R read groups, -y comments, --secondary-seq; of PAF: --paf-no-hit.
//   Paired-end short reads (mm2gb_map_frags_sr / _stream_sr; minimap2 -x sr r1.fq r2.fq without -c): the batch's units are FRAGMENTS of one or two mates (MapCall::frag,
//   frag_units).  Stage 1 seeds a fragment's mates as one list of qlen_sum bases (collect_matches_frag_refs, or seed_kernels.hip's k_f_view before the match kernels), stage 2 is
//   the single-end one at qlen = qlen_sum, stage 3 one chaining call per distinct (n_seg, max_dist_x, max_dist_y) with n_seg = 2 for two mates (chain_groups_sr), the rescue
//   also where the best chain lacks a mate, stage 5 as ever with the first mate's name in the hash, and stage 6 (finish_frags_sr) mm_set_parent, mm_select_sub_multi (pe.c:6-43),
//   mm_seg_gen (hit.c:331-385) into per-mate hits, per mate mm_set_parent and mm_set_mapq, the pe_ori flip (map.c:1188-1199) and mate 0's lines, then mate 1's.
// Not reproduced: base-level alignment of mate pairs (-c with mm_pair, mm_set_pe_thru), SAM for pairs (none of mm_write_sam3's n_seg > 1 branches), more than two query segments,
// MM_F_INDEPEND_SEG, spliced mapping without base-level alignment, read overlap with base-level alignment, junction annotation, ALT contigs, --qstrand, multi-part indexes.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>
#include "engine.h"
#include "host_threads.h"
#include "host_chain.h"
#include "align_host.h"
#include "aln_text_host.h"
#include "eqx.h"
#include "est_err.h"
#include "trace.h"

namespace mm2gb {
namespace {

struct Hit {                                   // mm_reg1_t without the alignment (minimap.h:104-119)
	int id, cnt, rid, score, qs, qe, rs, re, parent, subsc, as, mlen, blen, n_sub, score0;
	int mapq;
	bool rev, strand_retained;
	uint32_t hash;
	float div;
	// with an alignment (mm_extra_t, minimap.h:94-102; the record's split and inv bits): none of it is set or looked at without one
	bool has_p = false, inv = false, sam_pri = false;   // sam_pri: mm_set_sam_pri's (hit.c:220-229), the read's one line without 0x100 / 0x800
	int split = 0, dp_score = 0, dp_max = 0, dp_max2 = 0, n_ambi = 0, trans_strand = 0, n_cigar = 0;
	uint32_t flags = 0;                        // mm_reg1_t's bit-field word as the record carries it between the calls
	int64_t aln = -1;                          // its place in the alignment call's result
	int src = -1;                              // the resident path: its place among the read's hit records as the device made them (where its walk's counts are)
};

enum { PARENT_UNSET = -1, PARENT_TMP_PRI = -2 };   // mmpriv.h:13-14

// khash.h:383-409
uint32_t name_hash(const char *s) { uint32_t h = (uint32_t)(unsigned char)*s; if (h) for (++s; *s; ++s) h = (h << 5) - h + (uint32_t)(unsigned char)*s; return h; }
uint32_t wang(uint32_t k) { k += ~(k << 15); k ^= k >> 10; k += k << 3; k ^= k >> 6; k += ~(k << 11); k ^= k >> 16; return k; }

// hit.c:125-198 without ALT: hits come best first; a hit is secondary to the first earlier primary it overlaps by
// more than mask_level of the shorter of the two (less what earlier primaries leave uncovered of it).  Where both carry an alignment
// the primary's dp_max2 follows, and a secondary within sub_diff of it counts as a sub-optimal hit (hit.c:171-176)
void set_parent(float mask_level, int mask_len, std::vector<Hit> &r, bool hard_mask_level, int sub_diff = 0)
{
	const int n = (int)r.size();
	if (n == 0) return;
	for (int i = 0; i < n; ++i) r[(size_t)i].id = i;
	std::vector<int> prim{ 0 };
	std::vector<uint64_t> cov;
	r[0].parent = 0;
	for (int i = 1; i < n; ++i) {
		Hit &ri = r[(size_t)i];
		const int si = ri.qs, ei = ri.qe;
		int uncov = 0;
		bool overlaps_any = true;
		if (!hard_mask_level) {
			cov.clear();
			for (int w : prim) {
				int sj = r[(size_t)w].qs, ej = r[(size_t)w].qe;
				if (ej <= si || sj >= ei) continue;
				cov.push_back((uint64_t)std::max(sj, si) << 32 | (uint32_t)std::min(ej, ei));
			}
			overlaps_any = !cov.empty();
			if (overlaps_any) {                          // length of [si, ei) no earlier primary covers
				std::sort(cov.begin(), cov.end());
				int x = si;
				for (uint64_t c : cov) {
					if ((int)(c >> 32) > x) uncov += (int)(c >> 32) - x;
					x = std::max(x, (int)(int32_t)c);
				}
				if (ei > x) uncov += ei - x;
			}
		}
		bool secondary = false;
		if (overlaps_any) {
			for (int w : prim) {
				Hit &rp = r[(size_t)w];
				const int sj = rp.qs, ej = rp.qe;
				if (ej <= si || sj >= ei) continue;
				const int lmin = std::min(ej - sj, ei - si), lmax = std::max(ej - sj, ei - si);
				const int ol = std::min(ei, ej) - std::max(si, sj);
				if ((float)ol / lmin - (float)uncov / lmax > mask_level && uncov <= mask_len) {
					ri.parent = rp.parent;
					rp.subsc = std::max(rp.subsc, ri.score);
					bool cnt_sub = ri.cnt >= rp.cnt;
					if (rp.has_p && ri.has_p && (rp.rid != ri.rid || rp.rs != ri.rs || rp.re != ri.re || ol != lmin)) {      // (the last condition: not the same hit after DP)
						rp.dp_max2 = std::max(rp.dp_max2, ri.dp_max);
						if (rp.dp_max - ri.dp_max <= sub_diff) cnt_sub = true;
					}
					if (cnt_sub) ++rp.n_sub;
					secondary = true;
					break;
				}
			}
		}
		if (!secondary) { prim.push_back(i); ri.parent = i; ri.n_sub = 0; }
	}
}

// hit.c:247-270 (+ mm_set_sam_pri, which has no effect on PAF)
void sync_hits(std::vector<Hit> &r)
{
	int max_id = -1;
	for (const Hit &h : r) max_id = std::max(max_id, h.id);
	std::vector<int> now((size_t)(max_id + 1), -1);
	for (size_t i = 0; i < r.size(); ++i) if (r[i].id >= 0) now[(size_t)r[i].id] = (int)i;
	for (size_t i = 0; i < r.size(); ++i) {
		Hit &h = r[i];
		h.id = (int)i;
		if (h.parent == PARENT_TMP_PRI) h.parent = (int)i;
		else if (h.parent >= 0 && now[(size_t)h.parent] >= 0) h.parent = now[(size_t)h.parent];
		else h.parent = PARENT_UNSET;
	}
}

// hit.c:272-295
void select_sub(float pri_ratio, int min_diff, int best_n, bool check_strand, int min_strand_sc, std::vector<Hit> &r)
{
	if (!(pri_ratio > 0.0f) || r.empty()) return;
	const size_t n = r.size();
	size_t k = 0;
	int n_2nd = 0;
	for (size_t i = 0; i < n; ++i) {
		const int p = r[i].parent;
		if (p == (int)i || r[i].inv) { r[k++] = r[i]; continue; }          // primary, or an inversion (only an alignment makes one)
		const Hit &rp = r[(size_t)p];                 // parents precede their secondaries and are never dropped: still at index p? see below
		if ((r[i].score >= rp.score * pri_ratio || r[i].score + min_diff >= rp.score) && n_2nd < best_n) {
			if (!(r[i].qs == rp.qs && r[i].qe == rp.qe && r[i].rid == rp.rid && r[i].rs == rp.rs && r[i].re == rp.re)) { r[k++] = r[i]; ++n_2nd; }
		} else if (check_strand && n_2nd < best_n && r[i].score > min_strand_sc && r[i].rev != rp.rev) {
			r[i].strand_retained = true;
			r[k++] = r[i]; ++n_2nd;
		}
	}
	if (k != n) { r.resize(k); sync_hits(r); }
}

void reg_from(const struct Hit &h, mm2gb_reg_t &g);

// esterr.c:30-64: the walk is est_err.cpp's (the definition of the device form); the pow of esterr.c:62 is finished here
void estimate_divergence(int qlen, const std::vector<int32_t> &ref_len, std::vector<Hit> &r, const mm2gb_anchor_t *a, int n_mini, const uint64_t *mini_pos)
{
	if (n_mini == 0 || r.empty()) return;
	std::vector<mm2gb_reg_t> g(r.size());
	std::vector<mm2gb_est_err_t> e(r.size());
	uint64_t sum_k = 0;
	for (size_t i = 0; i < r.size(); ++i) reg_from(r[i], g[i]);
	est_err_read(qlen, (int64_t)r.size(), g.data(), a, n_mini, mini_pos, ref_len.data(), e.data(), &sum_k);
	for (size_t i = 0; i < r.size(); ++i) r[i].div = mm2gb_est_err_div(e[i].n_match, e[i].n_tot, sum_k, n_mini);
}

// the same from the counts the device's walk left (the resident path): e, the counts of the read's records as the device made them
void divergence_from_counts(std::vector<Hit> &r, const mm2gb_est_err_t *e, uint64_t sum_k, int n_mini)
{
	if (n_mini == 0) return;
	for (Hit &h : r) h.div = mm2gb_est_err_div(e[h.src].n_match, e[h.src].n_tot, sum_k, n_mini);
}

// hit.c:297-309
void filter_strand_retained(std::vector<Hit> &r)
{
	size_t k = 0;
	for (size_t i = 0; i < r.size(); ++i) {
		const int p = r[i].parent;
		if (!r[i].strand_retained || r[i].div < r[(size_t)p].div * 5.0f || r[i].div < 0.01f) r[k++] = r[i];
	}
	r.resize(k);
}

// hit.c:420-466 (is_sr: hit.c:446-449 left out); match_sc: the alignment's match score, looked at only where a hit carries an alignment
void set_mapq(std::vector<Hit> &r, int min_chain_sc, int rep_len, int match_sc = 1, bool is_sr = false)
{
	if (r.empty()) return;
	int64_t sum_sc = 0;
	for (const Hit &h : r) if (h.parent == h.id) sum_sc += h.score;
	const float uniq_ratio = (float)sum_sc / (sum_sc + rep_len);
	bool any_inv = false;
	for (Hit &h : r) {
		if (h.inv) { h.mapq = 0; any_inv = true; continue; }
		if (h.parent != h.id) { h.mapq = 0; continue; }
		const float pen_s1 = (h.score > 100 ? 1.0f : 0.01f * h.score) * uniq_ratio;
		float pen_cm = h.cnt > 10 ? 1.0f : 0.1f * h.cnt;
		pen_cm = pen_s1 < pen_cm ? pen_s1 : pen_cm;
		const int subsc = h.subsc > min_chain_sc ? h.subsc : min_chain_sc;
		int mapq;
		if (h.has_p && h.dp_max2 > 0 && h.dp_max > 0) {
			const float identity = (float)h.mlen / h.blen;
			const float x = (float)h.dp_max2 * subsc / h.dp_max / h.score0;
			mapq = (int)(identity * pen_cm * 40.0f * (1.0f - x * x) * logf((float)h.dp_max / match_sc));
			if (!is_sr) {
				const int mapq_alt = (int)(6.02f * identity * identity * (h.dp_max - h.dp_max2) / match_sc + .499f);  // "BWA-MEM like", in case the long-read heuristic fails
				mapq = mapq < mapq_alt ? mapq : mapq_alt;
			}
		} else {
			const float x = (float)subsc / h.score0;
			if (h.has_p) {
				const float identity = (float)h.mlen / h.blen;
				mapq = (int)(identity * pen_cm * 40.0f * (1.0f - x) * logf((float)h.dp_max / match_sc));
			} else mapq = (int)(pen_cm * 40.0f * (1.0f - x) * logf((float)h.score));
		}
		mapq -= (int)(4.343f * logf((float)(h.n_sub + 1)) + .499f);
		mapq = mapq > 0 ? mapq : 0;
		h.mapq = mapq < 60 ? mapq : 60;
		if (h.has_p && h.dp_max > h.dp_max2 && h.mapq == 0) h.mapq = 1;
	}
	// mm_set_inv_mapq (hit.c:395-419): an inversion between two primaries on the reference takes the smaller of their qualities
	if (!any_inv || r.size() < 3) return;
	std::vector<mm2gb_anchor_t> aux;
	for (size_t i = 0; i < r.size(); ++i) if (r[i].parent == (int)i || r[i].parent < 0) aux.push_back({ (uint64_t)r[i].rid << 32 | (uint32_t)r[i].rs, (uint64_t)i });
	sort_by_x_like_host(aux.data(), aux.data() + aux.size());
	for (size_t i = 1; i + 1 < aux.size(); ++i) {
		Hit &h = r[(size_t)aux[i].y];
		if (h.inv) h.mapq = std::min(r[(size_t)aux[i - 1].y].mapq, r[(size_t)aux[i + 1].y].mapq);
	}
}

void append_int(std::string &s, long long v) { char buf[24]; snprintf(buf, sizeof buf, "%lld", v); s += buf; }

// write_tags (format.c:274-300), what a PAF and a SAM line share; words: the hit's CIGAR words where it carries an alignment (mm_event_identity, align.c:895-915, counts its gaps)
void write_tags(std::string &out, const Hit &h, const uint32_t *words)
{
	if (h.has_p) {
		out += "\tNM:i:"; append_int(out, h.blen - h.mlen + h.n_ambi); out += "\tms:i:"; append_int(out, h.dp_max); out += "\tAS:i:"; append_int(out, h.dp_score);
		out += "\tnn:i:"; append_int(out, h.n_ambi);
		if (h.trans_strand == 1 || h.trans_strand == 2) { out += "\tts:A:"; out += "?+-?"[h.trans_strand]; }
	}
	out += "\ttp:A:"; out += h.id == h.parent ? (h.inv ? 'I' : 'P') : (h.inv ? 'i' : 'S');
	out += "\tcm:i:"; append_int(out, h.cnt);
	out += "\ts1:i:"; append_int(out, h.score);
	if (h.parent == h.id) { out += "\ts2:i:"; append_int(out, h.subsc); }
	if (h.has_p) {
		int32_t n_gap = 0, n_gapo = 0;
		for (int32_t k = 0; k < h.n_cigar; ++k) if ((words[k] & 0xf) == 1 || (words[k] & 0xf) == 2) { ++n_gapo; n_gap += (int32_t)(words[k] >> 4); }
		const double ident = (double)h.mlen / (h.blen + h.n_ambi - n_gap + n_gapo), de = 1.0 - ident;
		out += "\tde:f:";
		if (de == 0.0) out += '0';
		else { char buf[16]; snprintf(buf, sizeof buf, "%.4f", de); out += buf; }
	} else if (h.div >= 0.0f && h.div <= 1.0f) {
		out += "\tdv:f:";
		if (h.div == 0.0f) out += '0';
		else { char buf[16]; snprintf(buf, sizeof buf, "%.4f", h.div); out += buf; }
	}
	if (h.split) { out += "\tzd:i:"; append_int(out, h.split); }
}

// format.c:302-321; the line ends after rl:i -- what follows it (cg:Z, cs:Z, MD:Z) and the line's end are the caller's
void write_paf(std::string &out, const char *qname, int qlen, const Hit &h, const char *rname, int rlen, int rep_len, const uint32_t *words = nullptr)
{
	out += qname; out += '\t'; append_int(out, qlen); out += '\t'; append_int(out, h.qs); out += '\t'; append_int(out, h.qe); out += '\t';
	out += h.rev ? '-' : '+'; out += '\t'; out += rname; out += '\t'; append_int(out, rlen); out += '\t'; append_int(out, h.rs); out += '\t';
	append_int(out, h.re); out += '\t'; append_int(out, h.mlen); out += '\t'; append_int(out, h.blen); out += '\t'; append_int(out, h.mapq);
	write_tags(out, h, words);
	out += "\trl:i:"; append_int(out, rep_len);
}

// CIGAR words as "%d%c" each (format.c:326, 383)
void append_cigar(std::string &out, const uint32_t *words, int32_t n)
{
	for (int32_t k = 0; k < n; ++k) { append_int(out, words[k] >> 4); out += "MIDNSHP=XB??????"[words[k] & 0xf]; }
}

// sam_write_sq (format.c:339-351) for SEQ: on the reverse strand the bases backwards, each letter's complement in the sense of bseq.c's table, restated: the IUPAC
// pairs A/T, C/G, B/V, D/H, K/M, R/Y swap, U gives A, every other byte (N, S, W, the letters that are no code, whatever is no letter) stays; case is kept
char sam_complement(char ch)
{
	static const char *pairs = "ATCGBVDHKMRY";
	const bool lower = ch >= 'a' && ch <= 'z';
	const char up = lower ? (char)(ch - 32) : ch;
	char to = up == 'U' ? 'A' : up;
	for (int i = 0; i < 12; ++i) if (pairs[i] == up) { to = pairs[i ^ 1]; break; }
	return lower && to >= 'A' && to <= 'Z' ? (char)(to + 32) : to;
}
void append_seq(std::string &out, const char *seq, int len, bool rev)
{
	if (!rev) { out.append(seq, (size_t)len); return; }
	const size_t at = out.size();
	out.resize(at + (size_t)len);
	for (int i = 0; i < len; ++i) out[at + (size_t)i] = sam_complement(seq[len - 1 - i]);
}

// mm_write_sam3 at n_seg = 1 (format.c:389-546) for hit h of hs, the read's hits; out_flag: MM2GB_F_SOFTCLIP is looked at; cigar / n_cigar: the words the CIGAR column
// shows (the M words, or their = / X form); words: the M words for write_tags.  The line ends after the tags and SA:Z -- cs:Z / MD:Z, rl:i and the line's end are the caller's
void write_sam(std::string &out, const char *qname, int qlen, const char *seq, const Hit &h, const std::vector<Hit> &hs, const char *const *ref_names, int64_t out_flag,
               const uint32_t *cigar, int32_t n_cigar, const uint32_t *words)
{
	const int flag = (h.rev ? 0x10 : 0) | (h.parent != h.id ? 0x100 : !h.sam_pri ? 0x800 : 0);
	const bool soft = (out_flag & MM2GB_F_SOFTCLIP) != 0, whole = (flag & 0x900) == 0 || soft;
	out += qname; out += '\t'; append_int(out, flag); out += '\t'; out += ref_names[h.rid]; out += '\t'; append_int(out, h.rs + 1); out += '\t'; append_int(out, h.mapq); out += '\t';
	if (!h.has_p) out += '*';
	else {
		const int clip[2] = { h.rev ? qlen - h.qe : h.qs, h.rev ? h.qs : qlen - h.qe };
		const char clip_char = (flag & 0x800) && !soft ? 'H' : 'S';
		if (clip[0]) { append_int(out, clip[0]); out += clip_char; }
		append_cigar(out, cigar, n_cigar);
		if (clip[1]) { append_int(out, clip[1]); out += clip_char; }
	}
	out += "\t*\t0\t0\t";
	if (whole) append_seq(out, seq, qlen, h.rev);
	else if (flag & 0x100) out += '*';
	else append_seq(out, seq + h.qs, h.qe - h.qs, h.rev);
	out += "\t*";
	write_tags(out, h, words);
	if (h.parent == h.id && h.has_p && hs.size() > 1) {                                 // supplementary alignments may exist (format.c:510-533)
		bool any = false;
		for (const Hit &q : hs) {
			if (&q == &h || q.parent != q.id || !q.has_p) continue;
			if (!any) { out += "\tSA:Z:"; any = true; }
			const int ql = q.qe - q.qs, tl = q.re - q.rs, l_m = std::min(ql, tl), l_i = ql > tl ? ql - tl : 0, l_d = tl > ql ? tl - ql : 0;
			const int clip5 = q.rev ? qlen - q.qe : q.qs, clip3 = q.rev ? q.qs : qlen - q.qe;
			out += ref_names[q.rid]; out += ','; append_int(out, q.rs + 1); out += ','; out += q.rev ? '-' : '+'; out += ',';
			if (clip5) { append_int(out, clip5); out += 'S'; }
			if (l_m) { append_int(out, l_m); out += 'M'; }
			if (l_i) { append_int(out, l_i); out += 'I'; }
			if (l_d) { append_int(out, l_d); out += 'D'; }
			if (clip3) { append_int(out, clip3); out += 'S'; }
			out += ','; append_int(out, q.mapq); out += ','; append_int(out, q.blen - q.mlen + q.n_ambi); out += ';';
		}
	}
}

// the line of a read without a hit (format.c:419, 440, 481-488)
void write_sam_unmapped(std::string &out, const char *qname, int qlen, const char *seq, int rep_len)
{
	out += qname; out += "\t4\t*\t0\t0\t*\t*\t0\t0\t"; out.append(seq, (size_t)qlen); out += "\t*\trl:i:"; append_int(out, rep_len); out += '\n';
}

// a hit record as a Hit; x: its alignment, where the record has been through the alignment call
Hit hit_from(const mm2gb_reg_t &g, const mm2gb_aln_t *x = nullptr)
{
	Hit h;
	h.id = g.id; h.cnt = g.cnt; h.rid = g.rid; h.score = g.score; h.qs = g.qs; h.qe = g.qe; h.rs = g.rs; h.re = g.re; h.parent = g.parent;
	h.subsc = g.subsc; h.as = g.as; h.mlen = g.mlen; h.blen = g.blen; h.n_sub = g.n_sub; h.score0 = g.score0;
	h.mapq = 0; h.rev = (g.flags >> 10) & 1; h.hash = g.hash; h.div = g.div; h.flags = g.flags;
	h.strand_retained = x && ((g.flags >> 26) & 1);       // (bit 26 is reg_from's: it means something only after the alignment call)
	if (!x) return h;
	h.inv = (g.flags >> 11) & 1; h.split = (int)(g.flags >> 8 & 3);
	h.has_p = x->cigar_off >= 0;
	if (h.has_p) { h.dp_score = x->dp_score; h.dp_max = x->dp_max; h.dp_max2 = x->dp_max2; h.n_ambi = x->n_ambi; h.trans_strand = x->trans_strand; h.n_cigar = x->n_cigar; }
	return h;
}

// a Hit as the record the alignment call takes; strand_retained travels in bit 26
void reg_from(const Hit &h, mm2gb_reg_t &g)
{
	g.id = h.id; g.cnt = h.cnt; g.rid = h.rid; g.score = h.score; g.qs = h.qs; g.qe = h.qe; g.rs = h.rs; g.re = h.re; g.parent = h.parent; g.subsc = h.subsc; g.as = h.as;
	g.mlen = h.mlen; g.blen = h.blen; g.n_sub = h.n_sub; g.score0 = h.score0; g.hash = h.hash; g.div = h.div;
	g.flags = h.flags | (h.strand_retained ? 1u << 26 : 0u);
}

// MM_F_NO_DIAG / MM_F_NO_DUAL (map.c:211): the names of reads and references in one strcmp order (bytes as unsigned char), equal names equal ranks.  A read without
// a name has rank -1, below and unequal to every reference's: no test drops a hit of its (map.c:208 tests qname first)
void name_ranks(int32_t n_reads, const char *const *names, int32_t n_ref, const char *const *ref_names, std::vector<int32_t> &q_rank, std::vector<int32_t> &ref_rank)
{
	std::vector<std::pair<const char*, int32_t>> all;     // (name, index: reads first)
	for (int32_t r = 0; r < n_reads; ++r) if (names[r]) all.emplace_back(names[r], r);
	for (int32_t i = 0; i < n_ref; ++i) all.emplace_back(ref_names[i] ? ref_names[i] : "", n_reads + i);
	std::sort(all.begin(), all.end(), [](const std::pair<const char*, int32_t> &u, const std::pair<const char*, int32_t> &v) { return strcmp(u.first, v.first) < 0; });
	q_rank.assign((size_t)n_reads, -1); ref_rank.assign((size_t)n_ref, 0);
	int32_t rank = 0;
	for (size_t i = 0; i < all.size(); ++i) {
		if (i > 0 && strcmp(all[i - 1].first, all[i].first) != 0) ++rank;
		(all[i].second < n_reads ? q_rank[(size_t)all[i].second] : ref_rank[(size_t)(all[i].second - n_reads)]) = rank;
	}
}

// the arguments of a mapping call (eng: the one engine of mm2gb_map_reads, unused by the stream)
struct MapCall {
	mm2gb_engine_t *eng; const mm2gb_index_t *ix; int k; const char *const *ref_names; const int32_t *ref_lens; int32_t n_ref;
	const mm2gb_map_opt_t *opt; int32_t n_reads; const char *const *names; const char *const *seqs; const int32_t *lens;
	char **paf_out; int64_t *paf_len; mm2gb_map_stats_t *stats; const mm2gb_map_aln_t *aln; double *s_extra;
	const mm2gb_align_splice_opt_t *spl = nullptr;       // the spliced calls: their alignment options (aln then holds the rest of the mm2gb_map_splice_t)
	const int32_t *q_rank = nullptr, *ref_rank = nullptr; // MM_F_NO_DIAG / MM_F_NO_DUAL: the names' ranks where the caller has them already (the stream: once for all chunks)
	const mm2gb_map_sr_t *sr = nullptr;                  // mm2gb_map_reads_sr: short single-end reads (MM_F_SR); aln then holds its alignment's share, or is null
	mm2gb_map_sr_out_t *sr_out = nullptr;                // ... and where its own counts go
	const mm2gb_map_out_t *out = nullptr;                // the _out calls: SAM, = / X words (null, or zeroed: the PAF of the calls without it)
	// mm2gb_map_frags_sr: the call's units (n_reads, names, seqs, lens above) are FRAGMENTS -- the first mate's name, the mates' summed length -- and unit u's reads are
	// frag_off[u] .. frag_off[u + 1] (one or two) of frag's arrays, which hold all the call's reads whatever part of the units a chunk takes
	const struct FragReads *frag = nullptr;
	const int32_t *frag_off = nullptr;
	int n_segs(size_t u) const { return frag ? frag_off[u + 1] - frag_off[u] : 1; }
};

struct FragReads { const char *const *names; const char *const *seqs; const int32_t *lens; int32_t pe_ori; };   // seqs: a mate that pe_ori turns is turned already (map.c:1169-1171)

// what the stages of one batch share
struct Batch {
	const MapCall &c;
	mm2gb_map_opt_t opt;                                 // the call's, resolved
	const mm2gb_map_aln_t *const aln;
	const size_t R;
	const int nt;                                        // host threads
	const mm2gb_seed_opt_t so;
	mm2gb_misc_t misc;
	std::vector<mm2gb_matches_t> mt;                     // (freed on every way out)
	std::vector<std::vector<const uint64_t*>> occ;       // per read and kept seed: its occurrences, where the index holds them (copied once, into the batch's array)
	int64_t dev_seeds = 0, dev_hits = 0;                 // seeded on the device: what lies there
	std::vector<int32_t> qlen, ref_len;
	std::vector<int64_t> a_off;
	BigBuf<mm2gb_anchor_t> &anchors;                     // the engine's
	// the current chains, read where they lie: the chaining call's (ch_own) until re-chaining splices new ones into the engine's arrays
	ChainsOwner ch_own;
	BigBuf<uint64_t> first_u;                            // under MM_F_RMQ: the first chainer's result instead (splice)
	BigBuf<mm2gb_anchor_t> first_a;
	std::vector<int64_t> u_off, c_off;
	const uint64_t *u = nullptr;
	const mm2gb_anchor_t *ca = nullptr;
	std::vector<mm2gb_reg_t> regs;
	std::vector<int32_t> own_q_rank, own_ref_rank;       // MM_F_NO_DIAG / MM_F_NO_DUAL: the names' ranks, where the call did not bring them
	const int32_t *q_rank = nullptr, *ref_rank = nullptr;
	bool out_sam = false, out_eqx = false;               // the _out calls: SAM lines; = / X words
	bool resident = false;                               // the resident path runs: no anchor, chain or kept anchor on the host (u, ca, a_off's anchors stay unset)
	std::vector<mm2gb_est_err_t> est;                    // ... the walk's counts per hit record and sum_k per read instead
	std::vector<uint64_t> sum_k;
	int64_t link[2] = { 0, 0 };                          // seeded on the device: bytes the stages copied to the device / back (the MM2GB_DEBUG_PHASES line; profiles/ava_rate.py)
	std::vector<std::string> lines;
	std::vector<uint8_t> no_hit;                         // SAM: the read's line is the one of a read without a hit (not counted in n_mapped)
	mm2gb_map_stats_t st = {};
	mm2gb_map_sr_out_t sro = {};                         // the short-read path's own counts
	double *const s_extra;

	Batch(const MapCall &call, const mm2gb_map_opt_t &o)
		: c(call), opt(o), aln(call.aln), R((size_t)call.n_reads), nt(std::max(1, o.host_threads)), so{ o.mid_occ, o.max_max_occ, o.occ_dist, o.q_occ_frac }, mt(R), occ(R),
		  qlen(call.lens, call.lens + R), ref_len(call.ref_lens, call.ref_lens + call.n_ref), a_off(R + 1, 0), anchors(host_scratch(call.eng).anchors), lines(R), no_hit(R, 0), s_extra(call.s_extra)
	{
		out_sam = call.out && call.out->format == 1; out_eqx = call.out && (call.out->flag & MM2GB_F_EQX);
	}
	~Batch() { release_matches(); }
	void release_matches() { for (auto &m : mt) mm2gb_matches_free(&m); }
};

// 1. matches on host threads
int seed_on_host(Batch &B)
{
	std::atomic<int> bad(0);
	std::string why;                                      // error text is per thread: carry the first one over
	std::mutex why_lock;
	for_each_on_threads(B.R, B.nt, 1, [&](size_t r) {
		if (B.c.lens[r] <= 0) return;
		const int32_t r0 = B.c.frag ? B.c.frag_off[r] : 0;
		if (B.c.frag ? collect_matches_frag_refs(B.c.ix, B.c.n_segs(r), B.c.frag->seqs + r0, B.c.frag->lens + r0, &B.so, B.so.mid_occ, &B.mt[r], &B.occ[r])
		             : collect_matches_refs(B.c.ix, B.c.seqs[r], B.c.lens[r], &B.so, &B.mt[r], &B.occ[r])) {
			std::lock_guard<std::mutex> g(why_lock);
			if (!bad.exchange(1)) why = mm2gb_last_error();
		}
	});
	return bad ? fail(why) : 0;
}

// 1. on the device (seeding_on_device = 1): the reads go up as bytes, sketch / look-up / match selection run as kernels (seed_kernels.hip) and leave
//    the arrays step 2's kernels read where they are; what comes down is what the host's mapq and divergence code wants (rep_len, mini_pos)
// what one chaining micro-batch of the engine holds (Engine::chain_gpu slices a larger batch, and a sliced batch's chains do not lie end to end on the device)
int64_t resident_max_anchors()
{
	int64_t slice = 64 * 1000 * 1000;
	if (const char *v = getenv("MM2GB_CHAIN_SLICE_ANCHORS")) slice = std::max<int64_t>(1, atoll(v));
	return slice + slice / 2;
}

int seed_on_device(Batch &B)
{
	const size_t R = B.R;
	Engine &e = B.c.eng->e;
	// the sequences that go up: the batch's reads, or with fragments every unit's mates (the device then joins them into units again: Engine::collect_matches_device)
	const bool frags = B.c.frag != nullptr;
	const int32_t first = frags ? B.c.frag_off[0] : 0;
	const size_t S = frags ? (size_t)(B.c.frag_off[R] - first) : R;
	const int32_t *lens = frags ? B.c.frag->lens + first : B.c.lens;
	const char *const *seqs = frags ? B.c.frag->seqs + first : B.c.seqs;
	std::vector<int64_t> seq_off(S + 1, 0), frag_off(frags ? R + 1 : 0);
	for (size_t r = 0; r < S; ++r) seq_off[r + 1] = seq_off[r] + lens[r];
	for (size_t u = 0; u < frag_off.size(); ++u) frag_off[u] = B.c.frag_off[u] - first;
	if (seq_off[S] >= ((int64_t)1 << 31) - 1) return fail("mm2gb_map_reads: a batch seeded on the device is limited to 2^31 bases");
	BigBuf<uint64_t> &flat = host_scratch(B.c.eng).hits;      // (no host array of hits in this form: its memory holds the reads end to end)
	flat.resize((size_t)seq_off[S] / 8 + 1);
	char *const bases = (char*)flat.data();
	for_each_on_threads(S, B.nt, 1, [&](size_t r) { if (lens[r] > 0) memcpy(bases + seq_off[r], seqs[r], (size_t)lens[r]); });
	DevIndexView view;
	if (index_on_device(B.c.ix, e.device, &view)) return -1;
	if (e.collect_matches_device(view, B.so, (int64_t)S, seq_off.data(), bases, &B.dev_seeds, &B.dev_hits, frags ? (int64_t)R : 0, frags ? frag_off.data() : nullptr)) return -1;
	std::vector<int64_t> seed_off(R + 1, 0);
	std::vector<int32_t> rep(R, 0);
	// (the resident path walks the minimizer positions where they are: only their number per read comes down)
	B.resident = B.resident && B.dev_hits > 0 && B.dev_hits <= resident_max_anchors();
	std::vector<uint64_t> mini_pos(B.resident ? 1 : (size_t)B.dev_seeds + 1);
	if (hipMemcpy(seed_off.data(), e.sd_seed_off.ptr, (R + 1) * 8, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(rep.data(), e.sd_rep_len.ptr, R * 4, hipMemcpyDeviceToHost) != hipSuccess ||
	    (!B.resident && B.dev_seeds > 0 && hipMemcpy(mini_pos.data(), e.sd_mini_pos.ptr, (size_t)B.dev_seeds * 8, hipMemcpyDeviceToHost) != hipSuccess))
		return fail("mm2gb_map_reads: the device's matches could not be copied back");
	B.link[0] += seq_off[S] + (int64_t)(S + 1) * 8;
	B.link[1] += (int64_t)((R + 1) * 8 + R * 4) + (B.resident ? 0 : B.dev_seeds * 8);
	for (size_t r = 0; r < R; ++r) {
		const int64_t n = seed_off[r + 1] - seed_off[r];
		mm2gb_matches_t &m = B.mt[r];
		m.rep_len = rep[r]; m.n_seeds = m.n_mini_pos = (int32_t)n;
		if (B.resident) continue;
		m.mini_pos = (uint64_t*)malloc(((size_t)n + 1) * 8);
		if (!m.mini_pos) return fail("mm2gb_map_reads: out of memory");
		if (n > 0) memcpy(m.mini_pos, mini_pos.data() + seed_off[r], (size_t)n * 8);
	}
	return 0;
}

// 2. anchors, sorted: from the matches resident on the device, or from the host's matches -- on the device for large batches
//    (mm2gb_collect_seeds_gpu: matches up, anchors down, one wave sorts a read); below that the host threads are quicker: the largest
//    read's sort alone is hundreds of milliseconds for one wave, milliseconds for a core
int64_t seed_flag(const Batch &B) { return B.opt.flag & ~(int64_t)MM2GB_F_RMQ; }       // the strand bits: all that seed collection looks at

int collect_anchors(Batch &B, bool dev_seed)
{
	const size_t R = B.R;
	mm2gb_engine_t *eng = B.c.eng;
	if (dev_seed) {
		if (!B.resident) B.anchors.resize((size_t)std::max<int64_t>(B.dev_hits, 1));
		return B.c.eng->e.collect_seeds_resident(seed_flag(B), B.c.n_reads, B.dev_seeds, B.dev_hits, B.q_rank, B.c.n_ref, B.ref_len.data(), B.ref_rank, B.a_off.data(),
		                                         B.resident ? nullptr : B.anchors.data()) ? -1 : 0;
	}
	const std::vector<mm2gb_matches_t> &mt = B.mt;
	std::vector<int64_t> seed_off(R + 1, 0);
	for (size_t r = 0; r < R; ++r) seed_off[r + 1] = seed_off[r] + mt[r].n_seeds;
	std::vector<mm2gb_seed_t> seeds((size_t)seed_off[R]);
	std::vector<int64_t> hit_off((size_t)seed_off[R] + 1, 0);
	int64_t n_hits = 0;
	for (size_t r = 0; r < R; ++r) {
		if (mt[r].n_seeds) memcpy(seeds.data() + seed_off[r], mt[r].seeds, (size_t)mt[r].n_seeds * sizeof(mm2gb_seed_t));
		for (int s = 0; s < mt[r].n_seeds; ++s) { hit_off[(size_t)(seed_off[r] + s) + 1] = hit_off[(size_t)(seed_off[r] + s)] + mt[r].seeds[s].n; }
		n_hits += mt[r].n_hits;
	}
	// (the batch's two largest arrays are the engine's from call to call: a gigabyte of fresh pages costs more to touch than to fill)
	BigBuf<uint64_t> &hits = host_scratch(eng).hits;
	hits.resize((size_t)n_hits);
	uint64_t *const hits_ptr = hits.data();
	for_each_on_threads(R, B.nt, 16, [&](size_t r) {
		for (int32_t q = 0; q < mt[r].n_seeds; ++q)
			memcpy(hits_ptr + hit_off[(size_t)seed_off[r] + (size_t)q], B.occ[r][(size_t)q], (size_t)mt[r].seeds[q].n * 8);
	});
	B.anchors.resize((size_t)std::max<int64_t>(n_hits, 1));
	const bool seeds_on_device = B.opt.seeds_on_device > 0 || (B.opt.seeds_on_device == 0 && n_hits >= 400000000);
	return seeds_on_device ? mm2gb_collect_seeds_gpu(eng, seed_flag(B), B.c.n_reads, seed_off.data(), seeds.data(), hit_off.data(), hits.data(), B.qlen.data(), B.q_rank, B.c.n_ref, B.q_rank ? B.ref_len.data() : nullptr, B.ref_rank,
	                                                 B.a_off.data(), B.anchors.data())
	                       : mm2gb_collect_seeds_host(seed_flag(B), B.c.n_reads, seed_off.data(), seeds.data(), hit_off.data(), hits.data(), B.qlen.data(), B.q_rank, B.c.n_ref, B.q_rank ? B.ref_len.data() : nullptr, B.ref_rank,
	                                                  B.nt, B.a_off.data(), B.anchors.data());
}

// 3. chains on the device; map.c:393-426 for the parameters (the GPU path chains with max-chain-skip = infinity unless the options set
//    a finite one: then the engine keeps it for this call, and the re-chaining call gets it too)
int chain(Batch &B)
{
	mm2gb_engine_t *eng = B.c.eng;
	const mm2gb_map_opt_t &opt = B.opt;
	mm2gb_misc_t &misc = B.misc;
	misc.max_iter = opt.max_chain_iter; misc.max_dist_y = opt.max_gap; misc.max_dist_x = opt.max_gap_ref > 0 ? opt.max_gap_ref : opt.max_gap;
	misc.max_skip = opt.max_chain_skip; misc.bw = opt.bw; misc.min_cnt = opt.min_cnt; misc.min_score = opt.min_chain_score; misc.is_cdna = B.c.spl ? 1 : 0; misc.n_seg = 1;
	misc.chn_pen_gap = (float)(opt.chain_gap_scale * 0.01 * B.c.k); misc.chn_pen_skip = (float)(opt.chain_skip_scale * 0.01 * B.c.k);
	if (mm2gb_engine_set_misc(eng, &misc)) return -1;
	if (opt.flag & MM2GB_F_RMQ) return 0;                // (mg_lchain_rmq instead, map.c:690-692: first_chain below, which shares stage 4's fill)
	mm2gb_chains_t &ch = B.ch_own.c;
	struct ChainSkipMode {                               // the engine's own mode comes back on every way out of the chaining call
		bool &mode; const bool before;
		ChainSkipMode(bool &m, bool keep) : mode(m), before(m) { mode = keep; }
		~ChainSkipMode() { mode = before; }
	} guard(eng->e.chain_skip, opt.max_chain_skip != INT32_MAX);
	// backtrack + compaction as kernels for large batches; below that on host threads, overlapped with the device: a single huge read (a
	// tandem array) keeps one wave busy for hundreds of milliseconds where a core needs tens
	if (B.a_off[B.R] >= 200000000 ? mm2gb_chain_gpu(eng, B.c.n_reads, B.a_off.data(), B.anchors.data(), &ch, nullptr)
	                              : mm2gb_chain_host(eng, B.c.n_reads, B.a_off.data(), B.anchors.data(), B.nt, &ch, nullptr)) return -1;
	// (the chains are read where the chaining call left them -- a gigabyte of kept anchors per batch is not copied again)
	B.u_off.assign(ch.u_off, ch.u_off + B.R + 1); B.c_off.assign(ch.a_off, ch.a_off + B.R + 1);
	B.u = ch.u; B.ca = ch.a;
	return 0;
}

// ---- 4. re-chaining of long reads whose best chain leaves much of the read uncovered (map.c:697-708): the chained anchors, sorted again,
//      through mg_lchain_rmq's fill, and the new chains spliced in ----

// the reads to do again (largest first: a read is one wave's, or one thread's, work from start to end, and the call ends with its longest
// read), and their anchors end to end, sorted, in the engine's `ra` (ro: where each read's begin)
void rechain_pick(Batch &B, std::vector<int32_t> &redo, std::vector<int64_t> &ro)
{
	const std::vector<int64_t> &u_off = B.u_off, &c_off = B.c_off;
	const int32_t *lens = B.c.lens;
	if (B.opt.bw_long > B.opt.bw && !(B.opt.flag & MM2GB_F_NO_LJOIN)) {                      // map.c:698
		for (size_t r = 0; r < B.R; ++r) {
			if (u_off[r + 1] - u_off[r] <= 1) continue;
			const mm2gb_anchor_t *a = B.ca + c_off[r];
			const int st = (int32_t)a[0].y, en = (int32_t)a[(int32_t)B.u[(size_t)u_off[r]] - 1].y;
			if (lens[r] - (en - st) > B.opt.rmq_rescue_size || en - st > lens[r] * B.opt.rmq_rescue_ratio) redo.push_back((int32_t)r);
		}
	}
	std::sort(redo.begin(), redo.end(), [&](int32_t u, int32_t v) { const int64_t nu = c_off[(size_t)u + 1] - c_off[(size_t)u], nv = c_off[(size_t)v + 1] - c_off[(size_t)v]; return nu != nv ? nu > nv : u < v; });
	if (redo.empty()) return;
	ro.assign(redo.size() + 1, 0);
	for (size_t q = 0; q < redo.size(); ++q) ro[q + 1] = ro[q] + (c_off[(size_t)redo[q] + 1] - c_off[(size_t)redo[q]]);
	// (the engine's, kept between calls like the gathers of mm2gb_rmq_chain: fresh pages cost more to touch than to fill)
	BigBuf<mm2gb_anchor_t> &ra = host_scratch(B.c.eng).ra;
	ra.resize((size_t)ro.back());
	mm2gb_anchor_t *const ra_ptr = ra.data();
	for_each_on_threads(redo.size(), B.nt, 1, [&](size_t q) {
		memcpy(ra_ptr + ro[q], B.ca + c_off[(size_t)redo[q]], (size_t)(ro[q + 1] - ro[q]) * sizeof(mm2gb_anchor_t));
		sort_by_x_like_host(ra_ptr + ro[q], ra_ptr + ro[q + 1]);
	});
	if (const char *path = getenv("MM2GB_DUMP_RECHAIN")) {       // the re-chaining call's input, for profiling csrc/rmq_host.cpp off the box: offsets, then anchors
		if (FILE *fp = fopen(path, "wb")) {
			const int64_t nr = (int64_t)redo.size();
			fwrite(&nr, 8, 1, fp); fwrite(ro.data(), 8, ro.size(), fp); fwrite(ra.data(), sizeof(mm2gb_anchor_t), ra.size(), fp);
			fclose(fp);
		}
	}
}

// the new chains of the re-chained reads, where the fill's form left them
struct Refill {
	ChainsOwner rc, rc_tie;                              // rechain_on_device != 0: the one call's result, and that of the host call for the tied reads
	RmqParts parts;                                      // the default: the results of the call's three sides
	std::vector<int32_t> tied;                           // per re-chained read: done again on the host after a tie
	std::vector<unsigned char> side;                     // ... which result holds it (0: rc, 1: rc_tie, 2 + k: parts.chains[k]) ...
	std::vector<int64_t> slot;                           // ... and where
	explicit Refill(size_t n) : tied(n, 0), side(n, 0), slot(n, 0) {}
	const mm2gb_chains_t &at(size_t q) const { return side[q] == 0 ? rc.c : side[q] == 1 ? rc_tie.c : parts.chains[side[q] - 2]; }
};

// mg_lchain_rmq's fill.  Default: mm2gb_rmq_chain (csrc/rmq_hybrid.cpp) -- the kernel form takes the bulk of the reads, the host
// threads, at the same time, the few whose windows are so dense that one wave would still be on them long after the rest of the
// batch is done, and afterwards the reads the kernel reported a tie for (where the reference's answer follows from the shape of
// its tree; the host form keeps that tree's rules).  rechain_on_device = 1: every read on the device first; -1: host threads only.
// Both callers: stage 4 with bw_long on the chained anchors, sorted again, and under MM_F_RMQ stage 3 with bw on a read's raw sorted anchors
// (map.c:690-692 and 705-706 differ in that argument alone).  stage: its name in the MM2GB_DEBUG_PHASES line
int rmq_fill(Batch &B, int32_t bw, const char *stage, const int64_t *ro, size_t n, const mm2gb_anchor_t *ra, bool verbose, Refill &F)
{
	const mm2gb_map_opt_t &opt = B.opt;
	const mm2gb_rmq_param_t rp = { opt.max_gap, opt.rmq_inner_dist, bw, opt.max_chain_skip, opt.rmq_size_cap, opt.min_cnt, opt.min_chain_score, B.misc.chn_pen_gap, B.misc.chn_pen_skip };
	if (opt.rechain_on_device == 0) {
		std::vector<int32_t> where(n, 0);
		mm2gb_rmq_deal_t deal = {};
		if (rmq_chain_parts(B.c.eng, &rp, (int64_t)n, ro, ra, B.nt, F.parts, where.data(), &deal)) return -1;
		for (size_t q = 0; q < n; ++q) { F.tied[q] = where[q] == 2; F.side[q] = (unsigned char)(2 + F.parts.which[q]); F.slot[q] = F.parts.slot[q]; }
		if (verbose) fprintf(stderr, "[mm2gb] %s deal: %lld reads on the device, %d of them a whole workgroup's (%.3f s, estimated %.3f), %lld on host threads by cost (%.3f s, estimated %.3f), %lld redone after a tie (%.3f s)\n",
		                     stage, (long long)deal.n_device, (int)deal.n_team, deal.device_s, deal.est_device_s, (long long)deal.n_host_cost, deal.host_s, deal.est_host_s, (long long)deal.n_host_tie, deal.tie_s);
		return 0;
	}
	for (size_t q = 0; q < n; ++q) F.slot[q] = (int64_t)q;
	if (opt.rechain_on_device < 0) return mm2gb_rmq_chain_host(&rp, (int64_t)n, ro, ra, B.nt, &F.rc.c, F.tied.data());
	if (mm2gb_rmq_chain_gpu(B.c.eng, &rp, (int64_t)n, ro, ra, &F.rc.c, F.tied.data(), nullptr)) return -1;
	std::vector<int64_t> to(1, 0);                       // the tied reads, again on host threads
	std::vector<mm2gb_anchor_t> ta;
	for (size_t q = 0; q < n; ++q)
		if (F.tied[q]) {
			F.side[q] = 1; F.slot[q] = (int64_t)to.size() - 1;
			ta.insert(ta.end(), ra + ro[q], ra + ro[q + 1]);
			to.push_back((int64_t)ta.size());
		}
	return to.size() > 1 ? mm2gb_rmq_chain_host(&rp, (int64_t)to.size() - 1, to.data(), ta.data(), B.nt, &F.rc_tie.c, nullptr) : 0;
}

// the batch's chains with the re-chained reads' new ones in place, in the engine's arrays (touched pages); the chaining call's result goes
// (first: stage 3 under MM_F_RMQ -- there are no chains yet, a read outside `redo` has none, and the result goes to the batch's own arrays, which
// stage 4's splice then reads while it fills the engine's)
void splice(Batch &B, const std::vector<int32_t> &redo, const Refill &F, bool first = false)
{
	const size_t R = B.R;
	std::vector<int64_t> nu_off(R + 1, 0), nc_off(R + 1, 0);
	std::vector<int> which(R, -1);
	if (first) { B.u_off.assign(R + 1, 0); B.c_off.assign(R + 1, 0); }
	for (size_t q = 0; q < redo.size(); ++q) { which[(size_t)redo[q]] = (int)q; if (F.tied[q]) ++B.st.n_rmq_tied; }
	for (size_t r = 0; r < R; ++r) {
		const int q = which[r];
		if (q < 0) { nu_off[r + 1] = nu_off[r] + (B.u_off[r + 1] - B.u_off[r]); nc_off[r + 1] = nc_off[r] + (B.c_off[r + 1] - B.c_off[r]); continue; }
		const mm2gb_chains_t &from = F.at((size_t)q);
		const int64_t qq = F.slot[(size_t)q];
		nu_off[r + 1] = nu_off[r] + (from.u_off[qq + 1] - from.u_off[qq]);
		nc_off[r + 1] = nc_off[r] + (from.a_off[qq + 1] - from.a_off[qq]);
	}
	BigBuf<uint64_t> &nu = first ? B.first_u : host_scratch(B.c.eng).nu;
	BigBuf<mm2gb_anchor_t> &nc = first ? B.first_a : host_scratch(B.c.eng).nc;
	nu.resize((size_t)std::max<int64_t>(nu_off[R], 1)); nc.resize((size_t)std::max<int64_t>(nc_off[R], 1));
	uint64_t *const nu_ptr = nu.data();
	mm2gb_anchor_t *const nc_ptr = nc.data();
	// (a batch's kept anchors are a gigabyte: the copies go to all host threads)
	for_each_on_threads(R, B.nt, 32, [&](size_t r) {
		const int q = which[r];
		const mm2gb_chains_t *from = q < 0 ? nullptr : &F.at((size_t)q);
		const int64_t qq = q < 0 ? 0 : F.slot[(size_t)q];
		const uint64_t *su = q < 0 ? B.u + B.u_off[r] : from->u + from->u_off[qq];
		const mm2gb_anchor_t *sa = q < 0 ? B.ca + B.c_off[r] : from->a + from->a_off[qq];
		if (nu_off[r + 1] > nu_off[r]) memcpy(nu_ptr + nu_off[r], su, (size_t)(nu_off[r + 1] - nu_off[r]) * 8);
		if (nc_off[r + 1] > nc_off[r]) memcpy(nc_ptr + nc_off[r], sa, (size_t)(nc_off[r + 1] - nc_off[r]) * sizeof(mm2gb_anchor_t));
	});
	B.u = nu_ptr; B.ca = nc_ptr; B.u_off.swap(nu_off); B.c_off.swap(nc_off);
	mm2gb_chains_free(&B.ch_own.c);
}

// 3 under MM_F_RMQ (map.c:690-692): every read that has anchors through the same fill with bw, its raw sorted anchors where stage 2 left them
// (a read's anchors are contiguous there: the offsets of the picked reads' begins and ends are stage 2's own); the chains land where the chaining
// call's would.  A read without anchors has no chains; a batch without any is not sent.  The reads go in batch order, not largest first as
// rechain_pick sends them: the default form deals by cost itself (rmq_chain_parts), but with rechain_on_device = 1 or -1 a large contig at the
// end of a batch sets the length of the call
int first_chain(Batch &B)
{
	using clk = std::chrono::steady_clock;
	const auto t0 = clk::now();
	std::vector<int32_t> redo;
	for (size_t r = 0; r < B.R; ++r) if (B.a_off[r + 1] > B.a_off[r]) redo.push_back((int32_t)r);
	Refill F(redo.size());
	if (!redo.empty()) {
		// (the reads in between are empty, so the picked reads' anchors are end to end already: no gather)
		std::vector<int64_t> ro(redo.size() + 1, 0);
		for (size_t q = 0; q < redo.size(); ++q) ro[q + 1] = B.a_off[(size_t)redo[q] + 1] - B.a_off[(size_t)redo[0]];
		const bool verbose = getenv("MM2GB_DEBUG_PHASES") != nullptr;
		if (rmq_fill(B, B.opt.bw, "first chaining", ro.data(), redo.size(), B.anchors.data() + B.a_off[(size_t)redo[0]], verbose, F)) return -1;
		const auto t_filled = clk::now();
		splice(B, redo, F, true);
		if (verbose) fprintf(stderr, "[mm2gb] first chaining (MM_F_RMQ) %zu reads (%lld redone on the host after a tie), %lld anchors: fill %.3f s, splice %.3f s\n", redo.size(), (long long)B.st.n_rmq_tied,
		                     (long long)ro.back(), std::chrono::duration<double>(t_filled - t0).count(), std::chrono::duration<double>(clk::now() - t_filled).count());
	} else splice(B, redo, F, true);
	return 0;
}

int rechain(Batch &B)
{
	using clk = std::chrono::steady_clock;
	auto seconds = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); };
	const auto t_rechain = clk::now();
	std::vector<int32_t> redo;
	std::vector<int64_t> ro;
	rechain_pick(B, redo, ro);
	B.st.n_rechained = (int64_t)redo.size();
	const int64_t tied_before = B.st.n_rmq_tied;         // (under MM_F_RMQ the first chaining stage's ties are in the count already)
	if (!redo.empty()) {
		const auto t_sorted = clk::now();
		const bool verbose = getenv("MM2GB_DEBUG_PHASES") != nullptr;
		Refill F(redo.size());
		if (rmq_fill(B, B.opt.bw_long, "re-chaining", ro.data(), redo.size(), host_scratch(B.c.eng).ra.data(), verbose, F)) return -1;
		const auto t_filled = clk::now();
		splice(B, redo, F);
		if (verbose) fprintf(stderr, "[mm2gb] re-chaining %zu reads (%lld redone on the host after a tie), %lld anchors: sort %.3f s, fill %.3f s, splice %.3f s\n", redo.size(), (long long)(B.st.n_rmq_tied - tied_before), (long long)ro.back(),
		                     seconds(t_rechain, t_sorted), seconds(t_sorted, t_filled), seconds(t_filled, clk::now()));
	}
	B.st.n_chains = B.u_off[B.R];
	return 0;
}

// 5. hit records on the device (hit.c:52-88); the hash of map.c:660-662
int hit_records(Batch &B)
{
	std::vector<uint32_t> hash(B.R);
	for (size_t r = 0; r < B.R; ++r) {
		uint32_t h = B.c.names[r] ? name_hash(B.c.names[r]) : 0;
		h ^= wang((uint32_t)B.c.lens[r]) + wang((uint32_t)B.opt.seed);
		hash[r] = wang(h);
	}
	B.regs.resize((size_t)std::max<int64_t>(B.u_off[B.R], 1));
	mm2gb_chains_t view; view.u_off = B.u_off.data(); view.u = const_cast<uint64_t*>(B.u); view.a_off = B.c_off.data(); view.a = const_cast<mm2gb_anchor_t*>(B.ca);
	return mm2gb_gen_regs_gpu(B.c.eng, B.c.n_reads, &view, B.qlen.data(), hash.data(), 0, B.regs.data());
}

// 3 and 5 of the resident path (seeding_on_device = 2): the anchors are where step 2 left them on the device, the engine chains them there with the mode chain() sets,
// and hit records and the walk's counts are all that comes down
int chain_resident(Batch &B)
{
	mm2gb_engine_t *eng = B.c.eng;
	const mm2gb_map_opt_t &opt = B.opt;
	mm2gb_misc_t &misc = B.misc;
	misc.max_iter = opt.max_chain_iter; misc.max_dist_y = opt.max_gap; misc.max_dist_x = opt.max_gap_ref > 0 ? opt.max_gap_ref : opt.max_gap;
	misc.max_skip = opt.max_chain_skip; misc.bw = opt.bw; misc.min_cnt = opt.min_cnt; misc.min_score = opt.min_chain_score; misc.is_cdna = 0; misc.n_seg = 1;
	misc.chn_pen_gap = (float)(opt.chain_gap_scale * 0.01 * B.c.k); misc.chn_pen_skip = (float)(opt.chain_skip_scale * 0.01 * B.c.k);
	if (mm2gb_engine_set_misc(eng, &misc)) return -1;
	const bool before = eng->e.chain_skip;
	eng->e.chain_skip = opt.max_chain_skip != INT32_MAX;
	int64_t n_kept = 0;
	const int rc = eng->e.resident_chain(B.c.n_reads, B.a_off[B.R], &B.st.n_chains, &n_kept);
	eng->e.chain_skip = before;
	B.link[1] += (int64_t)(B.R + 1) * 8 + 16;            // step 2's offsets, the chains' totals
	if (B.q_rank) B.link[0] += (int64_t)B.R * 4 + (int64_t)B.c.n_ref * 8;
	return rc;
}

int hit_records_resident(Batch &B)
{
	const size_t R = B.R, n_u = (size_t)B.st.n_chains;
	std::vector<uint32_t> hash(R);
	for (size_t r = 0; r < R; ++r) {
		uint32_t h = B.c.names[r] ? name_hash(B.c.names[r]) : 0;
		h ^= wang((uint32_t)B.c.lens[r]) + wang((uint32_t)B.opt.seed);
		hash[r] = wang(h);
	}
	B.u_off.assign(R + 1, 0);
	B.regs.resize(std::max<size_t>(n_u, 1)); B.est.resize(std::max<size_t>(n_u, 1)); B.sum_k.assign(R, 0);
	if (n_u == 0) return 0;                               // (no chain in the batch: no line either)
	if (B.c.eng->e.resident_regs(B.c.n_reads, B.st.n_chains, hash.data(), B.c.n_ref, B.ref_len.data(), B.u_off.data(), B.regs.data(), B.est.data(), B.sum_k.data())) return -1;
	if (B.u_off[R] != B.st.n_chains) return fail("mm2gb_map_reads: the resident chains' offsets do not add up to their total");
	B.link[0] += (int64_t)R * 4 + (int64_t)B.c.n_ref * 4;
	B.link[1] += (int64_t)(R + 1) * 8 + (int64_t)R * 8 + (int64_t)n_u * (int64_t)(sizeof(mm2gb_reg_t) + sizeof(mm2gb_est_err_t));
	return 0;
}

// ---- short single-end reads (mm2gb_map_reads_sr; minimap2 -x sr without base-level alignment): stages 2 and 3 in their MM_F_SR forms ----

// 2 for a list of reads (ascending), from the host's matches: anchors in the heap's order under MM_F_HEAP_SORT (map.c:229-293), sorted otherwise; on the device or
// on host threads as seeds_on_device says.  a_off: the list's offsets (one more than reads); out: its anchors
int collect_anchors_sr(Batch &B, const std::vector<int32_t> &reads, std::vector<int64_t> &a_off, BigBuf<mm2gb_anchor_t> &out, int64_t *n_tied)
{
	const size_t n = reads.size();
	const std::vector<mm2gb_matches_t> &mt = B.mt;
	std::vector<int64_t> seed_off(n + 1, 0);
	std::vector<int32_t> qlen(n);
	for (size_t q = 0; q < n; ++q) { seed_off[q + 1] = seed_off[q] + mt[(size_t)reads[q]].n_seeds; qlen[q] = B.qlen[(size_t)reads[q]]; }
	std::vector<mm2gb_seed_t> seeds((size_t)seed_off[n]);
	std::vector<int64_t> hit_off((size_t)seed_off[n] + 1, 0);
	for (size_t q = 0; q < n; ++q) {
		const mm2gb_matches_t &m = mt[(size_t)reads[q]];
		if (m.n_seeds) memcpy(seeds.data() + seed_off[q], m.seeds, (size_t)m.n_seeds * sizeof(mm2gb_seed_t));
		for (int s = 0; s < m.n_seeds; ++s) hit_off[(size_t)(seed_off[q] + s) + 1] = hit_off[(size_t)(seed_off[q] + s)] + m.seeds[s].n;
	}
	const int64_t n_hits = hit_off[(size_t)seed_off[n]];
	BigBuf<uint64_t> &hits = host_scratch(B.c.eng).hits;
	hits.resize((size_t)std::max<int64_t>(n_hits, 1));
	uint64_t *const hits_ptr = hits.data();
	for_each_on_threads(n, B.nt, 64, [&](size_t q) {
		const size_t r = (size_t)reads[q];
		for (int32_t s = 0; s < mt[r].n_seeds; ++s) memcpy(hits_ptr + hit_off[(size_t)seed_off[q] + (size_t)s], B.occ[r][(size_t)s], (size_t)mt[r].seeds[s].n * 8);
	});
	out.resize((size_t)std::max<int64_t>(n_hits, 1));
	a_off.assign(n + 1, 0);
	const bool on_device = B.opt.seeds_on_device > 0 || (B.opt.seeds_on_device == 0 && n_hits >= 400000000);
	const int64_t flag = seed_flag(B);
	*n_tied = 0;
	if (B.opt.flag & MM2GB_F_HEAP_SORT)
		return on_device ? mm2gb_collect_seeds_heap_gpu(B.c.eng, flag, (int64_t)n, seed_off.data(), seeds.data(), hit_off.data(), hits_ptr, qlen.data(), nullptr, 0, nullptr, nullptr, a_off.data(), out.data(), n_tied)
		                 : mm2gb_collect_seeds_heap_host(flag, (int64_t)n, seed_off.data(), seeds.data(), hit_off.data(), hits_ptr, qlen.data(), nullptr, 0, nullptr, nullptr, B.nt, a_off.data(), out.data(), n_tied);
	return on_device ? mm2gb_collect_seeds_gpu(B.c.eng, flag, (int64_t)n, seed_off.data(), seeds.data(), hit_off.data(), hits_ptr, qlen.data(), nullptr, 0, nullptr, nullptr, a_off.data(), out.data())
	                 : mm2gb_collect_seeds_host(flag, (int64_t)n, seed_off.data(), seeds.data(), hit_off.data(), hits_ptr, qlen.data(), nullptr, 0, nullptr, nullptr, B.nt, a_off.data(), out.data());
}

// the chains of a batch whose reads were chained in several calls: the calls' results, and per read which one holds it and where
struct SrChains {
	std::vector<std::unique_ptr<ChainsOwner>> parts;
	std::vector<int32_t> part;
	std::vector<int64_t> slot;
	int64_t n_calls = 0;
	explicit SrChains(size_t R) : part(R, -1), slot(R, 0) {}
};

// 3 for a list of reads with their anchors: under MM_F_SR the gaps depend on the read's length (map.c:678-686) -- max_dist_y = max(qlen, max_gap),
// max_dist_x = max(max_frag_len - qlen, max_gap), or max_gap_ref where it is set -- and the engine takes both per call.  dq <= qlen always holds, so any
// max_dist_y >= the longest read gives lchain.c:118-120 the same answers: one value for the batch.  max_dist_x moves the window and max_ii (lchain.c:172-173,
// 190) and must be exact: one chaining call per distinct value among the list's reads that have anchors, each over those reads' anchors gathered end to
// end (a list with one value goes as it lies).  Reads of one length share a value, and so do all reads of max_frag_len - max_gap bases or more.
int chain_groups_sr(Batch &B, const std::vector<int32_t> &reads, const std::vector<int64_t> &a_off, const mm2gb_anchor_t *anchors, SrChains &S)
{
	// With fragments (mm2gb_map_frags_sr) a unit of two mates is chained at n_seg = 2, where max_dist_y also bounds the reference gap between anchors of different
	// mates (lchain.c:121: same segment or not, dr > max_dist_y is out) and must be exact as well: max(qlen_sum, max_gap).  So the key of a call is (n_seg, max_dist_x,
	// max_dist_y); the units of one read share one max_dist_y as ever and are grouped as ever.
	const mm2gb_map_opt_t &opt = B.opt;
	struct Key { int32_t n_seg, max_x, max_y, second; bool same(const Key &o) const { return n_seg == o.n_seg && max_x == o.max_x && max_y == o.max_y; } };
	std::vector<Key> key;                                    // (the call's parameters, place in the list) of the reads that have anchors
	int32_t longest = 0;
	for (size_t q = 0; q < reads.size(); ++q) if (B.c.n_segs((size_t)reads[q]) == 1) longest = std::max(longest, B.qlen[(size_t)reads[q]]);
	for (size_t q = 0; q < reads.size(); ++q) {
		const int32_t len = B.qlen[(size_t)reads[q]], n_seg = B.c.n_segs((size_t)reads[q]);
		if (a_off[q + 1] > a_off[q]) key.push_back({ n_seg, opt.max_gap_ref > 0 ? opt.max_gap_ref : std::max(B.c.sr->max_frag_len > 0 ? B.c.sr->max_frag_len - len : opt.max_gap, opt.max_gap),
		                                             std::max(n_seg == 1 ? longest : len, opt.max_gap), (int32_t)q });
	}
	std::sort(key.begin(), key.end(), [](const Key &u, const Key &v) { return u.n_seg != v.n_seg ? u.n_seg < v.n_seg : u.max_x != v.max_x ? u.max_x < v.max_x : u.max_y != v.max_y ? u.max_y < v.max_y : u.second < v.second; });
	mm2gb_misc_t &misc = B.misc;
	misc.max_iter = opt.max_chain_iter;
	misc.max_skip = opt.max_chain_skip; misc.bw = opt.bw; misc.min_cnt = opt.min_cnt; misc.min_score = opt.min_chain_score; misc.is_cdna = 0; misc.n_seg = 1;
	misc.chn_pen_gap = (float)(opt.chain_gap_scale * 0.01 * B.c.k); misc.chn_pen_skip = (float)(opt.chain_skip_scale * 0.01 * B.c.k);
	struct ChainSkipMode {
		bool &mode; const bool before;
		ChainSkipMode(bool &m, bool keep) : mode(m), before(m) { mode = keep; }
		~ChainSkipMode() { mode = before; }
	} guard(B.c.eng->e.chain_skip, opt.max_chain_skip != INT32_MAX);
	std::vector<int64_t> go;
	std::vector<mm2gb_anchor_t> ga;
	for (size_t i = 0; i < key.size();) {
		size_t j = i;
		while (j < key.size() && key[j].same(key[i])) ++j;
		misc.max_dist_x = key[i].max_x; misc.max_dist_y = key[i].max_y; misc.n_seg = key[i].n_seg;
		if (mm2gb_engine_set_misc(B.c.eng, &misc)) return -1;
		const bool whole = i == 0 && j == key.size();        // one value: the list's anchors as they lie (the reads without anchors are empty reads of the call)
		const int64_t n = whole ? (int64_t)reads.size() : (int64_t)(j - i);
		if (!whole) {
			go.assign((size_t)n + 1, 0);
			for (size_t t = i; t < j; ++t) go[t - i + 1] = go[t - i] + (a_off[(size_t)key[t].second + 1] - a_off[(size_t)key[t].second]);
			ga.resize((size_t)go.back());
			for (size_t t = i; t < j; ++t) memcpy(ga.data() + go[t - i], anchors + a_off[(size_t)key[t].second], (size_t)(go[t - i + 1] - go[t - i]) * sizeof(mm2gb_anchor_t));
		}
		S.parts.emplace_back(new ChainsOwner);
		if (mm2gb_chain_host(B.c.eng, n, whole ? a_off.data() : go.data(), whole ? anchors : ga.data(), B.nt, &S.parts.back()->c, nullptr)) return -1;
		++S.n_calls;
		for (size_t t = i; t < j; ++t) { const size_t r = (size_t)reads[(size_t)key[t].second]; S.part[r] = (int32_t)S.parts.size() - 1; S.slot[r] = whole ? key[t].second : (int64_t)(t - i); }
		i = j;
	}
	return 0;
}

// 2 and 3 under MM_F_SR, with the rescue of map.c:708-731: if max_occ > mid_occ, the reads with rep_len > 0 that are left without a chain (for one segment that is
// all n_chained_segs < n_segs can mean) get their matches again with max_occ in mid_occ's place -- that round's rep_len and mini_pos replace the first's --, their
// anchors again and are chained again, as one more batch.  Then every read's chains end to end in the batch's own arrays, where stage 5 reads them
//      dev_seed: the first round's matches lie on the device and its anchors come from them there (Engine::collect_seeds_heap_resident); the rescue's few reads are
//      seeded on host threads as ever
int anchors_and_chains_sr(Batch &B, bool dev_seed)
{
	const size_t R = B.R;
	std::vector<int32_t> all(R);
	for (size_t r = 0; r < R; ++r) all[r] = (int32_t)r;
	int64_t tied = 0, tied2 = 0;
	if (dev_seed) {
		B.anchors.resize((size_t)std::max<int64_t>(B.dev_hits, 1));
		Engine &e = B.c.eng->e;
		if ((B.opt.flag & MM2GB_F_HEAP_SORT) ? e.collect_seeds_heap_resident(seed_flag(B), B.c.n_reads, B.dev_seeds, B.dev_hits, B.a_off.data(), B.anchors.data(), &tied)
		                                     : e.collect_seeds_resident(seed_flag(B), B.c.n_reads, B.dev_seeds, B.dev_hits, nullptr, B.c.n_ref, B.ref_len.data(), nullptr, B.a_off.data(), B.anchors.data())) return -1;
	} else
	if (collect_anchors_sr(B, all, B.a_off, B.anchors, &tied)) return -1;
	B.st.n_anchors = B.a_off[R];
	SrChains S(R);
	if (chain_groups_sr(B, all, B.a_off, B.anchors.data(), S)) return -1;
	auto n_chains = [&](size_t r) { return S.part[r] < 0 ? (int64_t)0 : S.parts[(size_t)S.part[r]]->c.u_off[S.slot[r] + 1] - S.parts[(size_t)S.part[r]]->c.u_off[S.slot[r]]; };
	// a fragment of two mates also goes again when its best-scoring chain -- the first with the strictly largest score -- holds anchors of one mate only (map.c:710-720)
	auto lacks_mate = [&](size_t r) {
		const mm2gb_chains_t &c = S.parts[(size_t)S.part[r]]->c;
		const uint64_t *u = c.u + c.u_off[S.slot[r]];
		const mm2gb_anchor_t *a = c.a + c.a_off[S.slot[r]];
		int64_t best = 0, best_i = -1, best_off = -1, off = 0;
		for (int64_t i = 0; i < n_chains(r); ++i) {
			if (best < (int64_t)(u[i] >> 32)) { best = (int64_t)(u[i] >> 32); best_i = i; best_off = off; }
			off += (uint32_t)u[i];
		}
		if (best_i < 0) return false;
		int n_chained = 1;
		for (int64_t i = 1; i < (int64_t)(uint32_t)u[best_i]; ++i) if ((a[best_off + i].y >> 48 & 0xff) != (a[best_off + i - 1].y >> 48 & 0xff)) ++n_chained;
		return n_chained < B.c.n_segs(r);
	};
	std::vector<int32_t> redo;
	if (B.c.sr->max_occ > B.opt.mid_occ)
		for (size_t r = 0; r < R; ++r) if (B.mt[r].rep_len > 0 && (n_chains(r) == 0 || (B.c.n_segs(r) > 1 && lacks_mate(r)))) redo.push_back((int32_t)r);
	std::vector<int64_t> a_off2;
	BigBuf<mm2gb_anchor_t> anchors2;
	if (!redo.empty()) {
		mm2gb_seed_opt_t so = B.so;
		so.mid_occ = B.c.sr->max_occ;
		std::atomic<int> bad(0);
		std::string why;
		std::mutex why_lock;
		for_each_on_threads(redo.size(), B.nt, 1, [&](size_t q) {
			const size_t r = (size_t)redo[q];
			mm2gb_matches_free(&B.mt[r]);
			const int32_t r0 = B.c.frag ? B.c.frag_off[r] : 0;      // (two mates: the q-occurrence filter keeps mid_occ -- map.c:664 runs it once, before either round)
			if (B.c.n_segs(r) > 1 ? collect_matches_frag_refs(B.c.ix, 2, B.c.frag->seqs + r0, B.c.frag->lens + r0, &so, B.so.mid_occ, &B.mt[r], &B.occ[r])
			                      : collect_matches_refs(B.c.ix, B.c.seqs[r], B.c.lens[r], &so, &B.mt[r], &B.occ[r])) {
				std::lock_guard<std::mutex> g(why_lock);
				if (!bad.exchange(1)) why = mm2gb_last_error();
			}
		});
		if (bad) return fail(why);
		if (collect_anchors_sr(B, redo, a_off2, anchors2, &tied2)) return -1;
		B.st.n_anchors += a_off2.back();
		for (int32_t r : redo) S.part[(size_t)r] = -1;
		if (chain_groups_sr(B, redo, a_off2, anchors2.data(), S)) return -1;
	}
	B.sro.n_rescued = (int64_t)redo.size();
	B.u_off.assign(R + 1, 0); B.c_off.assign(R + 1, 0);
	for (size_t r = 0; r < R; ++r) {
		B.u_off[r + 1] = B.u_off[r] + n_chains(r);
		if (S.part[r] >= 0) { const mm2gb_chains_t &c = S.parts[(size_t)S.part[r]]->c; B.c_off[r + 1] = c.a_off[S.slot[r] + 1] - c.a_off[S.slot[r]]; }
		B.c_off[r + 1] += B.c_off[r];
	}
	B.first_u.resize((size_t)std::max<int64_t>(B.u_off[R], 1)); B.first_a.resize((size_t)std::max<int64_t>(B.c_off[R], 1));
	uint64_t *const nu = B.first_u.data();
	mm2gb_anchor_t *const nc = B.first_a.data();
	for_each_on_threads(R, B.nt, 256, [&](size_t r) {
		if (S.part[r] < 0) return;
		const mm2gb_chains_t &c = S.parts[(size_t)S.part[r]]->c;
		const int64_t q = S.slot[r];
		if (B.u_off[r + 1] > B.u_off[r]) memcpy(nu + B.u_off[r], c.u + c.u_off[q], (size_t)(B.u_off[r + 1] - B.u_off[r]) * 8);
		if (B.c_off[r + 1] > B.c_off[r]) memcpy(nc + B.c_off[r], c.a + c.a_off[q], (size_t)(B.c_off[r + 1] - B.c_off[r]) * sizeof(mm2gb_anchor_t));
	});
	B.u = nu; B.ca = nc;
	B.st.n_chains = B.u_off[R];
	B.sro.n_tied_reads = tied + tied2; B.sro.n_chain_calls = S.n_calls;
	if (getenv("MM2GB_DEBUG_PHASES"))
		fprintf(stderr, "[mm2gb] sr: %lld chaining calls, %lld reads through the max_occ rescue, %lld reads with equal index entries\n", (long long)S.n_calls, (long long)redo.size(), (long long)(tied + tied2));
	return 0;
}

// 6 under MM_F_SR without an alignment: mm_set_parent and mm_select_sub as ever, no mm_est_err and no mm_filter_strand_retained (map.c:750: div stays -1, no dv:f),
// mm_set_mapq, and under MM_F_NO_PRINT_2ND no line for a hit that is not its own parent (map.c:1359)
void finish_reads_sr(Batch &B)
{
	const mm2gb_map_opt_t &opt = B.opt;
	for_each_on_threads(B.R, B.nt, 64, [&](size_t r) {
		std::vector<Hit> hs;
		for (int64_t j = B.u_off[r]; j < B.u_off[r + 1]; ++j) hs.push_back(hit_from(B.regs[(size_t)j]));
		if (hs.empty()) return;
		set_parent(opt.mask_level, opt.mask_len, hs, false);
		select_sub(opt.pri_ratio, B.c.k * 2, opt.best_n, true, (int)(opt.max_gap * 0.8), hs);
		set_mapq(hs, opt.min_chain_score, B.mt[r].rep_len, 1, true);
		for (const Hit &h : hs) {
			if ((opt.flag & MM2GB_F_NO_PRINT_2ND) && h.id != h.parent) continue;
			write_paf(B.lines[r], B.c.names[r] ? B.c.names[r] : "*", B.c.lens[r], h, B.c.ref_names[h.rid], B.c.ref_lens[h.rid], B.mt[r].rep_len);
			B.lines[r] += '\n';
		}
	});
}

// ---- fragments of two mates (mm2gb_map_frags_sr; minimap2 -x sr on paired ends without base-level alignment): stage 6 ----

// pe.c:6-43: mm_select_sub for a fragment.  A secondary stays if it is within min_diff of its parent; else, where it lies close to its parent on the reference (same
// strand and sequence, within the mates' lengths + max_gap_ref), if it has pri1 of the parent's score; else pri_ratio of it -- but pri2 where the parent spans the mates'
// boundary and the secondary does not; at most best_n of them.  (In place like the reference: r[parent] is read from the array as squeezed so far.)
void select_sub_multi(float pri_ratio, float pri1, float pri2, int max_gap_ref, int min_diff, int best_n, int n_segs, const int32_t *qlens, std::vector<Hit> &r)
{
	if (!(pri_ratio > 0.0f) || r.empty()) return;
	const size_t n = r.size();
	const int max_dist = n_segs == 2 ? qlens[0] + qlens[1] + max_gap_ref : 0;
	size_t k = 0;
	int n_2nd = 0;
	for (size_t i = 0; i < n; ++i) {
		bool keep = false;
		if (r[i].parent == (int)i) keep = true;
		else if (r[i].score + min_diff >= r[(size_t)r[i].parent].score) keep = true;
		else {
			const Hit &p = r[(size_t)r[i].parent], &q = r[i];
			if (p.rev == q.rev && p.rid == q.rid && q.re - p.rs < max_dist && p.re - q.rs < max_dist) keep = q.score >= p.score * pri1;
			else {
				const bool par_both = n_segs == 2 && p.qs < qlens[0] && p.qe > qlens[0], chi_both = n_segs == 2 && q.qs < qlens[0] && q.qe > qlens[0];
				keep = q.score >= p.score * (chi_both || chi_both == par_both ? pri_ratio : pri2);
			}
		}
		if (keep && r[i].parent != (int)i && n_2nd++ >= best_n) keep = false;
		if (keep) r[k++] = r[i];
	}
	if (k == n) return;
	r.resize(k); sync_hits(r);
	bool first = true;                                     // mm_set_sam_pri at the end of mm_sync_regs (hit.c:220-229, 252): the record's bit 12, which no PAF line shows
	for (Hit &h : r) { h.sam_pri = h.id == h.parent && first; if (h.sam_pri) first = false; h.flags = (h.flags & ~(1u << 12)) | (h.sam_pri ? 1u << 12 : 0u); }
}

uint64_t hit_hash64(uint64_t key)                          // hit.c:40-50
{
	key = (~key + (key << 21)); key = key ^ key >> 24; key = ((key + (key << 3)) + (key << 8)); key = key ^ key >> 14;
	key = ((key + (key << 2)) + (key << 4)); key = key ^ key >> 28; key = (key + (key << 31));
	return key;
}

// mm_gen_regs (hit.c:52-88) on the host, for the few chains of one mate (the batch's fragment chains go through the device form, stage 5): best score first, ties by the
// hash of the chain's first anchor; as: where the chain's anchors begin in a
void gen_regs_host(uint32_t hash, int qlen, const std::vector<uint64_t> &u, const mm2gb_anchor_t *a, std::vector<Hit> &out)
{
	out.clear();
	std::vector<mm2gb_anchor_t> z(u.size());               // (a pair of words sorted by the first, like an anchor)
	int64_t k = 0;
	for (size_t i = 0; i < u.size(); ++i) {
		const uint32_t h = (uint32_t)hit_hash64((hit_hash64(a[k].x) + hit_hash64(a[k].y)) ^ hash);
		z[i].x = u[i] ^ h; z[i].y = (uint64_t)k << 32 | (uint32_t)u[i];
		k += (uint32_t)u[i];
	}
	sort_by_x_like_host(z.data(), z.data() + z.size());
	for (size_t i = 0; i < z.size(); ++i) {
		const mm2gb_anchor_t &zi = z[z.size() - 1 - i];
		Hit h = {};
		h.id = (int)i; h.parent = PARENT_UNSET; h.score = h.score0 = (int)(zi.x >> 32); h.hash = (uint32_t)zi.x; h.cnt = (int)(uint32_t)zi.y; h.as = (int)(zi.y >> 32); h.div = -1.0f;
		const mm2gb_anchor_t *f = a + h.as, *l = f + h.cnt - 1;
		const int q_span = (int)(f->y >> 32 & 0xff);
		h.rev = f->x >> 63; h.rid = (int)(f->x << 1 >> 33);
		h.rs = (int32_t)f->x + 1 > q_span ? (int32_t)f->x + 1 - q_span : 0; h.re = (int32_t)l->x + 1;
		if (!h.rev) { h.qs = (int32_t)f->y + 1 - q_span; h.qe = (int32_t)l->y + 1; }
		else { h.qs = qlen - ((int32_t)l->y + 1); h.qe = qlen - ((int32_t)f->y + 1 - q_span); }
		h.mlen = h.blen = q_span;                           // mm_cal_fuzzy_len (hit.c:8-20)
		for (int j = 1; j < h.cnt; ++j) {
			const int span = (int)(f[j].y >> 32 & 0xff), tl = (int32_t)f[j].x - (int32_t)f[j - 1].x, ql = (int32_t)f[j].y - (int32_t)f[j - 1].y;
			h.blen += tl > ql ? tl : ql;
			h.mlen += tl > span && ql > span ? span : tl < ql ? tl : ql;
		}
		h.flags = h.rev ? 1u << 10 : 0u;
		out.push_back(h);
	}
}

// mm_seg_gen (hit.c:331-385): a fragment's kept records split into per-mate hits.  Every anchor goes to its mate's list (y >> 48: the segment id) with its query
// position in the mate's own coordinates -- lowered by the lengths of the mates before it, on the reverse strand by those of the mates after it --; a per-mate chain is
// the fragment record's score over the mate's share of its anchors, the empty ones squeezed out; then mm_gen_regs per mate with the mate's length and the fragment's hash,
// seg_split and seg_id set (mm_reg1_t's bits 15 and 16-23).  a: the fragment's kept anchors, where the records' `as` count from.
void seg_gen(uint32_t hash, int n_segs, const int32_t *qlens, const std::vector<Hit> &r0, const mm2gb_anchor_t *a, std::vector<Hit> *regs, std::vector<mm2gb_anchor_t> *seg_a)
{
	int acc[3] = { 0, 0, 0 };
	for (int s = 1; s <= n_segs; ++s) acc[s] = acc[s - 1] + qlens[s - 1];
	const int qlen_sum = acc[n_segs];
	for (int s = 0; s < n_segs; ++s) {
		std::vector<uint64_t> u;
		seg_a[s].clear();
		for (const Hit &h : r0) {
			uint32_t n = 0;
			for (int j = 0; j < h.cnt; ++j) {
				mm2gb_anchor_t a1 = a[h.as + j];
				if ((int)(a1.y >> 48 & 0xff) != s) continue;
				a1.y -= a1.x >> 63 ? (uint64_t)(qlen_sum - (qlens[s] + acc[s])) : (uint64_t)acc[s];
				seg_a[s].push_back(a1); ++n;
			}
			if (n) u.push_back((uint64_t)h.score << 32 | n);
		}
		gen_regs_host(hash, qlens[s], u, seg_a[s].data(), regs[s]);
		for (Hit &h : regs[s]) h.flags |= 1u << 15 | (uint32_t)s << 16;
	}
}

// 6 for a batch of fragments: a unit of one read as finish_reads_sr has it; a unit of two mates through mm_select_sub_multi and mm_seg_gen, then per mate mm_set_parent and
// mm_set_mapq with the fragment's rep_len (map.c:749, 761-768), the hits of a mate that pe_ori turned flipped back (map.c:1188-1199), and the lines of mate 0, then mate 1
void finish_frags_sr(Batch &B)
{
	const mm2gb_map_opt_t &opt = B.opt;
	const FragReads &fr = *B.c.frag;
	for_each_on_threads(B.R, B.nt, 64, [&](size_t r) {
		std::vector<Hit> hs;
		for (int64_t j = B.u_off[r]; j < B.u_off[r + 1]; ++j) hs.push_back(hit_from(B.regs[(size_t)j]));
		if (hs.empty()) return;
		const int32_t r0 = B.c.frag_off[r], n_segs = B.c.n_segs(r), rep_len = B.mt[r].rep_len;
		set_parent(opt.mask_level, opt.mask_len, hs, false);
		auto lines = [&](const std::vector<Hit> &of, int32_t read) {
			for (const Hit &h : of) {
				if ((opt.flag & MM2GB_F_NO_PRINT_2ND) && h.id != h.parent) continue;
				write_paf(B.lines[r], fr.names[read] ? fr.names[read] : "*", fr.lens[read], h, B.c.ref_names[h.rid], B.c.ref_lens[h.rid], rep_len);
				B.lines[r] += '\n';
			}
		};
		if (n_segs == 1) {
			select_sub(opt.pri_ratio, B.c.k * 2, opt.best_n, true, (int)(opt.max_gap * 0.8), hs);
			set_mapq(hs, opt.min_chain_score, rep_len, 1, true);
			lines(hs, r0);
			return;
		}
		const int32_t *qlens = fr.lens + r0;
		const int32_t max_gap_ref = opt.max_gap_ref > 0 ? opt.max_gap_ref : std::max(B.c.sr->max_frag_len > 0 ? B.c.sr->max_frag_len - B.c.lens[r] : opt.max_gap, opt.max_gap);   // (the chaining call's max_dist_x)
		select_sub_multi(opt.pri_ratio, 0.2f, 0.7f, max_gap_ref, B.c.k * 2, opt.best_n, n_segs, qlens, hs);
		std::vector<Hit> regs[2];
		std::vector<mm2gb_anchor_t> seg_a[2];
		const uint32_t hash = wang((B.c.names[r] ? name_hash(B.c.names[r]) : 0) ^ (wang((uint32_t)B.c.lens[r]) + wang((uint32_t)opt.seed)));    // map.c:659-661, as hit_records has it
		seg_gen(hash, n_segs, qlens, hs, B.ca + B.c_off[r], regs, seg_a);
		for (int s = 0; s < n_segs; ++s) {
			set_parent(opt.mask_level, opt.mask_len, regs[s], false);
			set_mapq(regs[s], opt.min_chain_score, rep_len, 1, true);
			if ((s == 0 && (fr.pe_ori >> 1 & 1)) || (s == 1 && (fr.pe_ori & 1)))
				for (Hit &h : regs[s]) { const int t = h.qs; h.qs = qlens[s] - h.qe; h.qe = qlens[s] - t; h.rev = !h.rev; }
			lines(regs[s], r0 + s);
		}
	});
}

// ---- 6. per read on the host ----

// the hits of a read up to mm_filter_strand_retained (map.c:749-752)
void chain_hits(const Batch &B, size_t r, std::vector<Hit> &hs)
{
	const mm2gb_map_opt_t &opt = B.opt;
	hs.clear();
	for (int64_t j = B.u_off[r]; j < B.u_off[r + 1]; ++j) { hs.push_back(hit_from(B.regs[(size_t)j])); hs.back().src = (int)(j - B.u_off[r]); }
	if (hs.empty()) return;
	if (!(opt.flag & MM2GB_F_ALL_CHAINS)) {                                                           // map.c:335
		set_parent(opt.mask_level, opt.mask_len, hs, false);                                          // map.c:336
		select_sub(opt.pri_ratio, B.c.k * 2, opt.best_n, true, (int)(opt.max_gap * 0.8), hs);          // map.c:337
	}
	if (B.c.sr) return;                                                                               // map.c:750: neither under MM_F_SR
	if (B.resident) divergence_from_counts(hs, B.est.data() + B.u_off[r], B.sum_k[r], B.mt[r].n_mini_pos);
	else estimate_divergence(B.c.lens[r], B.ref_len, hs, B.ca + B.c_off[r], B.mt[r].n_mini_pos, B.mt[r].mini_pos);   // map.c:751
	filter_strand_retained(hs);                                                                       // map.c:752
}

void paf_line(Batch &B, size_t r, const Hit &h, const uint32_t *words = nullptr)
{
	write_paf(B.lines[r], B.c.names[r] ? B.c.names[r] : "*", B.c.lens[r], h, B.c.ref_names[h.rid], B.c.ref_lens[h.rid], B.mt[r].rep_len, words);
}

// without an alignment: mapping quality and the lines
void finish_reads(Batch &B)
{
	std::atomic<size_t> next(0);
	run_on_threads(B.nt, [&](int) {
		std::vector<Hit> hs;                                 // a worker's own
		for (size_t r; (r = next.fetch_add(1)) < B.R;) {
			chain_hits(B, r, hs);
			set_mapq(hs, B.opt.min_chain_score, B.mt[r].rep_len);                                       // map.c:758
			for (const Hit &h : hs) { paf_line(B, r, h); B.lines[r] += '\n'; }
		}
	});
}

// with one: what 6a, 6b and 6c share
struct Aligned {
	std::vector<std::vector<Hit>> kept;                  // per read: the records that are left
	std::vector<int64_t> reg_off, line_off;
	std::vector<mm2gb_reg_t> rin;
	mm2gb_align_out_t o;
	std::vector<mm2gb_reg_t> treg;                       // the records that get a line, as the text and = / X calls take them
	std::vector<mm2gb_aln_t> taln;
	std::vector<int32_t> tread;
	int64_t *tx_off = nullptr;
	char *tx = nullptr;
	mm2gb_aln_t *eq_aln = nullptr;                       // under MM_F_EQX: where the = / X words of every such record lie in eq_cigar
	uint32_t *eq_cigar = nullptr;
	Aligned() { memset(&o, 0, sizeof o); }
	Aligned(const Aligned&) = delete;
	~Aligned() { mm2gb_align_out_free(&o); free(tx_off); free(tx); free(eq_aln); free(eq_cigar); }       // (freed on every way out)
};

// 6a. the surviving records of every read, as map.c has them when it calls align_regs (map.c:756) ...
void kept_records(Batch &B, Aligned &A)
{
	const size_t R = B.R;
	A.kept.resize(R);
	for_each_on_threads(R, B.nt, 1, [&](size_t r) { chain_hits(B, r, A.kept[r]); });
	A.reg_off.assign(R + 1, 0);
	for (size_t r = 0; r < R; ++r) A.reg_off[r + 1] = A.reg_off[r] + (int64_t)A.kept[r].size();
	A.rin.resize((size_t)std::max<int64_t>(A.reg_off[R], 1));
	for (size_t r = 0; r < R; ++r)
		for (size_t i = 0; i < A.kept[r].size(); ++i) reg_from(A.kept[r][i], A.rin[(size_t)A.reg_off[r] + i]);
}

// ... through the alignment call (on an error the call's own text stays)
int align_kept(Batch &B, Aligned &A)
{
	const MapCall &c = B.c;
	const int idx_flag = mm2gb_index_flag(c.ix);
	if (idx_flag < 0) return -1;
	if (c.sr)
		return B.aln->align_on_device < 0 ? mm2gb_align_regs_sr_host(&B.aln->opt, c.k, idx_flag, c.n_ref, B.aln->ref_seqs, c.ref_lens, c.n_reads, c.seqs, c.lens, A.reg_off.data(), A.rin.data(), B.c_off.data(), B.ca,
		                                                             B.nt, &A.o, B.sro.sr_counts)
		                                  : mm2gb_align_regs_sr_gpu(c.eng, &B.aln->opt, c.k, idx_flag, c.n_ref, B.aln->ref_seqs, c.ref_lens, c.n_reads, c.seqs, c.lens, A.reg_off.data(), A.rin.data(), B.c_off.data(),
		                                                            B.ca, &A.o, B.sro.sr_counts);
	if (c.spl)
		return B.aln->align_on_device < 0 ? mm2gb_align_regs_splice_host(c.spl, c.k, idx_flag, c.n_ref, B.aln->ref_seqs, c.ref_lens, c.n_reads, c.seqs, c.lens, A.reg_off.data(), A.rin.data(), B.c_off.data(),
		                                                                 B.ca, B.nt, &A.o, nullptr)
		                                  : mm2gb_align_regs_splice_gpu(c.eng, c.spl, c.k, idx_flag, c.n_ref, B.aln->ref_seqs, c.ref_lens, c.n_reads, c.seqs, c.lens, A.reg_off.data(), A.rin.data(), B.c_off.data(),
		                                                                B.ca, &A.o, nullptr);
	// q == q2 && e == e2 (minimap2 -O4 -E2): mm_align_pair runs ksw_extz2_sse (align.c:331), the _extz pair
	const bool single = B.aln->opt.q == B.aln->opt.q2 && B.aln->opt.e == B.aln->opt.e2;
	return B.aln->align_on_device < 0 ? (single ? mm2gb_align_regs_extz_host : mm2gb_align_regs_host)(&B.aln->opt, c.k, idx_flag, c.n_ref, B.aln->ref_seqs, c.ref_lens, c.n_reads, c.seqs, c.lens, A.reg_off.data(),
	                                                                                                  A.rin.data(), B.c_off.data(), B.ca, B.nt, &A.o)
	                                  : (single ? mm2gb_align_regs_extz_gpu : mm2gb_align_regs_gpu)(c.eng, &B.aln->opt, c.k, idx_flag, c.n_ref, B.aln->ref_seqs, c.ref_lens, c.n_reads, c.seqs, c.lens, A.reg_off.data(),
	                                                                                                A.rin.data(), B.c_off.data(), B.ca, &A.o);
}

// 6b. per read: primary / secondary, which secondaries stay and the mapping quality, all with the alignment (map.c:347-348, 758)
void rank_aligned(Batch &B, Aligned &A)
{
	const mm2gb_map_opt_t &opt = B.opt;
	for_each_on_threads(B.R, B.nt, 1, [&](size_t r) {
		std::vector<Hit> &hs = A.kept[r];
		hs.clear();
		for (int64_t j = A.o.reg_off[r]; j < A.o.reg_off[r + 1]; ++j) { hs.push_back(hit_from(A.o.regs[j], &A.o.aln[j])); hs.back().aln = j; }
		set_parent(opt.mask_level, opt.mask_len, hs, false, B.aln->opt.a * 2 + B.aln->opt.b);
		select_sub(opt.pri_ratio, B.c.k * 2, opt.best_n, false, (int)(opt.max_gap * 0.8), hs);
		set_mapq(hs, opt.min_chain_score, B.mt[r].rep_len, B.aln->opt.a, B.c.sr != nullptr);
		bool first = true;                                                                            // mm_set_sam_pri (map.c:349)
		for (Hit &h : hs) { h.sam_pri = h.id == h.parent && first; if (h.sam_pri) first = false; }
	});
}

// 6c. the text of the tags for the records that are left, in one call ...
int tag_text(Batch &B, Aligned &A)
{
	const MapCall &c = B.c;
	const mm2gb_map_aln_t *aln = B.aln;
	const size_t R = B.R;
	A.line_off.assign(R + 1, 0);
	for (size_t r = 0; r < R; ++r) A.line_off[r + 1] = A.line_off[r] + (int64_t)A.kept[r].size();
	const int64_t n_out = A.line_off[R];
	// SAM shows the words in its CIGAR column and MM_F_EQX wants other words than the text call reads: cg:Z is then left to the lines (append_cigar)
	const int what = B.out_sam || B.out_eqx ? aln->what & ~MM2GB_TEXT_CG : aln->what;
	std::vector<mm2gb_reg_t> &treg = A.treg;
	std::vector<mm2gb_aln_t> &taln = A.taln;
	std::vector<int32_t> &tread = A.tread;
	treg.resize((size_t)n_out); taln.resize((size_t)n_out); tread.resize((size_t)n_out);
	for (size_t r = 0; r < R; ++r)
		for (size_t i = 0; i < A.kept[r].size(); ++i) {
			const size_t j = (size_t)A.line_off[r] + i;
			treg[j] = A.o.regs[A.kept[r][i].aln]; taln[j] = A.o.aln[A.kept[r][i].aln]; tread[j] = (int32_t)r;
		}
	if (!what || n_out == 0) return 0;
	if (aln->text_on_device <= 0)                         // text_on_device 0: the host form (profiles/aln_text_rate.json)
		return (c.spl ? mm2gb_aln_text_splice_host : mm2gb_aln_text_host)(what, c.n_ref, aln->ref_seqs, c.ref_lens, c.n_reads, c.seqs, c.lens, n_out, treg.data(), tread.data(), taln.data(), A.o.cigar,
		                                                                  B.nt, &A.tx_off, &A.tx);
	std::vector<int64_t> ref_at((size_t)c.n_ref + 1, 0), read_at(R + 1, 0);
	for (int32_t i = 0; i < c.n_ref; ++i) ref_at[(size_t)i + 1] = ref_at[(size_t)i] + c.ref_lens[i];
	for (size_t i = 0; i < R; ++i) read_at[i + 1] = read_at[i] + c.lens[i];
	// the alignment call's device backend says what it left resident (engine.h: al_resident): this batch's residues, or nothing
	Engine &e = c.eng->e;
	if (aln->align_on_device >= 0 && e.al_resident[0] == ref_at.back() && e.al_resident[1] == read_at.back())
		return aln_text_resident(e, c.spl != nullptr, c.spl ? "mm2gb_map_reads_splice" : "mm2gb_map_reads_aln", what, c.n_ref, c.ref_lens, ref_at.data(), c.n_reads, c.lens, read_at.data(), n_out, treg.data(), tread.data(), taln.data(),
		                         A.o.cigar, &A.tx_off, &A.tx);
	return (c.spl ? mm2gb_aln_text_splice_gpu : mm2gb_aln_text_gpu)(c.eng, what, c.n_ref, aln->ref_seqs, c.ref_lens, c.n_reads, c.seqs, c.lens, n_out, treg.data(), tread.data(), taln.data(), A.o.cigar, &A.tx_off, &A.tx);
}

// 6d. under MM_F_EQX: the = / X words of the same records, in one call (mm_update_cigar_eqx, align.c:169-238, as a pass after everything that reads the M words)
int eqx_words(Batch &B, Aligned &A)
{
	const MapCall &c = B.c;
	const int64_t n_out = (int64_t)A.treg.size();
	if (!B.out_eqx || n_out == 0) return 0;
	if (c.out->eqx_on_device <= 0)                         // eqx_on_device 0: the host form (profiles/eqx_rate.json)
		return mm2gb_cigar_eqx_host(c.n_ref, B.aln->ref_seqs, c.ref_lens, c.n_reads, c.seqs, c.lens, n_out, A.treg.data(), A.tread.data(), A.taln.data(), A.o.cigar, B.nt, &A.eq_aln, &A.eq_cigar);
	std::vector<int64_t> ref_at((size_t)c.n_ref + 1, 0), read_at(B.R + 1, 0);
	for (int32_t i = 0; i < c.n_ref; ++i) ref_at[(size_t)i + 1] = ref_at[(size_t)i] + c.ref_lens[i];
	for (size_t i = 0; i < B.R; ++i) read_at[i + 1] = read_at[i] + c.lens[i];
	Engine &e = c.eng->e;                                 // (as tag_text: the batch's residues where the alignment or the text call left them)
	if (B.aln->align_on_device >= 0 && e.al_resident[0] == ref_at.back() && e.al_resident[1] == read_at.back())
		return cigar_eqx_resident(e, "mm2gb_map_reads", c.n_ref, c.ref_lens, ref_at.data(), c.n_reads, c.lens, read_at.data(), n_out, A.treg.data(), A.tread.data(), A.taln.data(), A.o.cigar,
		                          &A.eq_aln, &A.eq_cigar);
	return mm2gb_cigar_eqx_gpu(c.eng, c.n_ref, B.aln->ref_seqs, c.ref_lens, c.n_reads, c.seqs, c.lens, n_out, A.treg.data(), A.tread.data(), A.taln.data(), A.o.cigar, &A.eq_aln, &A.eq_cigar);
}

// ... then the lines
void aligned_lines(Batch &B, const Aligned &A)
{
	const int64_t out_flag = B.c.out ? B.c.out->flag : 0;
	for_each_on_threads(B.R, B.nt, 1, [&](size_t r) {
		const char *qname = B.c.names[r] ? B.c.names[r] : "*";
		if (B.out_sam && A.kept[r].empty() && !(out_flag & MM2GB_F_SAM_HIT_ONLY)) {                   // map.c:1367
			write_sam_unmapped(B.lines[r], qname, B.c.lens[r], B.c.seqs[r], B.mt[r].rep_len);
			B.no_hit[r] = 1;
		}
		for (size_t i = 0; i < A.kept[r].size(); ++i) {
			const Hit &h = A.kept[r][i];
			const size_t j = (size_t)A.line_off[r] + i;
			if (B.c.sr && (B.opt.flag & MM2GB_F_NO_PRINT_2ND) && h.id != h.parent) continue;          // map.c:1359
			const uint32_t *words = h.has_p ? A.o.cigar + A.o.aln[h.aln].cigar_off : nullptr;
			const bool eq = h.has_p && A.eq_aln;
			const uint32_t *shown = eq ? A.eq_cigar + A.eq_aln[j].cigar_off : words;
			const int32_t n_shown = eq ? A.eq_aln[j].n_cigar : h.n_cigar;
			if (B.out_sam) write_sam(B.lines[r], qname, B.c.lens[r], B.c.seqs[r], h, A.kept[r], B.c.ref_names, out_flag, shown, n_shown, words);
			else {
				paf_line(B, r, h, words);
				if (B.out_eqx && h.has_p && (B.aln->what & MM2GB_TEXT_CG)) { B.lines[r] += "\tcg:Z:"; append_cigar(B.lines[r], shown, n_shown); }
			}
			if (A.tx_off) B.lines[r].append(A.tx + A.tx_off[j], (size_t)(A.tx_off[j + 1] - A.tx_off[j]));
			if (B.out_sam) { B.lines[r] += "\trl:i:"; append_int(B.lines[r], B.mt[r].rep_len); }     // format.c:540: after cs:Z / MD:Z in SAM
			B.lines[r] += '\n';
		}
	});
}

// the lines end to end
int emit_paf(Batch &B)
{
	size_t total = 0;
	for (const auto &l : B.lines) total += l.size();
	char *buf = (char*)malloc(total + 1);
	if (!buf) return fail("mm2gb_map_reads: out of memory");
	size_t at = 0;
	for (const auto &l : B.lines) { memcpy(buf + at, l.data(), l.size()); at += l.size(); if (!l.empty() && !B.no_hit[(size_t)(&l - B.lines.data())]) ++B.st.n_mapped; }
	buf[total] = 0;
	*B.c.paf_out = buf; *B.c.paf_len = (int64_t)total;
	B.st.n_reads = B.c.n_reads;
	if (B.c.stats) *B.c.stats = B.st;
	if (B.c.sr_out) { *B.c.sr_out = B.sro; for (int i = 0; i < 3; ++i) B.c.sr_out->s_extra[i] = B.s_extra ? B.s_extra[i] : 0.0; }
	return 0;
}

int map_reads_body(const MapCall &c)
{
	if (!c.opt) return fail("mm2gb_map_reads: null argument");
	mm2gb_map_opt_t opt = *c.opt;
	// (what the options rule out is said before anything else is looked at)
	constexpr int64_t overlap_bits = MM2GB_F_NO_DIAG | MM2GB_F_NO_DUAL | MM2GB_F_ALL_CHAINS;
	if (c.sr) {
		constexpr int64_t sr_bits = MM2GB_F_SR | MM2GB_F_FRAG_MODE | MM2GB_F_NO_PRINT_2ND | MM2GB_F_HEAP_SORT;
		static const struct { int64_t bit; const char *name; } refused[] = { { MM2GB_F_RMQ, "MM_F_RMQ (options.c:173)" }, { MM2GB_F_QSTRAND, "MM_F_QSTRAND" }, { MM2GB_F_EQX, "MM_F_EQX" }, { MM2GB_F_SPLICE, "MM_F_SPLICE" },
		                                                                     { MM2GB_F_NO_DIAG, "MM_F_NO_DIAG" }, { MM2GB_F_NO_DUAL, "MM_F_NO_DUAL" }, { MM2GB_F_ALL_CHAINS, "MM_F_ALL_CHAINS" } };
		for (const auto &x : refused) if (opt.flag & x.bit) return fail(std::string("mm2gb_map_reads_sr: ") + x.name + " is not supported");
		if (!(opt.flag & MM2GB_F_SR)) return fail("mm2gb_map_reads_sr: the options do not carry MM_F_SR (mm2gb_map_opt_init_sr)");
		if (opt.flag & ~(int64_t)(0x100000 | 0x200000 | sr_bits)) return fail("mm2gb_map_reads_sr: of mm_mapopt_t::flag only the preset's MM_F_SR, MM_F_FRAG_MODE, MM_F_NO_PRINT_2ND and MM_F_HEAP_SORT are supported, MM_F_FOR_ONLY and MM_F_REV_ONLY beside them");
		if (c.sr->align == 0 && c.sr->what != 0) return fail("mm2gb_map_reads_sr: what asks for alignment text and align is 0");
		if (c.sr->align != 0 && !c.aln) return fail("mm2gb_map_reads_sr: null argument");
		if (c.frag && c.aln) return fail("mm2gb_map_frags_sr: paired ends with base-level alignment are not supported (-c on mate pairs needs mm_pair and mm_set_pe_thru)");
		if (opt.seeding_on_device > 1) opt.seeding_on_device = 1;          // (the resident path skips nothing that the rescue needs)
		if (c.ix && (mm2gb_index_flag(c.ix) & MM2GB_I_HPC)) return fail("mm2gb_map_reads_sr: a homopolymer-compressed index does not work with MM_F_SR (align.c:583)");
	} else
	if (opt.flag & ~(int64_t)(0x100000 | 0x200000 | MM2GB_F_RMQ | MM2GB_F_NO_LJOIN | overlap_bits))
		return fail("mm2gb_map_reads: of mm_mapopt_t::flag only MM_F_FOR_ONLY and MM_F_REV_ONLY are supported, MM_F_RMQ, MM_F_NO_LJOIN and read overlap's MM_F_NO_DIAG, MM_F_NO_DUAL and MM_F_ALL_CHAINS beside them");
	if ((opt.flag & MM2GB_F_RMQ) && (opt.flag & overlap_bits))         // (read overlap goes through the chaining DP: no fixture has it with mg_lchain_rmq as the first chainer)
		return fail("mm2gb_map_reads: beside MM_F_RMQ only MM_F_FOR_ONLY and MM_F_REV_ONLY are supported, and MM_F_NO_LJOIN: not MM_F_NO_DIAG, MM_F_NO_DUAL or MM_F_ALL_CHAINS");
	if (c.aln && (opt.flag & overlap_bits)) {
		const char *bit = opt.flag & MM2GB_F_ALL_CHAINS ? "MM_F_ALL_CHAINS" : opt.flag & MM2GB_F_NO_DIAG ? "MM_F_NO_DIAG" : "MM_F_NO_DUAL";
		return fail(std::string(c.spl ? "mm2gb_map_reads_splice: " : "mm2gb_map_reads_aln: ") + bit + " is not supported with base-level alignment (read overlap runs without it)");
	}
	if (c.out) {
		const std::string who = c.sr ? "mm2gb_map_reads_sr_out: " : c.spl ? "mm2gb_map_reads_splice_out: " : "mm2gb_map_reads_aln_out: ";
		if (c.out->format != 0 && c.out->format != 1) return fail(who + "format is 0 (PAF) or 1 (SAM)");
		if (c.out->flag & ~(int64_t)(MM2GB_F_EQX | MM2GB_F_SOFTCLIP | MM2GB_F_SAM_HIT_ONLY)) return fail(who + "of mm_mapopt_t::flag the output options take only MM_F_EQX, MM_F_SOFTCLIP and MM_F_SAM_HIT_ONLY");
		if (c.out->format == 1 && !c.aln) return fail(who + "SAM output needs base-level alignment (minimap2 -a implies -c)");
		if ((c.out->flag & MM2GB_F_EQX) && !c.aln) return fail(who + "MM_F_EQX needs base-level alignment (there is no CIGAR to rewrite)");
	}
	if (!c.eng || !c.ix || !c.paf_out || !c.paf_len || c.n_reads < 0 || c.n_ref <= 0 || !c.ref_names || !c.ref_lens || (c.n_reads > 0 && (!c.names || !c.seqs || !c.lens)))
		return fail("mm2gb_map_reads: null argument");
	if (c.spl && (opt.flag & MM2GB_F_RMQ)) return fail("mm2gb_map_reads_splice: MM_F_RMQ does not work with MM_F_SPLICE (options.c:173)");
	if (opt.mid_occ <= 0) opt.mid_occ = mm2gb_index_mid_occ(c.ix, opt.mid_occ_frac, opt.min_mid_occ, opt.max_mid_occ);   // options.c:78-84
	if (opt.bw_long < opt.bw) opt.bw_long = opt.bw;
	if (opt.host_threads <= 0) opt.host_threads = std::min(32, usable_cpus());
	auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
	double t_mark = now();
	auto lap = [&](double &slot) { const double t = now(); slot += t - t_mark; t_mark = t; };
	*c.paf_out = nullptr; *c.paf_len = 0;
	if (c.n_reads == 0) {
		*c.paf_out = (char*)calloc(1, 1);
		if (c.stats) memset(c.stats, 0, sizeof *c.stats);
		return *c.paf_out ? 0 : fail("mm2gb_map_reads: out of memory");
	}
	Batch B(c, opt);
	std::unique_ptr<TraceRange> tr;                       // stage ranges for rocprofv3 --marker-trace / rocprof-sys
	auto stage = [&](const char *name) { tr.reset(); if (name) tr.reset(new TraceRange(name)); };
	const bool dev_seed = opt.seeding_on_device > 0;
	if (opt.flag & (MM2GB_F_NO_DIAG | MM2GB_F_NO_DUAL)) {                                             // (without the bits: no ranks, null pointers as ever)
		B.q_rank = c.q_rank; B.ref_rank = c.ref_rank;
		if (!B.q_rank || !B.ref_rank) {
			name_ranks(c.n_reads, c.names, c.n_ref, c.ref_names, B.own_q_rank, B.own_ref_rank);
			B.q_rank = B.own_q_rank.data(); B.ref_rank = B.own_ref_rank.data();
		}
	}
	const bool ask_resident = opt.seeding_on_device >= MM2GB_SEEDING_RESIDENT;
	const bool want_resident = ask_resident && !c.aln && !(opt.flag & MM2GB_F_RMQ) && ((opt.flag & MM2GB_F_NO_LJOIN) || opt.bw_long <= opt.bw);
	B.resident = want_resident;                           // (seed_on_device takes it back for a batch beyond one chaining micro-batch, or one without a hit)
	const bool verbose = getenv("MM2GB_DEBUG_PHASES") != nullptr;

	stage("mm2gb:map_seed");
	if (dev_seed ? seed_on_device(B) : seed_on_host(B)) return -1;                                    // 1
	lap(B.st.s_seed);
	stage("mm2gb:map_anchors");
	if (c.sr) {
		if (anchors_and_chains_sr(B, dev_seed)) return -1;                                            // 2 and 3 with the rescue (one lap: the rescue runs both again)
		lap(B.st.s_chain);
		stage("mm2gb:map_hit_records");
		if (hit_records(B)) return -1;                                                                // 5
		lap(B.st.s_regs);
		stage("mm2gb:map_hits_to_paf");
		if (!B.aln) { if (c.frag) finish_frags_sr(B); else finish_reads_sr(B); }                      // 6
		else {
			Aligned A;
			kept_records(B, A);
			lap(B.st.s_post);
			if (align_kept(B, A)) return -1;
			lap(B.s_extra[0]);
			rank_aligned(B, A);
			lap(B.s_extra[1]);
			if (tag_text(B, A) || eqx_words(B, A)) return -1;
			lap(B.s_extra[2]);
			aligned_lines(B, A);
		}
		B.release_matches();
		lap(B.st.s_post);
		stage(nullptr);
		return emit_paf(B);
	}
	if (collect_anchors(B, dev_seed)) return -1;                                                      // 2
	B.st.n_anchors = B.a_off[B.R];
	lap(B.st.s_anchors);
	if (B.resident) {
		stage("mm2gb:map_chain");
		if (chain_resident(B)) return -1;                                                             // 3 (no stage 4: that is what lets the chains stay)
		lap(B.st.s_chain);
		stage("mm2gb:map_hit_records");
		if (hit_records_resident(B)) return -1;                                                       // 5, and the divergence walk of 6
		lap(B.st.s_regs);
	} else {
		stage("mm2gb:map_chain");
		if (chain(B) || ((opt.flag & MM2GB_F_RMQ) && first_chain(B))) return -1;                      // 3
		lap(B.st.s_chain);
		stage("mm2gb:map_rechain");
		if (c.spl) B.st.n_chains = B.u_off[B.R];                                                      // 4 (map.c:698: not under MM_F_SPLICE)
		else if (rechain(B)) return -1;
		lap(B.st.s_rechain);
		stage("mm2gb:map_hit_records");
		if (hit_records(B)) return -1;                                                                // 5
		lap(B.st.s_regs);
		if (verbose && dev_seed && !(opt.flag & MM2GB_F_RMQ)) {       // what the staged stages copied, from their arrays' sizes (re-chaining on the device not counted)
			const int64_t R8 = (int64_t)(B.R + 1) * 8, n = B.st.n_anchors, n_u = B.u_off[B.R], n_c = B.c_off[B.R];
			B.link[1] += R8 + n * 16;                                                                 // 2: offsets and anchors down
			B.link[0] += R8 + n * 16;                                                                 // 3: and up again
			B.link[1] += n >= 200000000 ? 2 * R8 + n_u * 8 + n_c * 16 : n * 8;                        //    chains down (mm2gb_chain_gpu), or scores and predecessors (mm2gb_chain_host)
			B.link[0] += 2 * R8 + n_u * 8 + n_c * 16 + (int64_t)B.R * 8;                              // 5: chains up
			B.link[1] += n_u * (int64_t)sizeof(mm2gb_reg_t);                                          //    hit records down
		}
	}
	if (verbose && dev_seed)
		fprintf(stderr, "[mm2gb] map path: %s%s; %lld anchors, %lld chains; copied to the device %lld B, back %lld B\n", B.resident ? "resident" : "staged",
		        ask_resident && !B.resident ? (want_resident ? " (resident asked for: the batch's anchors exceed one chaining micro-batch, or it has none)" : " (resident asked for: the options do not allow it)") : "",
		        (long long)B.st.n_anchors, (long long)B.st.n_chains, (long long)B.link[0], (long long)B.link[1]);
	stage("mm2gb:map_hits_to_paf");
	if (!B.aln) finish_reads(B);                                                                      // 6
	else {
		Aligned A;
		kept_records(B, A);                                                                           // 6a
		lap(B.st.s_post);
		if (align_kept(B, A)) return -1;
		lap(B.s_extra[0]);
		rank_aligned(B, A);                                                                           // 6b
		lap(B.s_extra[1]);
		if (tag_text(B, A) || eqx_words(B, A)) return -1;                                             // 6c, 6d
		lap(B.s_extra[2]);
		aligned_lines(B, A);
	}
	B.release_matches();
	lap(B.st.s_post);
	stage(nullptr);
	return emit_paf(B);
}

// a batch's arrays are gigabytes: running out of host memory on this thread is an error of the call, not the end of the process
int map_reads_try(const MapCall &c)
{
	try { return map_reads_body(c); }
	catch (const std::bad_alloc&) { return fail("mm2gb_map_reads: out of host memory"); }
}

// nullptr, or why a mm2gb_map_aln_t cannot be used
const char *bad_aln(const mm2gb_map_aln_t *aln)
{
	if (!aln || !aln->ref_seqs) return "null argument";
	if (aln->what & ~(MM2GB_TEXT_CG | MM2GB_TEXT_CS | MM2GB_TEXT_CS_LONG | MM2GB_TEXT_MD)) return "what has a bit outside MM2GB_TEXT_*";
	return nullptr;
}

// the parts' PAF end to end (the parts are freed) and their stats as one: counts summed, stage seconds summed or the largest taken
int join_parts(const std::string &who, std::vector<char*> &part, const std::vector<int64_t> &part_len, const std::vector<mm2gb_map_stats_t> &st, bool sum_seconds,
               char **paf_out, int64_t *paf_len, mm2gb_map_stats_t *stats)
{
	int64_t all = 0;
	for (int64_t l : part_len) all += l;
	char *buf = (char*)malloc((size_t)all + 1);
	int64_t at = 0;
	mm2gb_map_stats_t sum; memset(&sum, 0, sizeof sum);
	static double mm2gb_map_stats_t::*const seconds[] = { &mm2gb_map_stats_t::s_seed, &mm2gb_map_stats_t::s_anchors, &mm2gb_map_stats_t::s_chain, &mm2gb_map_stats_t::s_rechain, &mm2gb_map_stats_t::s_regs, &mm2gb_map_stats_t::s_post };
	for (size_t i = 0; i < part.size(); ++i) {
		if (buf && part_len[i]) memcpy(buf + at, part[i], (size_t)part_len[i]);
		at += part_len[i]; free(part[i]); part[i] = nullptr;
		const mm2gb_map_stats_t &q = st[i];
		sum.n_reads += q.n_reads; sum.n_mapped += q.n_mapped; sum.n_anchors += q.n_anchors; sum.n_chains += q.n_chains; sum.n_rechained += q.n_rechained; sum.n_rmq_tied += q.n_rmq_tied;
		for (auto s : seconds) sum.*s = sum_seconds ? sum.*s + q.*s : std::max(sum.*s, q.*s);
	}
	if (!buf) return fail(who + ": out of memory");
	buf[all] = 0;
	*paf_out = buf; *paf_len = all;
	if (stats) *stats = sum;
	return 0;
}

// A run of any size as a stream of batches (role of the batch rotation of worker_for, map.c:924-1153: seed batch k+1 while batch k is
// chained and batch k-1 is finished): the reads are cut into consecutive chunks of about chunk_bases bases, and every engine -- several
// per device are the point: each has its own streams and arenas -- has a host thread that takes the next chunk and maps it from
// seeding to PAF.  A chunk's stages alternate between host threads and the device, so with two or three engines on a GPU one chunk is
// being seeded or post-processed while another one's kernels run; with engines on several GPUs the reads shard (no
// exchange).  The host threads of opt are shared out with over-subscription (2.5 x), because a chunk's threads idle while its kernels run.
// PAF in read order; stats: counts summed, s_* = seconds of each stage SUMMED over chunks (they overlap: not wall time).
int stream_body(mm2gb_engine_t *const *engines, int n_engines, int64_t chunk_bases, const MapCall &c)
{
	const int32_t n_reads = c.n_reads;
	if (!engines || n_engines < 1 || !c.ix || !c.opt || !c.paf_out || !c.paf_len || n_reads < 0 || (n_reads > 0 && (!c.lens || !c.names || !c.seqs)) || (c.n_ref > 0 && (!c.ref_names || !c.ref_lens)))
		return fail("mm2gb_map_reads_stream: null argument");
	for (int e = 0; e < n_engines; ++e) if (!engines[e]) return fail("mm2gb_map_reads_stream: null engine");
	*c.paf_out = nullptr; *c.paf_len = 0;
	if (chunk_bases <= 0) chunk_bases = 96 * 1000 * 1000;
	std::vector<int32_t> cut(1, 0);
	{ int64_t acc = 0; for (int32_t r = 0; r < n_reads; ++r) { acc += c.lens[r]; if (acc >= chunk_bases && r + 1 < n_reads) { cut.push_back(r + 1); acc = 0; } } }
	cut.push_back(n_reads);
	const size_t n_chunks = cut.size() - 1;
	mm2gb_map_opt_t opt = *c.opt;
	const int all_threads = opt.host_threads > 0 ? opt.host_threads : std::min(32, usable_cpus());
	const int workers = (int)std::min<size_t>((size_t)n_engines, std::max<size_t>(1, n_chunks));
	// host threads of all workers together, in % of opt's (MM2GB_STREAM_THREADS_PCT): a chunk's threads idle while its kernels run, and the reads its
	// re-chaining gives to host threads want a core each when they come.  1.05 Gbp, four engines, 16 threads: 100 % 8.0 s, 150 % 6.8-7.1, 250 % 6.3-6.5, 400 % 6.6-6.9
	int oversub_pct = 250;
	if (const char *v = getenv("MM2GB_STREAM_THREADS_PCT")) oversub_pct = std::max(25, atoi(v));
	opt.host_threads = std::max(1, workers == 1 ? all_threads : (all_threads * oversub_pct / 100 + workers - 1) / workers);
	if (opt.mid_occ <= 0) opt.mid_occ = mm2gb_index_mid_occ(c.ix, opt.mid_occ_frac, opt.min_mid_occ, opt.max_mid_occ);     // once, not per chunk
	std::vector<int32_t> q_rank, ref_rank;                // the names' ranks too
	if ((opt.flag & (MM2GB_F_NO_DIAG | MM2GB_F_NO_DUAL)) && n_reads > 0 && c.n_ref > 0) name_ranks(n_reads, c.names, c.n_ref, c.ref_names, q_rank, ref_rank);
	std::vector<char*> part(n_chunks, nullptr);
	std::vector<int64_t> part_len(n_chunks, 0);
	std::vector<mm2gb_map_stats_t> st(n_chunks);
	std::vector<double> extra(n_chunks * 3, 0.0);         // with an alignment: seconds for align, the steps after it, text, per chunk
	std::vector<mm2gb_map_sr_out_t> sro(c.sr_out ? n_chunks : 0);
	std::atomic<size_t> next(0);
	std::atomic<int> failed(0);
	std::string why;                                      // error text is per thread: carry the first one over
	std::mutex why_lock;
	run_on_threads(workers, [&](int e) {                  // a worker keeps its engine from chunk to chunk
		for (;;) {
			const size_t k = next.fetch_add(1);
			if (k >= n_chunks || failed.load()) break;
			memset(&st[k], 0, sizeof(st[k]));
			MapCall one = c;
			one.eng = engines[e]; one.opt = &opt; one.n_reads = cut[k + 1] - cut[k]; one.names += cut[k]; one.seqs += cut[k]; one.lens += cut[k];
			if (c.frag) one.frag_off += cut[k];                // (a chunk is whole units: fragments are never split)
			one.paf_out = &part[k]; one.paf_len = &part_len[k]; one.stats = &st[k]; one.s_extra = &extra[k * 3];
			if (c.sr_out) { memset(&sro[k], 0, sizeof sro[k]); one.sr_out = &sro[k]; }
			if (!q_rank.empty()) { one.q_rank = q_rank.data() + cut[k]; one.ref_rank = ref_rank.data(); }
			if (map_reads_try(one)) {
				std::lock_guard<std::mutex> g(why_lock);
				if (!failed.exchange(1)) why = "chunk " + std::to_string(k) + " on engine " + std::to_string(e) + ": " + mm2gb_last_error();
			}
		}
	});
	if (failed.load()) { for (char *p : part) free(p); return fail("mm2gb_map_reads_stream: " + why); }
	if (join_parts("mm2gb_map_reads_stream", part, part_len, st, true, c.paf_out, c.paf_len, c.stats)) return -1;
	if (c.s_extra) for (size_t i = 0; i < extra.size(); ++i) c.s_extra[i % 3] += extra[i];
	if (c.sr_out) {
		memset(c.sr_out, 0, sizeof *c.sr_out);
		for (const mm2gb_map_sr_out_t &q : sro) {
			c.sr_out->n_chain_calls += q.n_chain_calls; c.sr_out->n_rescued += q.n_rescued; c.sr_out->n_tied_reads += q.n_tied_reads;
			for (int i = 0; i < MM2GB_SR_N_COUNTS; ++i) c.sr_out->sr_counts[i] += q.sr_counts[i];
			for (int i = 0; i < 3; ++i) c.sr_out->s_extra[i] += q.s_extra[i];
		}
	}
	return 0;
}

} // namespace
} // namespace mm2gb

using namespace mm2gb;

namespace mm2gb {
HostScratch &host_scratch(mm2gb_engine_t *eng)
{
	if (!eng->host_scratch) {
		eng->host_scratch = new HostScratch;
		eng->host_scratch_free = [](void *p) { delete static_cast<HostScratch*>(p); };
	}
	return *static_cast<HostScratch*>(eng->host_scratch);
}
}

extern "C" {

void mm2gb_map_opt_init(mm2gb_map_opt_t *o)       // mm_mapopt_init (options.c:15-75), the fields this path looks at
{
	memset(o, 0, sizeof(*o));
	o->seed = 11; o->mid_occ_frac = 2e-4f; o->min_mid_occ = 10; o->max_mid_occ = 1000000; o->q_occ_frac = 0.01f;
	o->min_cnt = 3; o->min_chain_score = 40; o->bw = 500; o->bw_long = 20000; o->max_gap = 5000; o->max_gap_ref = -1;
	o->max_chain_iter = 5000; o->rmq_inner_dist = 1000; o->rmq_size_cap = 100000; o->rmq_rescue_size = 1000; o->rmq_rescue_ratio = 0.1f;
	o->chain_gap_scale = 0.8f; o->chain_skip_scale = 0.0f; o->max_max_occ = 4095; o->occ_dist = 500;
	o->mask_level = 0.5f; o->mask_len = INT32_MAX; o->pri_ratio = 0.8f; o->best_n = 5;
	o->host_threads = 0;           // 0: as many as the process may use, at most 32
	o->max_chain_skip = INT32_MAX; // (mm_mapopt_init: 25) the GPU path's contract is max-chain-skip = infinity; a finite value is kept on request
}

int mm2gb_map_opt_init_preset(mm2gb_map_opt_t *o, const char *preset)       // options.c:95-131: the mapping fields of the table's row (align_host.cpp)
{
	if (!o || !preset) return fail("mm2gb_map_opt_init_preset: null argument");
	const PresetRow *p = preset_row(preset);
	if (!p) return fail(std::string("mm2gb_map_opt_init_preset: preset ") + preset + " is not supported (" + preset_names + ")");
	mm2gb_map_opt_init(o);
	o->bw = p->bw; o->bw_long = p->bw_long; o->max_gap = p->max_gap; o->flag |= p->map_flag;
	o->min_mid_occ = p->min_mid_occ; o->max_mid_occ = p->max_mid_occ; o->best_n = p->best_n;
	return 0;
}

int mm2gb_map_opt_init_ava(mm2gb_map_opt_t *o, const char *preset)          // options.c:96-109
{
	if (!o || !preset) return fail("mm2gb_map_opt_init_ava: null argument");
	const bool ont = !strcmp(preset, "ava-ont"), pb = !strcmp(preset, "ava-pb");
	if (!ont && !pb) return fail(std::string("mm2gb_map_opt_init_ava: preset ") + preset + " is not supported (ava-ont, ava-pb)");
	mm2gb_map_opt_init(o);
	o->flag |= MM2GB_F_ALL_CHAINS | MM2GB_F_NO_DIAG | MM2GB_F_NO_DUAL | MM2GB_F_NO_LJOIN;
	o->min_chain_score = 100; o->pri_ratio = 0.0f; o->occ_dist = 0;
	if (ont) o->bw = o->bw_long = 2000;
	else o->bw_long = o->bw;
	return 0;
}

void mm2gb_map_opt_init_sr(mm2gb_map_opt_t *o)    // options.c:133-150: the mapping fields this record has room for
{
	mm2gb_map_opt_init(o);
	o->flag |= MM2GB_F_SR | MM2GB_F_FRAG_MODE | MM2GB_F_NO_PRINT_2ND | MM2GB_F_HEAP_SORT;
	o->max_gap = 100; o->bw = o->bw_long = 100; o->pri_ratio = 0.5f; o->min_cnt = 2; o->min_chain_score = 25; o->best_n = 20; o->mid_occ = 1000;
}

void mm2gb_map_sr_init(mm2gb_map_sr_t *s)          // options.c:133-150: what the mapping options have no room for, and the alignment's values
{
	memset(s, 0, sizeof(*s));
	mm2gb_align_sr_opt_init(&s->opt);
	s->max_occ = 5000; s->max_frag_len = 800;
}

namespace {
// the call's arguments checked and, with an alignment, the mm2gb_map_aln_t the shared stages read; nullptr, or why not
const char *sr_as_aln(const mm2gb_map_sr_t *sr, mm2gb_map_aln_t &a, bool &aligned)
{
	if (!sr) return "null argument";
	aligned = sr->align != 0;
	if (!aligned) return nullptr;
	a.ref_seqs = sr->ref_seqs; a.opt = sr->opt; a.what = sr->what; a.align_on_device = sr->align_on_device; a.text_on_device = sr->text_on_device;
	return bad_aln(&a);
}
}

int mm2gb_map_reads_sr(mm2gb_engine_t *eng, const mm2gb_index_t *ix, int k, const char *const *ref_names, const int32_t *ref_lens, int32_t n_ref, const mm2gb_map_opt_t *opt,
                       const mm2gb_map_sr_t *sr, int32_t n_reads, const char *const *names, const char *const *seqs, const int32_t *lens, char **paf_out, int64_t *paf_len,
                       mm2gb_map_stats_t *stats, mm2gb_map_sr_out_t *sr_out)
{
	return mm2gb_map_reads_sr_out(eng, ix, k, ref_names, ref_lens, n_ref, opt, sr, n_reads, names, seqs, lens, paf_out, paf_len, stats, sr_out, nullptr);
}

int mm2gb_map_reads_sr_out(mm2gb_engine_t *eng, const mm2gb_index_t *ix, int k, const char *const *ref_names, const int32_t *ref_lens, int32_t n_ref, const mm2gb_map_opt_t *opt,
                           const mm2gb_map_sr_t *sr, int32_t n_reads, const char *const *names, const char *const *seqs, const int32_t *lens, char **paf_out, int64_t *paf_len,
                           mm2gb_map_stats_t *stats, mm2gb_map_sr_out_t *sr_out, const mm2gb_map_out_t *out)
{
	// (what the output options rule out is said before anything else is looked at, the engine included)
	if (out && sr && !sr->align && (out->format == 1 || (out->flag & MM2GB_F_EQX)))
		return fail(std::string("mm2gb_map_reads_sr_out: ") + (out->format == 1 ? "SAM output needs base-level alignment (minimap2 -a implies -c)" : "MM_F_EQX needs base-level alignment (there is no CIGAR to rewrite)"));
	if (!eng) return fail("mm2gb: null engine");
	mm2gb_map_aln_t aln;
	bool aligned = false;
	if (const char *why = sr_as_aln(sr, aln, aligned)) return fail(std::string("mm2gb_map_reads_sr: ") + why);
	double extra[3] = { 0, 0, 0 };
	if (sr_out) memset(sr_out, 0, sizeof *sr_out);
	MapCall c = { eng, ix, k, ref_names, ref_lens, n_ref, opt, n_reads, names, seqs, lens, paf_out, paf_len, stats, aligned ? &aln : nullptr, extra };
	c.sr = sr; c.sr_out = sr_out; c.out = out;
	return map_reads_try(c);
}

int mm2gb_map_reads_stream_sr(mm2gb_engine_t *const *engines, int n_engines, const mm2gb_index_t *ix, int k, const char *const *ref_names, const int32_t *ref_lens,
                              int32_t n_ref, const mm2gb_map_opt_t *opt, const mm2gb_map_sr_t *sr, int32_t n_reads, const char *const *names, const char *const *seqs,
                              const int32_t *lens, int64_t chunk_bases, char **paf_out, int64_t *paf_len, mm2gb_map_stats_t *stats, mm2gb_map_sr_out_t *sr_out)
{
	return mm2gb_map_reads_stream_sr_out(engines, n_engines, ix, k, ref_names, ref_lens, n_ref, opt, sr, n_reads, names, seqs, lens, chunk_bases, paf_out, paf_len, stats, sr_out, nullptr);
}

int mm2gb_map_reads_stream_sr_out(mm2gb_engine_t *const *engines, int n_engines, const mm2gb_index_t *ix, int k, const char *const *ref_names, const int32_t *ref_lens,
                                  int32_t n_ref, const mm2gb_map_opt_t *opt, const mm2gb_map_sr_t *sr, int32_t n_reads, const char *const *names, const char *const *seqs,
                                  const int32_t *lens, int64_t chunk_bases, char **paf_out, int64_t *paf_len, mm2gb_map_stats_t *stats, mm2gb_map_sr_out_t *sr_out,
                                  const mm2gb_map_out_t *out)
{
	mm2gb_map_aln_t aln;
	bool aligned = false;
	if (const char *why = sr_as_aln(sr, aln, aligned)) return fail(std::string("mm2gb_map_reads_stream_sr: ") + why);
	double extra[3] = { 0, 0, 0 };
	mm2gb_map_sr_out_t own;
	if (sr_out) memset(sr_out, 0, sizeof *sr_out);
	MapCall c = { nullptr, ix, k, ref_names, ref_lens, n_ref, opt, n_reads, names, seqs, lens, paf_out, paf_len, stats, aligned ? &aln : nullptr, extra };
	c.sr = sr; c.sr_out = sr_out ? sr_out : &own; c.out = out;
	return stream_body(engines, n_engines, chunk_bases, c);
}

// ---- fragments (paired ends) ----

int mm2gb_frag_offsets(int32_t n_reads, const char *const *names, int32_t *frag_off, int32_t *n_frag)
{
	if (n_reads < 0 || !frag_off || !n_frag || (n_reads > 0 && !names)) return fail("mm2gb_frag_offsets: null argument");
	auto name_len = [](const char *s) { const size_t l = strlen(s); return l >= 3 && s[l - 1] >= '0' && s[l - 1] <= '9' && s[l - 2] == '/' ? l - 2 : l; };   // bseq.h:31-36
	int32_t n = 0;
	frag_off[0] = 0;
	for (int32_t i = 1; i <= n_reads; ++i) {               // map.c:1299-1304
		bool same = false;
		if (i < n_reads && names[i - 1] && names[i]) { const size_t l1 = name_len(names[i - 1]), l2 = name_len(names[i]); same = l1 == l2 && strncmp(names[i - 1], names[i], l1) == 0; }
		if (!same) frag_off[++n] = i;
	}
	*n_frag = n;
	return 0;
}

namespace {
// what the two fragment calls share: the arguments checked, the mates that pe_ori turns reverse-complemented (own), the units' names and summed lengths (u_*), and the call
// record on units.  A batch in which no fragment has two reads is the plain call's (frag stays null).
struct FragUnits {
	std::vector<std::string> own;
	std::vector<const char*> seqs, u_names, u_seqs;
	std::vector<int32_t> u_lens;
	FragReads reads;
};
int frag_units(const char *who, MapCall &c, int32_t n_frag, const int32_t *frag_off, int32_t pe_ori, FragUnits &F)
{
	const std::string w(who);
	if (pe_ori < 0 || pe_ori > 3) return fail(w + ": pe_ori is 0..3 (mm_mapopt_t::pe_ori; -x sr: 1)");
	if (c.out && (c.out->format != 0 || (c.out->flag & MM2GB_F_EQX))) return fail(w + ": SAM output and MM_F_EQX are not supported for fragments (the pair fields of mm_write_sam3 and -c on mate pairs are not built)");
	if (c.n_reads < 0 || n_frag < 0 || !frag_off || frag_off[0] != 0 || frag_off[n_frag] != c.n_reads || (c.n_reads > 0 && (!c.names || !c.seqs || !c.lens))) return fail(w + ": null argument, or frag_off does not run from 0 to n_reads");
	bool any_pair = false;
	for (int32_t f = 0; f < n_frag; ++f) {
		const int32_t n = frag_off[f + 1] - frag_off[f];
		if (n < 1) return fail(w + ": a fragment without a read");
		if (n > 2) return fail(w + ": a fragment of more than two reads is not supported (MM_MAX_SEG > 2 is not taken): " + std::string(c.names[frag_off[f]] ? c.names[frag_off[f]] : "*"));
		any_pair |= n == 2;
	}
	c.out = nullptr;                                       // (PAF, no = / X: nothing of it is left to look at)
	if (!any_pair) return 0;
	if (c.sr && c.sr->align != 0) return fail(w + ": paired ends with base-level alignment are not supported (-c on mate pairs needs mm_pair and mm_set_pe_thru)");
	F.seqs.assign(c.seqs, c.seqs + c.n_reads);
	F.own.resize((size_t)c.n_reads);
	F.u_names.resize((size_t)n_frag); F.u_seqs.resize((size_t)n_frag); F.u_lens.resize((size_t)n_frag);
	for (int32_t f = 0; f < n_frag; ++f) {
		const int32_t r0 = frag_off[f], n = frag_off[f + 1] - r0;
		int64_t sum = 0;
		for (int32_t j = 0; j < n; ++j) {
			const int32_t r = r0 + j;
			if (c.lens[r] < 0 || (c.lens[r] > 0 && !c.seqs[r])) return fail(w + ": null argument");
			sum += c.lens[r];
			if (n == 2 && ((j == 0 && (pe_ori >> 1 & 1)) || (j == 1 && (pe_ori & 1)))) {                    // map.c:1169-1171
				append_seq(F.own[(size_t)r], c.seqs[r], c.lens[r], true);
				F.seqs[(size_t)r] = F.own[(size_t)r].c_str();
			}
		}
		if (sum >= INT32_MAX) return fail(w + ": a fragment of 2^31 bases or more");
		F.u_names[(size_t)f] = c.names[r0]; F.u_seqs[(size_t)f] = F.seqs[(size_t)r0]; F.u_lens[(size_t)f] = (int32_t)sum;
	}
	F.reads = { c.names, F.seqs.data(), c.lens, pe_ori };
	c.frag = &F.reads; c.frag_off = frag_off;
	c.n_reads = n_frag; c.names = F.u_names.data(); c.seqs = F.u_seqs.data(); c.lens = F.u_lens.data();
	return 0;
}
}

int mm2gb_map_frags_sr(mm2gb_engine_t *eng, const mm2gb_index_t *ix, int k, const char *const *ref_names, const int32_t *ref_lens, int32_t n_ref, const mm2gb_map_opt_t *opt,
                       const mm2gb_map_sr_t *sr, int32_t n_reads, const char *const *names, const char *const *seqs, const int32_t *lens, char **paf_out, int64_t *paf_len,
                       mm2gb_map_stats_t *stats, mm2gb_map_sr_out_t *sr_out, int32_t n_frag, const int32_t *frag_off, int32_t pe_ori, const mm2gb_map_out_t *out)
{
	if (!eng) return fail("mm2gb: null engine");
	mm2gb_map_aln_t aln;
	bool aligned = false;
	if (const char *why = sr_as_aln(sr, aln, aligned)) return fail(std::string("mm2gb_map_frags_sr: ") + why);
	double extra[3] = { 0, 0, 0 };
	if (sr_out) memset(sr_out, 0, sizeof *sr_out);
	MapCall c = { eng, ix, k, ref_names, ref_lens, n_ref, opt, n_reads, names, seqs, lens, paf_out, paf_len, stats, aligned ? &aln : nullptr, extra };
	c.sr = sr; c.sr_out = sr_out; c.out = out;
	FragUnits F;
	if (frag_units("mm2gb_map_frags_sr", c, n_frag, frag_off, pe_ori, F)) return -1;
	return map_reads_try(c);
}

int mm2gb_map_frags_stream_sr(mm2gb_engine_t *const *engines, int n_engines, const mm2gb_index_t *ix, int k, const char *const *ref_names, const int32_t *ref_lens,
                              int32_t n_ref, const mm2gb_map_opt_t *opt, const mm2gb_map_sr_t *sr, int32_t n_reads, const char *const *names, const char *const *seqs,
                              const int32_t *lens, int64_t chunk_bases, char **paf_out, int64_t *paf_len, mm2gb_map_stats_t *stats, mm2gb_map_sr_out_t *sr_out,
                              int32_t n_frag, const int32_t *frag_off, int32_t pe_ori, const mm2gb_map_out_t *out)
{
	mm2gb_map_aln_t aln;
	bool aligned = false;
	if (const char *why = sr_as_aln(sr, aln, aligned)) return fail(std::string("mm2gb_map_frags_stream_sr: ") + why);
	double extra[3] = { 0, 0, 0 };
	mm2gb_map_sr_out_t own;
	if (sr_out) memset(sr_out, 0, sizeof *sr_out);
	MapCall c = { nullptr, ix, k, ref_names, ref_lens, n_ref, opt, n_reads, names, seqs, lens, paf_out, paf_len, stats, aligned ? &aln : nullptr, extra };
	c.sr = sr; c.sr_out = sr_out ? sr_out : &own; c.out = out;
	FragUnits F;
	if (frag_units("mm2gb_map_frags_stream_sr", c, n_frag, frag_off, pe_ori, F)) return -1;
	return stream_body(engines, n_engines, chunk_bases, c);
}

// mm_select_sub_multi / mm_seg_gen by themselves, batched over fragments (the mapper's stage 6 calls the same two functions per fragment)
int mm2gb_select_sub_multi_host(float pri_ratio, float pri1, float pri2, int32_t min_diff, int32_t best_n, int64_t n_frag, const int32_t *n_segs, const int32_t *qlens,
                                const int32_t *max_gap_ref, const int64_t *reg_off, mm2gb_reg_t *regs, int32_t *n_kept)
{
	if (n_frag < 0 || (n_frag > 0 && (!n_segs || !qlens || !max_gap_ref || !reg_off || !n_kept)) || (n_frag > 0 && reg_off[n_frag] > reg_off[0] && !regs)) return fail("mm2gb_select_sub_multi_host: null argument");
	for (int64_t f = 0; f < n_frag; ++f) {
		if (n_segs[f] < 1 || n_segs[f] > 2) return fail("mm2gb_select_sub_multi_host: a fragment has one or two segments (MM_MAX_SEG > 2 is not taken)");
		const int64_t n = reg_off[f + 1] - reg_off[f];
		if (n < 0) return fail("mm2gb_select_sub_multi_host: reg_off must not decrease");
		for (int64_t i = 0; i < n; ++i) { const int p = regs[reg_off[f] + i].parent; if (p < 0 || p > i) return fail("mm2gb_select_sub_multi_host: a record's parent is itself or an earlier record of its fragment (mm_set_parent)"); }
	}
	for (int64_t f = 0; f < n_frag; ++f) {
		std::vector<Hit> hs;
		for (int64_t j = reg_off[f]; j < reg_off[f + 1]; ++j) hs.push_back(hit_from(regs[j]));
		select_sub_multi(pri_ratio, pri1, pri2, max_gap_ref[f], min_diff, best_n, n_segs[f], qlens + 2 * f, hs);
		for (size_t i = 0; i < hs.size(); ++i) reg_from(hs[i], regs[reg_off[f] + (int64_t)i]);
		n_kept[f] = (int32_t)hs.size();
	}
	return 0;
}

void mm2gb_seg_out_free(mm2gb_seg_out_t *o)
{
	if (!o) return;
	free(o->reg_off); free(o->regs); free(o->anchor_off); free(o->anchors);
	memset(o, 0, sizeof *o);
}

int mm2gb_seg_gen_host(int64_t n_frag, const int32_t *n_segs, const int32_t *qlens, const uint32_t *hash, const int64_t *reg_off, const mm2gb_reg_t *regs,
                       const int64_t *anchor_off, const mm2gb_anchor_t *anchors, mm2gb_seg_out_t *out)
{
	if (!out) return fail("mm2gb_seg_gen_host: null argument");
	memset(out, 0, sizeof *out);
	if (n_frag < 0 || (n_frag > 0 && (!n_segs || !qlens || !hash || !reg_off || !anchor_off))) return fail("mm2gb_seg_gen_host: null argument");
	for (int64_t f = 0; f < n_frag; ++f) {
		if (n_segs[f] < 1 || n_segs[f] > 2) return fail("mm2gb_seg_gen_host: a fragment has one or two segments (MM_MAX_SEG > 2 is not taken)");
		const int64_t n_a = anchor_off[f + 1] - anchor_off[f];
		if (reg_off[f + 1] < reg_off[f] || n_a < 0 || ((reg_off[f + 1] > reg_off[f]) && (!regs || !anchors))) return fail("mm2gb_seg_gen_host: offsets must not decrease, and records need anchors");
		for (int64_t j = reg_off[f]; j < reg_off[f + 1]; ++j) {
			if (regs[j].cnt < 1 || regs[j].as < 0 || (int64_t)regs[j].as + regs[j].cnt > n_a) return fail("mm2gb_seg_gen_host: a record's anchors lie outside its fragment's");
			for (int32_t t = 0; t < regs[j].cnt; ++t) if ((int)(anchors[anchor_off[f] + regs[j].as + t].y >> 48 & 0xff) >= n_segs[f]) return fail("mm2gb_seg_gen_host: an anchor's segment id is not below n_segs");
		}
	}
	std::vector<std::vector<Hit>> r((size_t)n_frag * 2);
	std::vector<std::vector<mm2gb_anchor_t>> a((size_t)n_frag * 2);
	for (int64_t f = 0; f < n_frag; ++f) {
		std::vector<Hit> hs;
		for (int64_t j = reg_off[f]; j < reg_off[f + 1]; ++j) hs.push_back(hit_from(regs[j]));
		seg_gen(hash[f], n_segs[f], qlens + 2 * f, hs, anchors + anchor_off[f], &r[(size_t)f * 2], &a[(size_t)f * 2]);
	}
	const size_t U = (size_t)n_frag * 2;
	out->reg_off = (int64_t*)calloc(U + 1, 8); out->anchor_off = (int64_t*)calloc(U + 1, 8);
	if (!out->reg_off || !out->anchor_off) { mm2gb_seg_out_free(out); return fail("mm2gb_seg_gen_host: out of memory"); }
	for (size_t q = 0; q < U; ++q) { out->reg_off[q + 1] = out->reg_off[q] + (int64_t)r[q].size(); out->anchor_off[q + 1] = out->anchor_off[q] + (int64_t)a[q].size(); }
	out->regs = (mm2gb_reg_t*)calloc((size_t)out->reg_off[U] + 1, sizeof(mm2gb_reg_t)); out->anchors = (mm2gb_anchor_t*)calloc((size_t)out->anchor_off[U] + 1, sizeof(mm2gb_anchor_t));
	if (!out->regs || !out->anchors) { mm2gb_seg_out_free(out); return fail("mm2gb_seg_gen_host: out of memory"); }
	for (size_t q = 0; q < U; ++q) {
		for (size_t i = 0; i < r[q].size(); ++i) reg_from(r[q][i], out->regs[out->reg_off[q] + (int64_t)i]);
		if (!a[q].empty()) memcpy(out->anchors + out->anchor_off[q], a[q].data(), a[q].size() * sizeof(mm2gb_anchor_t));
	}
	return 0;
}

int mm2gb_engine_release_host_scratch(mm2gb_engine_t *eng)
{
	if (!eng) return fail("mm2gb: null engine");
	if (eng->host_scratch) static_cast<HostScratch*>(eng->host_scratch)->release();
	return 0;
}

int mm2gb_map_reads_aln(mm2gb_engine_t *eng, const mm2gb_index_t *ix, int k, const char *const *ref_names, const int32_t *ref_lens, int32_t n_ref,
                        const mm2gb_map_opt_t *opt_in, const mm2gb_map_aln_t *aln, int32_t n_reads, const char *const *names, const char *const *seqs, const int32_t *lens,
                        char **paf_out, int64_t *paf_len, mm2gb_map_stats_t *stats, double *s_extra)
{
	return mm2gb_map_reads_aln_out(eng, ix, k, ref_names, ref_lens, n_ref, opt_in, aln, n_reads, names, seqs, lens, paf_out, paf_len, stats, s_extra, nullptr);
}

int mm2gb_map_reads_aln_out(mm2gb_engine_t *eng, const mm2gb_index_t *ix, int k, const char *const *ref_names, const int32_t *ref_lens, int32_t n_ref,
                            const mm2gb_map_opt_t *opt_in, const mm2gb_map_aln_t *aln, int32_t n_reads, const char *const *names, const char *const *seqs, const int32_t *lens,
                            char **paf_out, int64_t *paf_len, mm2gb_map_stats_t *stats, double *s_extra, const mm2gb_map_out_t *out)
{
	if (const char *why = bad_aln(aln)) return fail(std::string("mm2gb_map_reads_aln: ") + why);
	double s3[3] = { 0, 0, 0 };
	MapCall c = { eng, ix, k, ref_names, ref_lens, n_ref, opt_in, n_reads, names, seqs, lens, paf_out, paf_len, stats, aln, s3 };
	c.out = out;
	const int rc = map_reads_try(c);
	if (s_extra) for (int i = 0; i < 3; ++i) s_extra[i] = s3[i];
	return rc;
}

int mm2gb_map_reads(mm2gb_engine_t *eng, const mm2gb_index_t *ix, int k, const char *const *ref_names, const int32_t *ref_lens, int32_t n_ref,
                    const mm2gb_map_opt_t *opt_in, int32_t n_reads, const char *const *names, const char *const *seqs, const int32_t *lens,
                    char **paf_out, int64_t *paf_len, mm2gb_map_stats_t *stats)
{
	return map_reads_try({ eng, ix, k, ref_names, ref_lens, n_ref, opt_in, n_reads, names, seqs, lens, paf_out, paf_len, stats, nullptr, nullptr });
}

// Several devices (reads shard, no exchange): the batch is cut into contiguous runs of reads balanced by bases, every engine
// maps its run on its own host thread (the host threads of opt are shared out among them), the PAF comes back in read order.
int mm2gb_map_reads_multi(mm2gb_engine_t *const *engines, int n_engines, const mm2gb_index_t *ix, int k, const char *const *ref_names, const int32_t *ref_lens,
                          int32_t n_ref, const mm2gb_map_opt_t *opt_in, int32_t n_reads, const char *const *names, const char *const *seqs, const int32_t *lens,
                          char **paf_out, int64_t *paf_len, mm2gb_map_stats_t *stats)
{
	if (!engines || n_engines < 1 || !opt_in || !paf_out || !paf_len || n_reads < 0 || (n_reads > 0 && !lens)) return fail("mm2gb_map_reads_multi: null argument");
	if (n_engines == 1) return mm2gb_map_reads(engines[0], ix, k, ref_names, ref_lens, n_ref, opt_in, n_reads, names, seqs, lens, paf_out, paf_len, stats);
	*paf_out = nullptr; *paf_len = 0;
	int64_t total = 0;
	for (int32_t r = 0; r < n_reads; ++r) total += lens[r];
	std::vector<int32_t> cut((size_t)n_engines + 1, n_reads);
	cut[0] = 0;
	{ int64_t acc = 0; int e = 1; for (int32_t r = 0; r < n_reads && e < n_engines; ++r) { acc += lens[r]; if (acc * n_engines >= total * e) cut[(size_t)e++] = r + 1; } }
	mm2gb_map_opt_t opt = *opt_in;
	opt.host_threads = std::max(1, (opt_in->host_threads > 0 ? opt_in->host_threads : std::min(32, usable_cpus())) / n_engines);
	if (opt.mid_occ <= 0) opt.mid_occ = mm2gb_index_mid_occ(ix, opt.mid_occ_frac, opt.min_mid_occ, opt.max_mid_occ);     // once, not per engine
	std::vector<char*> part((size_t)n_engines, nullptr);
	std::vector<int64_t> part_len((size_t)n_engines, 0);
	std::vector<mm2gb_map_stats_t> st((size_t)n_engines);
	std::vector<int> rc((size_t)n_engines, 0);
	std::vector<std::string> err((size_t)n_engines);
	run_on_threads(n_engines, [&](int e) {
		const int32_t from = cut[(size_t)e], n = cut[(size_t)e + 1] - from;
		rc[(size_t)e] = mm2gb_map_reads(engines[e], ix, k, ref_names, ref_lens, n_ref, &opt, n, names + from, seqs + from, lens + from, &part[(size_t)e], &part_len[(size_t)e], &st[(size_t)e]);
		if (rc[(size_t)e]) err[(size_t)e] = mm2gb_last_error();          // error text is per thread: carry it over
	});
	int bad = -1;
	for (int e = 0; e < n_engines; ++e) if (rc[(size_t)e] && bad < 0) bad = e;
	if (bad >= 0) { for (char *p : part) free(p); return fail("mm2gb_map_reads_multi: engine " + std::to_string(bad) + ": " + err[(size_t)bad]); }
	return join_parts("mm2gb_map_reads_multi", part, part_len, st, false, paf_out, paf_len, stats);
}

int mm2gb_map_reads_stream(mm2gb_engine_t *const *engines, int n_engines, const mm2gb_index_t *ix, int k, const char *const *ref_names, const int32_t *ref_lens,
                           int32_t n_ref, const mm2gb_map_opt_t *opt_in, int32_t n_reads, const char *const *names, const char *const *seqs, const int32_t *lens,
                           int64_t chunk_bases, char **paf_out, int64_t *paf_len, mm2gb_map_stats_t *stats)
{
	return stream_body(engines, n_engines, chunk_bases, { nullptr, ix, k, ref_names, ref_lens, n_ref, opt_in, n_reads, names, seqs, lens, paf_out, paf_len, stats, nullptr, nullptr });
}

int mm2gb_map_reads_stream_aln(mm2gb_engine_t *const *engines, int n_engines, const mm2gb_index_t *ix, int k, const char *const *ref_names, const int32_t *ref_lens,
                               int32_t n_ref, const mm2gb_map_opt_t *opt_in, const mm2gb_map_aln_t *aln, int32_t n_reads, const char *const *names, const char *const *seqs,
                               const int32_t *lens, int64_t chunk_bases, char **paf_out, int64_t *paf_len, mm2gb_map_stats_t *stats, double *s_extra)
{
	return mm2gb_map_reads_stream_aln_out(engines, n_engines, ix, k, ref_names, ref_lens, n_ref, opt_in, aln, n_reads, names, seqs, lens, chunk_bases, paf_out, paf_len, stats, s_extra, nullptr);
}

int mm2gb_map_reads_stream_aln_out(mm2gb_engine_t *const *engines, int n_engines, const mm2gb_index_t *ix, int k, const char *const *ref_names, const int32_t *ref_lens,
                                   int32_t n_ref, const mm2gb_map_opt_t *opt_in, const mm2gb_map_aln_t *aln, int32_t n_reads, const char *const *names, const char *const *seqs,
                                   const int32_t *lens, int64_t chunk_bases, char **paf_out, int64_t *paf_len, mm2gb_map_stats_t *stats, double *s_extra, const mm2gb_map_out_t *out)
{
	if (const char *why = bad_aln(aln)) return fail(std::string("mm2gb_map_reads_stream_aln: ") + why);
	double s3[3] = { 0, 0, 0 };
	MapCall c = { nullptr, ix, k, ref_names, ref_lens, n_ref, opt_in, n_reads, names, seqs, lens, paf_out, paf_len, stats, aln, s3 };
	c.out = out;
	const int rc = stream_body(engines, n_engines, chunk_bases, c);
	if (s_extra) for (int i = 0; i < 3; ++i) s_extra[i] = s3[i];
	return rc;
}

// options.c:151-155 on top of mm_mapopt_init: the mapping fields of the `splice` presets
void mm2gb_map_opt_init_splice(mm2gb_map_opt_t *o)
{
	mm2gb_map_opt_init(o);
	o->bw = o->bw_long = o->max_gap_ref = 200000; o->max_gap = 2000;
}

namespace {
// the mm2gb_map_aln_t the shared stages read, from a mm2gb_map_splice_t; nullptr, or why it cannot be used
const char *splice_as_aln(const mm2gb_map_splice_t *s, mm2gb_map_aln_t &a)
{
	if (!s) return "null argument";
	a.ref_seqs = s->ref_seqs; a.opt = s->opt.base; a.what = s->what; a.align_on_device = s->align_on_device; a.text_on_device = s->text_on_device;
	return bad_aln(&a);
}
}

int mm2gb_map_reads_splice(mm2gb_engine_t *eng, const mm2gb_index_t *ix, int k, const char *const *ref_names, const int32_t *ref_lens, int32_t n_ref,
                           const mm2gb_map_opt_t *opt_in, const mm2gb_map_splice_t *spl, int32_t n_reads, const char *const *names, const char *const *seqs, const int32_t *lens,
                           char **paf_out, int64_t *paf_len, mm2gb_map_stats_t *stats, double *s_extra)
{
	return mm2gb_map_reads_splice_out(eng, ix, k, ref_names, ref_lens, n_ref, opt_in, spl, n_reads, names, seqs, lens, paf_out, paf_len, stats, s_extra, nullptr);
}

int mm2gb_map_reads_splice_out(mm2gb_engine_t *eng, const mm2gb_index_t *ix, int k, const char *const *ref_names, const int32_t *ref_lens, int32_t n_ref,
                               const mm2gb_map_opt_t *opt_in, const mm2gb_map_splice_t *spl, int32_t n_reads, const char *const *names, const char *const *seqs, const int32_t *lens,
                               char **paf_out, int64_t *paf_len, mm2gb_map_stats_t *stats, double *s_extra, const mm2gb_map_out_t *out)
{
	mm2gb_map_aln_t aln;
	if (const char *why = splice_as_aln(spl, aln)) return fail(std::string("mm2gb_map_reads_splice: ") + why);
	double s3[3] = { 0, 0, 0 };
	MapCall c = { eng, ix, k, ref_names, ref_lens, n_ref, opt_in, n_reads, names, seqs, lens, paf_out, paf_len, stats, &aln, s3 };
	c.spl = &spl->opt; c.out = out;
	const int rc = map_reads_try(c);
	if (s_extra) for (int i = 0; i < 3; ++i) s_extra[i] = s3[i];
	return rc;
}

int mm2gb_map_reads_stream_splice(mm2gb_engine_t *const *engines, int n_engines, const mm2gb_index_t *ix, int k, const char *const *ref_names, const int32_t *ref_lens,
                                  int32_t n_ref, const mm2gb_map_opt_t *opt_in, const mm2gb_map_splice_t *spl, int32_t n_reads, const char *const *names, const char *const *seqs,
                                  const int32_t *lens, int64_t chunk_bases, char **paf_out, int64_t *paf_len, mm2gb_map_stats_t *stats, double *s_extra)
{
	return mm2gb_map_reads_stream_splice_out(engines, n_engines, ix, k, ref_names, ref_lens, n_ref, opt_in, spl, n_reads, names, seqs, lens, chunk_bases, paf_out, paf_len, stats, s_extra, nullptr);
}

int mm2gb_map_reads_stream_splice_out(mm2gb_engine_t *const *engines, int n_engines, const mm2gb_index_t *ix, int k, const char *const *ref_names, const int32_t *ref_lens,
                                      int32_t n_ref, const mm2gb_map_opt_t *opt_in, const mm2gb_map_splice_t *spl, int32_t n_reads, const char *const *names, const char *const *seqs,
                                      const int32_t *lens, int64_t chunk_bases, char **paf_out, int64_t *paf_len, mm2gb_map_stats_t *stats, double *s_extra, const mm2gb_map_out_t *out)
{
	mm2gb_map_aln_t aln;
	if (const char *why = splice_as_aln(spl, aln)) return fail(std::string("mm2gb_map_reads_stream_splice: ") + why);
	double s3[3] = { 0, 0, 0 };
	MapCall c = { nullptr, ix, k, ref_names, ref_lens, n_ref, opt_in, n_reads, names, seqs, lens, paf_out, paf_len, stats, &aln, s3 };
	c.spl = &spl->opt; c.out = out;
	const int rc = stream_body(engines, n_engines, chunk_bases, c);
	if (s_extra) for (int i = 0; i < 3; ++i) s_extra[i] = s3[i];
	return rc;
}

void mm2gb_map_out_init(mm2gb_map_out_t *o) { if (o) memset(o, 0, sizeof *o); }

// mm_write_sam_hdr (format.c:118-139) without a read group: an @SQ line per reference, then this project's @PG line
int mm2gb_sam_header(int32_t n_ref, const char *const *ref_names, const int32_t *ref_lens, char **out, int64_t *len)
{
	if (!out || !len || n_ref < 0 || (n_ref > 0 && (!ref_names || !ref_lens))) return fail("mm2gb_sam_header: null argument");
	*out = nullptr; *len = 0;
	std::string s;
	for (int32_t i = 0; i < n_ref; ++i) {
		if (!ref_names[i]) return fail("mm2gb_sam_header: a reference without a name");
		s += "@SQ\tSN:"; s += ref_names[i]; s += "\tLN:"; append_int(s, ref_lens[i]); s += '\n';
	}
	s += "@PG\tID:mm2-gb_amd\tPN:mm2-gb_amd\n";
	char *buf = (char*)malloc(s.size() + 1);
	if (!buf) return fail("mm2gb_sam_header: out of memory");
	memcpy(buf, s.c_str(), s.size() + 1);
	*out = buf; *len = (int64_t)s.size();
	return 0;
}

} // extern "C"
