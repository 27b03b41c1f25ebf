// aln_text_host.cpp -- the text of a PAF line's alignment tags for a batch of records (mm2gb_aln_text_host): what mm_write_paf3
// appends after rl:i (format.c:322-329) -- cg:Z from the CIGAR words, cs:Z or MD:Z from the words and both sequences (write_cs_core,
// write_MD_core, format.c:141-218) -- written from scratch as a batch call.  A record is walked column by column with the rule of
// aln_text_cell.h and a running count; the device form (aln_text_kernels.hip) takes the same columns in parallel.  The host form is the
// definition.  This unit also checks a call and lays it out for either form (tx_prepare).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "engine.h"
#include "host_threads.h"
#include "align_host.h"
#include "aln_text_host.h"

namespace mm2gb {

namespace {
constexpr uint32_t RF_REV = 1u << 10;          // mm_reg1_t's bit-field word (minimap.h:115)
constexpr int WHAT_ALL = MM2GB_TEXT_CG | MM2GB_TEXT_CS | MM2GB_TEXT_CS_LONG | MM2GB_TEXT_MD;
}

int tx_prepare(bool splice, const std::string &who, int what, int32_t n_ref, const int32_t *ref_lens, const int64_t *ref_at, int64_t n_reads, const int32_t *read_lens,
               const int64_t *read_at, int64_t n_regs, const mm2gb_reg_t *regs, const int32_t *read_of_reg, const mm2gb_aln_t *aln, const uint32_t *cigar,
               int slice, TxPlan &plan)
{
	if (what & ~WHAT_ALL) return fail(who + ": what has a bit outside MM2GB_TEXT_*");
	if (n_regs < 0 || n_ref < 0 || n_reads < 0 || (n_regs > 0 && (!regs || !read_of_reg || !aln)) || (n_ref > 0 && !ref_lens) || (n_reads > 0 && !read_lens)) return fail(who + ": null argument");
	plan.cg = what & MM2GB_TEXT_CG; plan.tag = what & (MM2GB_TEXT_CS | MM2GB_TEXT_MD);
	plan.mode = what & MM2GB_TEXT_MD ? TX_MD : what & MM2GB_TEXT_CS_LONG ? TX_CS_LONG : TX_CS;
	for (int64_t i = 0; i < n_regs; ++i) {
		if (aln[i].cigar_off < 0) continue;
		const mm2gb_reg_t &g = regs[i];
		const std::string rec = who + ": record " + std::to_string(i);
		const int64_t r = read_of_reg[i];
		if (aln[i].n_cigar < 0 || (aln[i].n_cigar > 0 && !cigar)) return fail(rec + ": no CIGAR words");
		if (r < 0 || r >= n_reads || g.rid < 0 || g.rid >= n_ref || g.rs < 0 || g.rs > g.re || g.re > ref_lens[g.rid] || g.qs < 0 || g.qs > g.qe || g.qe > read_lens[r])
			return fail(rec + " lies outside its sequences");
		TxRec x;
		x.rev = g.flags & RF_REV ? 1 : 0;
		x.t_at = (ref_at ? ref_at[g.rid] : 0) + g.rs;
		x.q_at = (read_at ? read_at[r] : 0) + (x.rev ? g.qe - 1 : g.qs);
		x.w_off = (int64_t)plan.words.size(); x.n_words = aln[i].n_cigar;
		int64_t col = 0, q = 0, t = 0;
		for (int32_t k = 0; k < aln[i].n_cigar; ++k) {
			const uint32_t w = cigar[aln[i].cigar_off + k], op = w & 0xf, len = w >> 4;
			if (op > (splice ? 3u : 2u)) return fail(rec + ": CIGAR operation " + std::string(1, "MIDNSHP=XB??????"[op]) + " is not supported (" + (splice ? "M, I, D and N are)" : "M, I and D are)"));
			if (len == 0) return fail(rec + ": a CIGAR word of length 0");
			if (op == 3 && len < 2) return fail(rec + ": an N word shorter than 2 (format.c:180 asserts it)");
			plan.words.push_back({ (int32_t)col, (int32_t)q, (int32_t)t, w });
			if (op == 3) { col += 1; t += len; plan.introns = true; }          // an intron is one column
			else { col += len; if (op != 2) q += len; if (op != 1) t += len; }
			if (col > INT32_MAX) return fail(rec + ": more than 2^31 columns");
		}
		if (q != g.qe - g.qs || t != g.re - g.rs) return fail(rec + ": its CIGAR words do not sum to qe - qs and re - rs");
		x.n_cols = (int32_t)col;
		x.s_first = (int32_t)plan.slices.size(); x.n_cg_slices = x.n_tag_slices = 0;
		if (slice > 0) {
			const int32_t rid = (int32_t)plan.recs.size();
			if (plan.cg) for (int32_t s = 0; s == 0 || s < x.n_words; s += slice) { plan.slices.push_back({ rid, 0, s, std::min(slice, x.n_words - s), 0, 0 }); ++x.n_cg_slices; }
			if (plan.tag) {
				const TxWord *W = plan.words.data() + x.w_off;
				int32_t w0 = 0;
				for (int32_t s = 0; s == 0 || s < x.n_cols; s += slice) {
					const int32_t n = std::min(slice, x.n_cols - s);
					while (w0 + 1 < x.n_words && W[w0 + 1].col <= s) ++w0;
					int32_t w1 = w0;
					while (w1 + 1 < x.n_words && W[w1 + 1].col < s + n) ++w1;
					plan.slices.push_back({ rid, 1, s, n, w0, n > 0 ? w1 - w0 + 1 : 0 });
					++x.n_tag_slices;
				}
			}
			if (plan.slices.size() >= ((size_t)1 << 31)) return fail(who + ": more than 2^31 slices");
		}
		plan.recs.push_back(x); plan.reg_of.push_back(i);
	}
	return 0;
}

namespace {

// one record's text, appended to s: T(k) / Q(k): residue k of the record's target / query stretch, the query on the record's strand
template <class FT, class FQ> void tx_walk(const TxPlan &p, const TxRec &x, FT T, FQ Q, std::string &s)
{
	const TxWord *W = p.words.data() + x.w_off;
	auto put = [&s](int64_t at, char ch) { s[(size_t)at] = ch; };
	if (p.cg) {
		s += "\tcg:Z:";
		for (int32_t k = 0; k < x.n_words; ++k) { const size_t at = s.size(); s.resize(at + (size_t)tx_word_bytes(W[k].w)); tx_put_word(W[k].w, (int64_t)at, put); }
	}
	if (!p.tag) return;
	s += p.mode == TX_MD ? "\tMD:Z:" : "\tcs:Z:";
	int run = 0;
	auto close = [&](bool at_end) { const size_t at = s.size(); s.resize(at + (size_t)tx_len_bytes(p.mode, at_end, run)); tx_put_len(p.mode, at_end, run, (int64_t)at, put); run = 0; };
	for (int32_t k = 0; k < x.n_words; ++k) {
		const int op = (int)(W[k].w & 0xf), len = (int)(W[k].w >> 4);
		bool prev = false;
		if (op == 3) {          // an intron: one column, its own bytes in cs, nothing in MD
			if (p.mode == TX_MD) continue;
			if (p.mode == TX_CS) close(false);
			const size_t at = s.size();
			s.resize(at + (size_t)tx_intron_bytes((uint32_t)len));
			tx_put_intron((uint32_t)len, T(W[k].t), T(W[k].t + 1), T(W[k].t + len - 2), T(W[k].t + len - 1), (int64_t)at, put);
			continue;
		}
		for (int j = 0; j < len; ++j) {
			const int t = op != 1 ? T(W[k].t + j) : 0, q = op != 2 ? Q(W[k].q + j) : 0;
			const TxCol c = tx_col(p.mode, op, j == 0, t, q, prev);
			prev = op == 0 && t == q;
			if (c.ev) close(false);
			run += c.m;
			s.append(c.own, c.n_own);
		}
	}
	close(true);
}

} // namespace

} // namespace mm2gb

using namespace mm2gb;

namespace {

int aln_text_host_any(bool splice, const char *who_, int what, int32_t n_ref, const char *const *ref_seqs, const int32_t *ref_lens, int64_t n_reads, const char *const *read_seqs,
                      const int32_t *read_lens, int64_t n_regs, const mm2gb_reg_t *regs, const int32_t *read_of_reg, const mm2gb_aln_t *aln, const uint32_t *cigar, int n_threads,
                      int64_t **text_off, char **text)
{
	const std::string who = who_;
	if (!text_off || !text) return fail(who + ": null argument");
	*text_off = nullptr; *text = nullptr;
	if ((n_ref > 0 && !ref_seqs) || (n_reads > 0 && !read_seqs)) return fail(who + ": null argument");
	TxPlan p;
	if (tx_prepare(splice, who, what, n_ref, ref_lens, nullptr, n_reads, read_lens, nullptr, n_regs, regs, read_of_reg, aln, cigar, 0, p)) return -1;
	const size_t n = p.recs.size();
	std::vector<std::string> out(n);
	auto one = [&](size_t i) {
		const TxRec &x = p.recs[i];
		const mm2gb_reg_t &g = regs[p.reg_of[i]];
		const char *ref = ref_seqs[g.rid], *read = read_seqs[read_of_reg[p.reg_of[i]]];
		tx_walk(p, x, [&](int k) { return (int)nt4(ref[x.t_at + k]); },
		        [&](int k) { if (!x.rev) return (int)nt4(read[x.q_at + k]); const int c = nt4(read[x.q_at - k]); return c < 4 ? 3 - c : 4; }, out[i]);
	};
	for_each_on_threads(n, std::min(n_threads, 256), 1, one);
	int64_t *off = (int64_t*)malloc(((size_t)n_regs + 1) * sizeof(int64_t));
	if (!off) return fail(who + ": out of memory");
	int64_t total = 0;
	size_t k = 0;
	for (int64_t i = 0; i < n_regs; ++i) { off[i] = total; if (k < n && p.reg_of[k] == i) total += (int64_t)out[k++].size(); }
	off[n_regs] = total;
	char *buf = (char*)malloc((size_t)std::max<int64_t>(total, 1));
	if (!buf) { free(off); return fail(who + ": out of memory"); }
	k = 0;
	for (int64_t i = 0; i < n_regs; ++i) if (k < n && p.reg_of[k] == i) { memcpy(buf + off[i], out[k].data(), out[k].size()); ++k; }
	*text_off = off; *text = buf;
	return 0;
}

} // namespace

int mm2gb_aln_text_host(int what, int32_t n_ref, const char *const *ref_seqs, const int32_t *ref_lens, int64_t n_reads, const char *const *read_seqs, const int32_t *read_lens,
                        int64_t n_regs, const mm2gb_reg_t *regs, const int32_t *read_of_reg, const mm2gb_aln_t *aln, const uint32_t *cigar, int n_threads,
                        int64_t **text_off, char **text)
{
	return aln_text_host_any(false, "mm2gb_aln_text_host", what, n_ref, ref_seqs, ref_lens, n_reads, read_seqs, read_lens, n_regs, regs, read_of_reg, aln, cigar, n_threads, text_off, text);
}

int mm2gb_aln_text_splice_host(int what, int32_t n_ref, const char *const *ref_seqs, const int32_t *ref_lens, int64_t n_reads, const char *const *read_seqs, const int32_t *read_lens,
                               int64_t n_regs, const mm2gb_reg_t *regs, const int32_t *read_of_reg, const mm2gb_aln_t *aln, const uint32_t *cigar, int n_threads,
                               int64_t **text_off, char **text)
{
	return aln_text_host_any(true, "mm2gb_aln_text_splice_host", what, n_ref, ref_seqs, ref_lens, n_reads, read_seqs, read_lens, n_regs, regs, read_of_reg, aln, cigar, n_threads, text_off, text);
}
