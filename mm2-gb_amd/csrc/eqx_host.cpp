// eqx_host.cpp -- mm_update_cigar_eqx (align.c:169-238) for a batch of finished records (mm2gb_cigar_eqx_host): every M word of a
// record becomes runs of = and X, written from scratch as a call of its own on what the alignment calls return.  A record is walked word by
// word; the device form (eqx_kernels.hip) takes the same columns in parallel with the rule of eqx.h.  The host form is the definition.
// This unit also checks a call and shapes its results for either form (eqx_prepare, eqx_results).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "engine.h"
#include "host_threads.h"
#include "align_host.h"
#include "eqx.h"

namespace mm2gb {

int eqx_prepare(const std::string &who, int32_t n_ref, const int32_t *ref_lens, const int64_t *ref_at, int64_t n_reads, const int32_t *read_lens, const int64_t *read_at,
                int64_t n_regs, const mm2gb_reg_t *regs, const int32_t *read_of_reg, const mm2gb_aln_t *aln, const uint32_t *cigar, int slice, TxPlan &plan)
{
	if (aln && cigar)
		for (int64_t i = 0; i < n_regs; ++i)
			for (int32_t k = 0; aln[i].cigar_off >= 0 && k < aln[i].n_cigar; ++k) {
				const uint32_t op = cigar[aln[i].cigar_off + k] & 0xf;
				if (op == 7 || op == 8) return fail(who + ": record " + std::to_string(i) + ": CIGAR operation " + (op == 7 ? "=" : "X") + " in the input: its M words have been rewritten already");
			}
	return tx_prepare(true, who, MM2GB_TEXT_CS, n_ref, ref_lens, ref_at, n_reads, read_lens, read_at, n_regs, regs, read_of_reg, aln, cigar, slice, plan);
}

int eqx_results(const std::string &who, const TxPlan &plan, int64_t n_regs, const mm2gb_aln_t *aln, const int64_t *n_words, mm2gb_aln_t **aln_out, uint32_t **cigar_out)
{
	mm2gb_aln_t *a = (mm2gb_aln_t*)malloc((size_t)std::max<int64_t>(n_regs, 1) * sizeof(mm2gb_aln_t));
	if (!a) return fail(who + ": out of memory");
	if (n_regs > 0) memcpy(a, aln, (size_t)n_regs * sizeof(mm2gb_aln_t));
	int64_t total = 0;
	for (size_t k = 0; k < plan.recs.size(); ++k) {
		if (n_words[k] > INT32_MAX) { free(a); return fail(who + ": a record of more than 2^31 words"); }
		a[plan.reg_of[k]].cigar_off = total; a[plan.reg_of[k]].n_cigar = (int32_t)n_words[k];
		total += n_words[k];
	}
	uint32_t *w = (uint32_t*)malloc((size_t)std::max<int64_t>(total, 1) * sizeof(uint32_t));
	if (!w) { free(a); return fail(who + ": out of memory"); }
	*aln_out = a; *cigar_out = w;
	return 0;
}

} // namespace mm2gb

using namespace mm2gb;

int mm2gb_cigar_eqx_host(int32_t n_ref, const char *const *ref_seqs, const int32_t *ref_lens, int64_t n_reads, const char *const *read_seqs, const int32_t *read_lens,
                         int64_t n_regs, const mm2gb_reg_t *regs, const int32_t *read_of_reg, const mm2gb_aln_t *aln, const uint32_t *cigar, int n_threads,
                         mm2gb_aln_t **aln_out, uint32_t **cigar_out)
{
	const std::string who = "mm2gb_cigar_eqx_host";
	if (!aln_out || !cigar_out) return fail(who + ": null argument");
	*aln_out = nullptr; *cigar_out = nullptr;
	if ((n_ref > 0 && !ref_seqs) || (n_reads > 0 && !read_seqs)) return fail(who + ": null argument");
	TxPlan p;
	if (eqx_prepare(who, n_ref, ref_lens, nullptr, n_reads, read_lens, nullptr, n_regs, regs, read_of_reg, aln, cigar, 0, p)) return -1;
	const size_t n = p.recs.size();
	std::vector<std::vector<uint32_t>> out(n);
	for_each_on_threads(n, std::min(std::max(n_threads, 1), 256), 1, [&](size_t i) {
		const TxRec &x = p.recs[i];
		const mm2gb_reg_t &g = regs[p.reg_of[i]];
		const char *ref = ref_seqs[g.rid], *read = read_seqs[read_of_reg[p.reg_of[i]]];
		const TxWord *W = p.words.data() + x.w_off;
		std::vector<uint32_t> &o = out[i];
		o.reserve((size_t)x.n_words);
		for (int32_t k = 0; k < x.n_words; ++k) {
			if ((W[k].w & 0xf) != 0) { o.push_back(W[k].w); continue; }
			const int len = (int)(W[k].w >> 4);
			int from = 0;
			bool eq_run = false;
			for (int j = 0; j <= len; ++j) {
				bool eq = false;
				if (j < len) {
					const int t = nt4(ref[x.t_at + W[k].t + j]);
					int q = nt4(read[x.rev ? x.q_at - (W[k].q + j) : x.q_at + W[k].q + j]);
					if (x.rev) q = q < 4 ? 3 - q : 4;
					eq = t == q;
				}
				if (j > 0 && (j == len || eq != eq_run)) { o.push_back((uint32_t)(j - from) << 4 | (eq_run ? 7u : 8u)); from = j; }
				eq_run = eq;
			}
		}
	});
	std::vector<int64_t> n_words(n);
	for (size_t i = 0; i < n; ++i) n_words[i] = (int64_t)out[i].size();
	if (eqx_results(who, p, n_regs, aln, n_words.data(), aln_out, cigar_out)) return -1;
	for (size_t i = 0; i < n; ++i) if (!out[i].empty()) memcpy(*cigar_out + (*aln_out)[p.reg_of[i]].cigar_off, out[i].data(), out[i].size() * sizeof(uint32_t));
	return 0;
}
