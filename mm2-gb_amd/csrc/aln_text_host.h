// aln_text_host.h -- internal: what aln_text_host.cpp offers the device form (aln_text_kernels.hip): the checked batch, cut into slices, and
// the entry that takes sequences already resident on the device.
#pragma once
#include <string>
#include <vector>
#include "aln_text_cell.h"
#include "../../include/mm2gb_chain.h"

namespace mm2gb {

struct Engine;

// a CIGAR word with the column, the query position and the target position it starts at, all counted within its record
struct TxWord { int32_t col, q, t; uint32_t w; };
// a record with a CIGAR: t_at / q_at: where column position 0's residues lie in the batch's residue arrays (q_at: the residue at qe - 1 of a
// reverse-strand record, read downwards); its words and its slices
struct TxRec { int64_t t_at, q_at, w_off; int32_t n_words, n_cols, rev, s_first, n_cg_slices, n_tag_slices; };
// kind 0: words [start, start + n) of the record for cg:Z; kind 1: columns [start, start + n) for cs:Z / MD:Z, which lie in the n_w words
// from w_first on
struct TxSlice { int32_t rec, kind, start, n, w_first, n_w; };

struct TxPlan {
	int mode = TX_CS;
	bool cg = false, tag = false, introns = false;      // introns: some word is an N
	std::vector<TxRec> recs;
	std::vector<int64_t> reg_of;          // recs[i] is record reg_of[i] of the call
	std::vector<TxWord> words;
	std::vector<TxSlice> slices;
};

// checks the call (every refusal of mm2gb_aln_text_*) and lays the batch out; ref_at / read_at: n + 1 each, where a sequence's residues begin;
// slice: columns (words) per slice, 0: no slices wanted (the host form); splice: the spliced calls, which take N words (one column each)
int tx_prepare(bool splice, const std::string &who, int what, int32_t n_ref, const int32_t *ref_lens, const int64_t *ref_at, int64_t n_reads, const int32_t *read_lens,
               const int64_t *read_at, int64_t n_regs, const mm2gb_reg_t *regs, const int32_t *read_of_reg, const mm2gb_aln_t *aln, const uint32_t *cigar,
               int slice, TxPlan &plan);

// the device form on residues resident in e.al_refs / e.al_reads (one byte per base, laid out by ref_at / read_at as AlCtx has them)
int aln_text_resident(Engine &e, bool splice, const char *who, int what, int32_t n_ref, const int32_t *ref_lens, const int64_t *ref_at, int64_t n_reads, const int32_t *read_lens,
                      const int64_t *read_at, int64_t n_regs, const mm2gb_reg_t *regs, const int32_t *read_of_reg, const mm2gb_aln_t *aln, const uint32_t *cigar,
                      int64_t **text_off, char **text);

} // namespace mm2gb
