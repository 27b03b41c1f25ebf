// eqx.h -- internal: what the host and the device form of mm2gb_cigar_eqx_* share: mm_update_cigar_eqx (align.c:169-238) as a
// pass of its own over finished records.  Every M word becomes runs of = (op 7) and X (op 8), a run never crosses a word, I / D / N words are
// copied.  Restated per column so that columns can be taken in any order: a column is a START where a word of the result begins --
//   the first column of every word; an M column whose equality (target code == query code, N against N equal) differs from that of the column
//   before it in the same word.
// The word a start stores: an M column's "=" or "X" with the distance to the next start as its length; the input word itself otherwise (an
// I / D word takes `len` columns of which only the first is a start, so the distance to the next start is its own length anyway; an N word is
// ONE column, as in the text calls' plan).  Both forms lay a call out with tx_prepare (aln_text_host.h): the same checks, records, words, slices.
#pragma once
#include <string>
#include <vector>
#include "aln_text_host.h"

namespace mm2gb {

struct Engine;

constexpr int EQ_SLICE = 2048;          // columns of a slice: the cut of the text kernels (aln_text_kernels.hip: TX_SLICE)
constexpr int EQ_WG = 256;              // threads of a workgroup: a round takes EQ_WG columns (TX_WG)

// the call's checks and layout: tx_prepare's for the spliced text calls, and no = / X word (the rewrite has been done already); slice: 0 or EQ_SLICE
int eqx_prepare(const std::string &who, int32_t n_ref, const int32_t *ref_lens, const int64_t *ref_at, int64_t n_reads, const int32_t *read_lens, const int64_t *read_at,
                int64_t n_regs, const mm2gb_reg_t *regs, const int32_t *read_of_reg, const mm2gb_aln_t *aln, const uint32_t *cigar, int slice, TxPlan &plan);

// the call's results from the words per record of the plan: n_words[k] words for plan.recs[k], laid end to end in that order.  *aln_out: aln with
// cigar_off / n_cigar of the new words (a record without a CIGAR stays as it is); *cigar_out: room for them all (malloc'd, at least one word)
int eqx_results(const std::string &who, const TxPlan &plan, int64_t n_regs, const mm2gb_aln_t *aln, const int64_t *n_words, mm2gb_aln_t **aln_out, uint32_t **cigar_out);

// the device form on residues resident in e.al_refs / e.al_reads (as aln_text_resident takes them)
int cigar_eqx_resident(Engine &e, const char *who, int32_t n_ref, const int32_t *ref_lens, const int64_t *ref_at, int64_t n_reads, const int32_t *read_lens, const int64_t *read_at,
                       int64_t n_regs, const mm2gb_reg_t *regs, const int32_t *read_of_reg, const mm2gb_aln_t *aln, const uint32_t *cigar, mm2gb_aln_t **aln_out, uint32_t **cigar_out);

} // namespace mm2gb
