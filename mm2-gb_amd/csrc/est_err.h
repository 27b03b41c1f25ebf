// est_err.h -- internal: mm_est_err's walk (esterr.c:30-61) for one read, and what both batched forms check before they run.
#pragma once
#include <stdint.h>
#include "../../include/mm2gb_chain.h"

namespace mm2gb {

// one read: out[i] for regs[i] (as: within a[]), *sum_k (0 and every out marked when n_mini == 0)
void est_err_read(int32_t qlen, int64_t n_regs, const mm2gb_reg_t *regs, const mm2gb_anchor_t *a, int32_t n_mini, const uint64_t *mini_pos, const int32_t *ref_len,
                  mm2gb_est_err_t *out, uint64_t *sum_k);

// 0, or -1 with the error text: the arguments of mm2gb_est_err_host / _gpu (every index a record holds is looked up by the walk)
int est_err_check(const char *who, int64_t n_reads, const int64_t *reg_off, const mm2gb_reg_t *regs, const int64_t *anchor_off, const mm2gb_anchor_t *anchors, const int32_t *qlen,
                  const int64_t *mini_off, const uint64_t *mini_pos, int32_t n_ref, const int32_t *ref_len, const mm2gb_est_err_t *out, const uint64_t *sum_k);

} // namespace mm2gb
