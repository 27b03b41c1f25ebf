// ksw_host.h -- internal: what the two forms of the extension DP share on the host side (ksw_host.cpp).
#pragma once
#include "ksw_cell.h"

namespace mm2gb {

// every refusal of mm2gb_ksw_extd2_*: 0, or -1 with the error text set and nothing run
int  ksw_check(const char *who, const mm2gb_ksw_param_t *param, int64_t n_jobs, const mm2gb_ksw_job_t *jobs, const uint8_t *queries, const uint8_t *targets,
               const mm2gb_ksw_res_t *res, uint32_t **cigar, int64_t *n_cigar_total);
void ksw_store(const KswEz &z, int n_cigar, mm2gb_ksw_res_t *out);
// cigar_off of every job from its n_cigar, and the batch's word array (malloc'd, NULL when empty)
int  ksw_gather(int64_t n_jobs, mm2gb_ksw_res_t *res, uint32_t **cigar, int64_t *n_cigar_total);

} // namespace mm2gb
