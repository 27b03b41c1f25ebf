// ksw_host.h -- internal: what the forms of the extension DP share on the host side (ksw_host.cpp).
#pragma once
#include <vector>
#include "ksw_cell.h"

namespace mm2gb {

// every refusal of mm2gb_ksw_extd2_*: 0, or -1 with the error text set and nothing run
int  ksw_check(const char *who, const mm2gb_ksw_param_t *param, int64_t n_jobs, const mm2gb_ksw_job_t *jobs, const uint8_t *queries, const uint8_t *targets,
               const mm2gb_ksw_res_t *res, uint32_t **cigar, int64_t *n_cigar_total);
int  ksw_check_splice(const char *who, const mm2gb_ksw_splice_param_t *param, int64_t n_jobs, const mm2gb_ksw_job_t *jobs, const uint8_t *queries, const uint8_t *targets,
                      const mm2gb_ksw_res_t *res, uint32_t **cigar, int64_t *n_cigar_total);        // ... and of mm2gb_ksw_exts2_*
int  ksw_check_single(const char *who, const mm2gb_ksw_param_t *param, int64_t n_jobs, const mm2gb_ksw_job_t *jobs, const uint8_t *queries, const uint8_t *targets,
                      const mm2gb_ksw_res_t *res, uint32_t **cigar, int64_t *n_cigar_total);        // ... and of mm2gb_ksw_extz2_*
// one job on the calling thread (the body of mm2gb_ksw_extd2_host or, by c.form, of mm2gb_ksw_exts2_host without annotation or of mm2gb_ksw_extz2_host; the thread keeps its scratch): the record, and the job's words appended
void ksw_one_host(const KswConst &c, const mm2gb_ksw_job_t &job, const uint8_t *query, const uint8_t *target, mm2gb_ksw_res_t *out, std::vector<uint32_t> &words);
// cigar_off of every job from its n_cigar, and the batch's word array (malloc'd, NULL when empty)
int  ksw_gather(int64_t n_jobs, mm2gb_ksw_res_t *res, uint32_t **cigar, int64_t *n_cigar_total);

// the device forms' planning and launches (ksw_kernels.hip), c.form choosing the DP; junc: the splice-aware form's annotation bytes, indexed
// like targets, or null; resident: the sequences already lie in the engine's arenas
struct Engine;
int  ksw_run(Engine &e, const KswConst &c, int64_t n_jobs, const mm2gb_ksw_job_t *jobs, const uint8_t *queries, const uint8_t *targets, const uint8_t *junc, bool resident,
             mm2gb_ksw_res_t *res, uint32_t **cigar, int64_t *n_cigar_total);

} // namespace mm2gb
