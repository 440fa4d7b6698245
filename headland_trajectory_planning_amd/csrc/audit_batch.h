// htp_obca_batch + htp_obca_audit_opts/result -> the audit core's launch shape and pointer view, with the
// argument checks of the C ABI; shared by the gfx950 library (htp_audit.hip) and the test-only host build
// (audit_hostsim.cpp).
#pragma once
#include "../../include/htp.h"
#include "audit_core.h"

namespace htp {
namespace audit {

static_assert(HTP_AUDIT_NMETRIC == 8, "htp.h audit metrics");

// 0 = OK; -1 with *err set: nothing may be launched
inline int check_args(const htp_obca_batch* in, const double* x, const htp_obca_audit_opts* o,
                      const htp_obca_audit_result* out, const char** err) {
  if (!in || !o || !out) { *err = "[audit] null argument"; return -1; }
  if (in->batch < 0) { *err = "[audit] batch must be >= 0"; return -1; }
  if (in->N < 2) { *err = "[audit] N must be >= 2"; return -1; }
  if (in->N > MAXN) { *err = "[audit] N must be <= HTP_AUDIT_MAX_N (480)"; return -1; }
  if (in->M < 1 || in->M > MAXM) { *err = "[audit] M must be in [1, 16]"; return -1; }
  if (in->K < 1 || in->K > MAXK) { *err = "[audit] K must be in [1, 4]"; return -1; }
  if (o->substeps < 1 || o->substeps > MAXSUB) { *err = "[audit] substeps must be in [1, HTP_AUDIT_MAX_SUBSTEPS (16)]"; return -1; }
  if (!(o->margin_tol >= 0.0) || !(o->dyn_tol >= 0.0) || !(o->bound_tol >= 0.0) || !(o->term_tol >= 0.0)) {
    *err = "[audit] tolerances must be >= 0";
    return -1;
  }
  if (!in->obs_edges || !in->body_edges) { *err = "[audit] null argument (edge counts)"; return -1; }
  for (int m = 0; m < in->M; ++m)
    if (in->obs_edges[m] < 3 || in->obs_edges[m] > MAXE) { *err = "[audit] obstacle edges must be in [3, 8]"; return -1; }
  for (int k = 0; k < in->K; ++k)
    if (in->body_edges[k] < 3 || in->body_edges[k] > MAXE) { *err = "[audit] body edges must be in [3, 8]"; return -1; }
  if (in->batch == 0) return 0;
  if (!x || !in->traj || !in->obs_A || !in->obs_b || !in->body_G || !in->body_g || !in->params) {
    *err = "[audit] null argument (input array)";
    return -1;
  }
  if (!out->metrics || !out->worst || !out->flags) { *err = "[audit] null argument (output array)"; return -1; }
  return 0;
}

inline Batch batch_view(const htp_obca_batch& in, const double* x, const htp_obca_audit_result& out) {
  return Batch{in.traj, in.obs_A, in.obs_b, in.body_G, in.body_g, in.params, x,
               out.metrics, out.worst, out.flags, out.stage_clearance};
}

}  // namespace audit
}  // namespace htp
