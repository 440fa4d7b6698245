// htp_obca_batch + htp_obca_ltrack_opts/result -> the ltrack core's launch shape and pointer view, with the
// argument checks of the C ABI; shared by the gfx950 library (htp_ltrack.hip) and the test-only host build
// (ltrack_hostsim.cpp).
#pragma once
#include "../../include/htp.h"
#include "ltrack_core.h"

namespace htp {
namespace ltrack {

static_assert(HTP_TRACK_NMETRIC == 8 && HTP_TRACK_NDIST == 6 && HTP_TRACK_NFLAG == 10, "htp.h track sizes");
static_assert(HTP_LQR_NGAIN == 10, "htp.h gain row");

// 0 = OK; -1 with *err set: nothing may be launched
inline int check_args(const htp_obca_batch* in, const double* x, const htp_obca_ltrack_opts* o,
                      const htp_obca_ltrack_result* out, const char** err) {
  using audit::nonfinite_;
  if (!in || !o || !out) { *err = "[ltrack] null argument"; return -1; }
  if (in->batch < 0) { *err = "[ltrack] batch must be >= 0"; return -1; }
  if (in->N < 2) { *err = "[ltrack] N must be >= 2"; return -1; }
  if (in->N > MAXN) { *err = "[ltrack] N must be <= HTP_TRACK_MAX_N (480)"; return -1; }
  if (in->M < 1 || in->M > MAXM) { *err = "[ltrack] M must be in [1, 16]"; return -1; }
  if (in->K < 1 || in->K > MAXK) { *err = "[ltrack] K must be in [1, 4]"; return -1; }
  if (nonfinite_(o->dt) || !(o->dt > 0.0)) { *err = "[ltrack] dt must be finite and > 0"; return -1; }
  if (o->max_ticks < 2) { *err = "[ltrack] max_ticks must be >= 2"; return -1; }
  if (o->plant_substeps < 1 || o->plant_substeps > HTP_TRACK_MAX_SUBSTEPS) {
    *err = "[ltrack] plant_substeps must be in [1, HTP_TRACK_MAX_SUBSTEPS (16)]";
    return -1;
  }
  if (o->R < 1 || o->R > HTP_TRACK_MAX_SCENARIOS) { *err = "[ltrack] R must be in [1, HTP_TRACK_MAX_SCENARIOS (4096)]"; return -1; }
  if (nonfinite_(o->margin_tol) || !(o->margin_tol >= 0.0)) { *err = "[ltrack] margin_tol must be finite and >= 0"; return -1; }
  if (!(o->abort_dist > 0.0)) { *err = "[ltrack] abort_dist must be > 0"; return -1; }
  if (!in->obs_edges || !in->body_edges) { *err = "[ltrack] null argument (edge counts)"; return -1; }
  for (int m = 0; m < in->M; ++m)
    if (in->obs_edges[m] < 3 || in->obs_edges[m] > MAXE) { *err = "[ltrack] obstacle edges must be in [3, 8]"; return -1; }
  for (int k = 0; k < in->K; ++k)
    if (in->body_edges[k] < 3 || in->body_edges[k] > MAXE) { *err = "[ltrack] body edges must be in [3, 8]"; return -1; }
  if (in->batch == 0) return 0;
  if (!x || !in->obs_A || !in->obs_b || !in->body_G || !in->body_g || !in->params || !o->scenarios) {
    *err = "[ltrack] null argument (input array)";
    return -1;
  }
  if (!o->gains) { *err = "[ltrack] null argument (gains)"; return -1; }
  if (!out->metrics || !out->worst || !out->flags || !out->tally || !out->worst_scenario) {
    *err = "[ltrack] null argument (output array)";
    return -1;
  }
  return 0;
}

inline Batch batch_view(const htp_obca_batch& in, const double* x, const htp_obca_ltrack_opts& o,
                        const htp_obca_ltrack_result& out) {
  return Batch{track::Batch{in.obs_A, in.obs_b, in.body_G, in.body_g, in.params, x, o.scenarios, out.metrics,
                            out.worst, out.flags, out.tally, out.worst_scenario, out.tick_clearance, out.reference},
               o.gains, out.tick_error};
}

}  // namespace ltrack
}  // namespace htp
