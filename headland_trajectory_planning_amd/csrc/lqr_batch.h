// htp_obca_batch + htp_obca_lqr_opts/result -> the lqr core's launch shape and pointer view, with the argument
// checks of the C ABI; shared by the gfx950 library (htp_lqr.hip) and the test-only host build (lqr_hostsim.cpp).
#pragma once
#include "../../include/htp.h"
#include "lqr_core.h"

namespace htp {
namespace lqr {

// 0 = OK; -1 with *err set: nothing may be launched
inline int check_args(const htp_obca_batch* in, const double* x, const htp_obca_lqr_opts* o,
                      const htp_obca_lqr_result* out, const char** err) {
  using audit::nonfinite_;
  if (!in || !o || !out) { *err = "[lqr] null argument"; return -1; }
  if (in->batch < 0) { *err = "[lqr] batch must be >= 0"; return -1; }
  if (in->N < 2) { *err = "[lqr] N must be >= 2"; return -1; }
  if (in->N > MAXN) { *err = "[lqr] N must be <= HTP_LQR_MAX_N (480)"; return -1; }
  if (in->M < 1 || in->M > MAXM) { *err = "[lqr] M must be in [1, 16]"; return -1; }
  if (in->K < 1 || in->K > MAXK) { *err = "[lqr] K must be in [1, 4]"; return -1; }
  const double wt[6] = {o->q_lon, o->q_lat, o->q_v, o->q_th, o->q_st, o->qf};
  for (double v : wt)
    if (nonfinite_(v) || !(v >= 0.0)) { *err = "[lqr] weights q_* and qf must be finite and >= 0"; return -1; }
  if (nonfinite_(o->r_a) || nonfinite_(o->r_w) || !(o->r_a > 0.0) || !(o->r_w > 0.0)) {
    *err = "[lqr] control weights r_a and r_w must be finite and > 0";
    return -1;
  }
  const double sg[10] = {o->sig0_lon, o->sig0_lat, o->sig0_v, o->sig0_th, o->sig0_st,
                         o->w_lon, o->w_lat, o->w_v, o->w_th, o->w_st};
  for (double v : sg)
    if (nonfinite_(v) || !(v >= 0.0)) { *err = "[lqr] sigmas sig0_* and w_* must be finite and >= 0"; return -1; }
  if (!(o->k_sigma >= 0.0)) { *err = "[lqr] k_sigma must be >= 0"; return -1; }
  if (!in->obs_edges || !in->body_edges) { *err = "[lqr] null argument (edge counts)"; return -1; }
  for (int m = 0; m < in->M; ++m)
    if (in->obs_edges[m] < 3 || in->obs_edges[m] > MAXE) { *err = "[lqr] obstacle edges must be in [3, 8]"; return -1; }
  for (int k = 0; k < in->K; ++k)
    if (in->body_edges[k] < 3 || in->body_edges[k] > MAXE) { *err = "[lqr] body edges must be in [3, 8]"; return -1; }
  if (in->batch == 0) return 0;
  if (!x || !in->params) { *err = "[lqr] null argument (input array)"; return -1; }
  if (!out->gains || !out->tube || !out->metrics || !out->worst || !out->flags) {
    *err = "[lqr] null argument (output array)";
    return -1;
  }
  return 0;
}

inline Batch batch_view(const htp_obca_batch& in, const double* x, const htp_obca_lqr_result& out) {
  return Batch{in.params, x, out.gains, out.tube, out.metrics, out.worst, out.flags, out.cost_to_go,
               out.linearisation};
}

}  // namespace lqr
}  // namespace htp
