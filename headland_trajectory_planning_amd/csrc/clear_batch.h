// Argument checks shared by the entries of the pose clearance and the turn selection: htp_pose_clearance_batch[_device]
// and htp_turn_select_batch[_device] (htp_clear.hip) and the test-only host build (clear_hostsim.cpp).  Nothing is
// dereferenced beyond the structs and the two host arrays of edge counts.
#pragma once
#include "../../include/htp.h"
#include "clear_core.h"

namespace htp {
namespace clr {

inline int check_args(const htp_clear_in* in, const htp_clear_result* out, const char** msg) {
  if (!in || !out) { *msg = "[clearance] null argument"; return -1; }
  if (in->batch < 0) { *msg = "[clearance] batch must be >= 0"; return -1; }
  if (in->cap_poses < 1) { *msg = "[clearance] cap_poses must be >= 1"; return -1; }
  if (in->stride < 3 || in->stride > 65536) { *msg = "[clearance] stride must be in 3..65536"; return -1; }
  const int cx = in->col_x, cy = in->col_y, cw = in->col_yaw;
  if (cx < 0 || cy < 0 || cw < 0 || cx >= in->stride || cy >= in->stride || cw >= in->stride || cx == cy || cx == cw ||
      cy == cw) {
    *msg = "[clearance] col_x, col_y and col_yaw must be distinct and below stride";
    return -1;
  }
  if (in->M < 1 || in->M > MAXM) { *msg = "[clearance] M must be in 1..16"; return -1; }
  if (in->K < 1 || in->K > MAXK) { *msg = "[clearance] K must be in 1..4"; return -1; }
  if (!in->obs_edges || !in->body_edges) { *msg = "[clearance] null argument (edge counts)"; return -1; }
  for (int m = 0; m < in->M; ++m)
    if (in->obs_edges[m] < 3 || in->obs_edges[m] > MAXE) { *msg = "[clearance] obs_edges must be in 3..8"; return -1; }
  for (int k = 0; k < in->K; ++k)
    if (in->body_edges[k] < 3 || in->body_edges[k] > MAXE) { *msg = "[clearance] body_edges must be in 3..8"; return -1; }
  if (in->n_scenes < 1) { *msg = "[clearance] n_scenes must be >= 1"; return -1; }
  if (!in->scene && in->n_scenes != in->batch) {
    *msg = "[clearance] without scene, n_scenes must equal batch";
    return -1;
  }
  if (in->substeps < 1 || in->substeps > MAXSUB) { *msg = "[clearance] substeps must be in 1..16"; return -1; }
  if (!(in->margin_tol >= 0.0) || hm::nonfinite(in->margin_tol)) {
    *msg = "[clearance] margin_tol must be finite and >= 0";
    return -1;
  }
  if (in->max_groups < 0) { *msg = "[clearance] max_groups must be >= 0"; return -1; }
  if ((int64_t)in->cap_poses * in->substeps * in->M * in->K >= ((int64_t)1 << 31)) {
    *msg = "[clearance] cap_poses * substeps * M * K must be below 2^31";
    return -1;
  }
  if (!in->poses || !in->n_poses || !in->obs_A || !in->obs_b || !in->body_G || !in->body_g) {
    *msg = "[clearance] null argument (input array)";
    return -1;
  }
  if (!out->status || !out->flags || !out->metrics || !out->worst) {
    *msg = "[clearance] null argument (output array)";
    return -1;
  }
  return 0;
}

inline int check_select(const htp_select_in* in, const htp_select_result* out, const char** msg) {
  if (!in || !out) { *msg = "[select] null argument"; return -1; }
  if (in->batch < 0) { *msg = "[select] batch must be >= 0"; return -1; }
  if (in->C < 1 || in->C > HTP_SEL_MAX_CAND) { *msg = "[select] C must be in 1..8"; return -1; }
  if (!(in->t_max >= 0.0)) { *msg = "[select] t_max must be >= 0"; return -1; }
  if (!in->spd_status || !in->spd_flags || !in->spd_summary || !in->clr_status || !in->clr_flags) {
    *msg = "[select] null argument (input array)";
    return -1;
  }
  if (!out->verdict || !out->winner || !out->score) { *msg = "[select] null argument (output array)"; return -1; }
  if (in->rows && (!in->count || !out->out_rows || !out->out_count || in->cap_rows < 1)) {
    *msg = "[select] rows need count, out_rows, out_count and cap_rows >= 1";
    return -1;
  }
  if (out->clearance && !in->clr_metrics) { *msg = "[select] clearance needs clr_metrics"; return -1; }
  return 0;
}

}  // namespace clr
}  // namespace htp
