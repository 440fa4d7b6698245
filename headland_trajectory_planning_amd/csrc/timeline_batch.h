// htp_obca_batch + htp_obca_timeline_opts/result -> the timeline core's launch shape and pointer view, with
// the argument checks of the C ABI; shared by the gfx950 library (htp_timeline.hip) and the test-only host
// build (timeline_hostsim.cpp).
#pragma once
#include "../../include/htp.h"
#include "timeline_core.h"

namespace htp {
namespace timeline {

static_assert(HTP_TIMELINE_NCOL == 10, "htp.h timeline columns");

// 0 = OK; -1 with *err set: nothing may be launched
inline int check_args(const htp_obca_batch* in, const double* x, const htp_obca_timeline_opts* o,
                      const htp_obca_timeline_result* out, const char** err) {
  if (!in || !o || !out) { *err = "[timeline] null argument"; return -1; }
  if (in->batch < 0) { *err = "[timeline] batch must be >= 0"; return -1; }
  if (in->N < 2) { *err = "[timeline] N must be >= 2"; return -1; }
  if (in->N > MAXN) { *err = "[timeline] N must be <= HTP_TIMELINE_MAX_N (480)"; return -1; }
  if (in->M < 1 || in->M > MAXM) { *err = "[timeline] M must be in [1, 16]"; return -1; }
  if (in->K < 1 || in->K > MAXK) { *err = "[timeline] K must be in [1, 4]"; return -1; }
  if (audit::nonfinite_(o->dt) || !(o->dt > 0.0)) { *err = "[timeline] dt must be finite and > 0"; return -1; }
  if (o->cap < 2) { *err = "[timeline] cap must be >= 2"; return -1; }
  if (!in->obs_edges || !in->body_edges) { *err = "[timeline] null argument (edge counts)"; return -1; }
  for (int m = 0; m < in->M; ++m)
    if (in->obs_edges[m] < 3 || in->obs_edges[m] > MAXE) { *err = "[timeline] obstacle edges must be in [3, 8]"; return -1; }
  for (int k = 0; k < in->K; ++k)
    if (in->body_edges[k] < 3 || in->body_edges[k] > MAXE) { *err = "[timeline] body edges must be in [3, 8]"; return -1; }
  if (in->batch == 0) return 0;
  if (!x || !in->params) { *err = "[timeline] null argument (input array)"; return -1; }
  if (!out->rows || !out->count || !out->flags) { *err = "[timeline] null argument (output array)"; return -1; }
  return 0;
}

inline Batch batch_view(const htp_obca_batch& in, const double* x, const htp_obca_timeline_result& out) {
  return Batch{in.params, x, out.rows, out.stage, out.count, out.flags, out.duration};
}

}  // namespace timeline
}  // namespace htp
