// htp_obca_batch + htp_obca_envelope_opts/result -> the envelope core's launch shape and pointer view, with the
// argument checks of the C ABI; shared by the gfx950 library (htp_envelope.hip) and the test-only host build
// (envelope_hostsim.cpp).
#pragma once
#include "../../include/htp.h"
#include "envelope_core.h"

namespace htp {
namespace envelope {

static_assert(HTP_ENVELOPE_MAX_CELLS == 65536 && HTP_ENVELOPE_MAX_N == 480, "htp.h and the messages below");

// 0 = OK; -1 with *err set: nothing may be launched
inline int check_args(const htp_obca_batch* in, const double* x, const double* frame, const htp_obca_envelope_opts* o,
                      const htp_obca_envelope_result* out, const char** err) {
  if (!in || !o || !out) { *err = "[envelope] null argument"; return -1; }
  if (in->batch < 0) { *err = "[envelope] batch must be >= 0"; return -1; }
  if (in->N < 2) { *err = "[envelope] N must be >= 2"; return -1; }
  if (in->N > MAXN) { *err = "[envelope] N must be <= HTP_ENVELOPE_MAX_N (480)"; return -1; }
  if (in->M < 1 || in->M > MAXM) { *err = "[envelope] M must be in [1, 16]"; return -1; }
  if (in->K < 1 || in->K > MAXK) { *err = "[envelope] K must be in [1, 4]"; return -1; }
  if (o->substeps < 1 || o->substeps > audit::MAXSUB) {
    *err = "[envelope] substeps must be in [1, HTP_AUDIT_MAX_SUBSTEPS (16)]";
    return -1;
  }
  if (o->W < 0 || o->H < 0) { *err = "[envelope] W and H must be >= 0"; return -1; }
  if ((o->W == 0) != (o->H == 0)) { *err = "[envelope] W and H must both be 0 (extent only) or both be > 0"; return -1; }
  if (o->W % 32 != 0) { *err = "[envelope] W must be a multiple of 32"; return -1; }
  if ((int64_t)o->W * (int64_t)o->H > (int64_t)MAXCELLS) { *err = "[envelope] W * H must be <= 65536"; return -1; }
  if (o->W > 0 && (audit::nonfinite_(o->res) || !(o->res > 0.0))) { *err = "[envelope] res must be finite and > 0"; return -1; }
  if (!in->obs_edges || !in->body_edges) { *err = "[envelope] null argument (edge counts)"; return -1; }
  for (int m = 0; m < in->M; ++m)
    if (in->obs_edges[m] < 3 || in->obs_edges[m] > MAXE) { *err = "[envelope] obstacle edges must be in [3, 8]"; return -1; }
  for (int k = 0; k < in->K; ++k)
    if (in->body_edges[k] < 3 || in->body_edges[k] > MAXE) { *err = "[envelope] body edges must be in [3, 8]"; return -1; }
  if (in->batch == 0) return 0;
  if (!x || !frame || !in->body_G || !in->body_g || !in->params) { *err = "[envelope] null argument (input array)"; return -1; }
  if (!out->extent || !out->where || !out->flags || (o->W > 0 && !out->cells)) {
    *err = "[envelope] null argument (output array)";
    return -1;
  }
  return 0;
}

inline Batch batch_view(const htp_obca_batch& in, const double* x, const double* frame,
                        const htp_obca_envelope_result& out) {
  return Batch{in.body_G, in.body_g, in.params, x, frame, out.extent, out.where, out.extent_body, out.cells,
               out.bitmap, out.flags};
}

}  // namespace envelope
}  // namespace htp
