// Argument checks shared by the entries of the speed profile: htp_speed_profile_batch[_device] (htp_speed.hip) and the
// test-only host build (speed_hostsim.cpp).  Nothing is dereferenced beyond the two structs.
#pragma once
#include "../../include/htp.h"
#include "speed_core.h"

namespace htp {
namespace spd {

inline int check_args(const htp_speed_in* in, const htp_speed_result* out, const char** msg) {
  if (!in || !out) { *msg = "[speed] null argument"; return -1; }
  if (in->batch < 0) { *msg = "[speed] batch must be >= 0"; return -1; }
  if (in->cap_path < 2) { *msg = "[speed] cap_path must be >= 2"; return -1; }
  if (in->max_groups < 0) { *msg = "[speed] max_groups must be >= 0"; return -1; }
  if (hm::nonfinite(in->dt) || in->dt < 0.0) { *msg = "[speed] dt must be finite and >= 0"; return -1; }
  if (!in->path || !in->n_path || !in->limits) { *msg = "[speed] null argument (input array)"; return -1; }
  if (!out->status || !out->flags || !out->summary || !out->count) {
    *msg = "[speed] null argument (output array)";
    return -1;
  }
  if (in->dt > 0.0 && in->cap_rows < 2) { *msg = "[speed] cap_rows must be >= 2 when dt > 0"; return -1; }
  if (in->dt > 0.0 && !out->rows) { *msg = "[speed] rows is required when dt > 0"; return -1; }
  return 0;
}

}  // namespace spd
}  // namespace htp
