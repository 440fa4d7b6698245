// TEST-ONLY host build of the pose clearance and the turn selection (clear_core.h, serial single-lane context), same
// structs and argument checks as htp_pose_clearance_batch and htp_turn_select_batch.  The product never loads it.
#include <cstdint>
#include <cstdio>
#include <vector>

#define HTP_HD
#include "clear_batch.h"

namespace {

int refuse(const char* e, char* msg, int32_t msg_len) {
  if (msg && msg_len > 0) std::snprintf(msg, (size_t)msg_len, "%s", e);
  return -1;
}

}  // namespace

extern "C" int htp_hostsim_pose_clearance(const htp_clear_in* in, htp_clear_result* out, char* msg, int32_t msg_len) {
  using namespace htp;
  const char* e = nullptr;
  if (clr::check_args(in, out, &e)) return refuse(e, msg, msg_len);
  clr::Shape sh;
  clr::make_shape(sh, *in);
  const clr::Batch b = clr::batch_view(*in, *out);
  // on the heap, exactly sized: the sanitizer build sees an overrun of what stands for the kernel's LDS
  std::vector<double> sl(clr::L_TOTAL);
  clr::HostLane c;
  for (int64_t p = 0; p < in->batch; ++p) clr::run_path(c, sh, b, p, sl.data());
  return 0;
}

extern "C" int htp_hostsim_turn_select(const htp_select_in* in, htp_select_result* out, char* msg, int32_t msg_len) {
  using namespace htp;
  const char* e = nullptr;
  if (clr::check_select(in, out, &e)) return refuse(e, msg, msg_len);
  clr::HostLane c;
  for (int64_t b = 0; b < in->batch; ++b) clr::select_problem(c, *in, *out, b);
  return 0;
}
