// TEST-ONLY host build of the trajectory timeline (timeline_core.h): a serial loop over the problems with the
// argument checks, structs and outputs of htp_obca_timeline_batch.  Lets CPU tests pin the device code's logic
// against a numpy restatement and a high-precision evaluation without a GPU, and the GPU tests compare bit for
// bit.
#include <cstdint>
#include <cstring>
#include <vector>

#define HTP_HD
#include "timeline_batch.h"

using namespace htp;

extern "C" int htp_hostsim_obca_timeline(const htp_obca_batch* in, const double* x,
                                         const htp_obca_timeline_opts* opts, htp_obca_timeline_result* out,
                                         char* err, int32_t err_len) {
  const char* e = nullptr;
  if (timeline::check_args(in, x, opts, out, &e)) {
    if (err && err_len > 0) {
      std::strncpy(err, e, (size_t)err_len - 1);
      err[err_len - 1] = 0;
    }
    return -1;
  }
  if (in->batch == 0) return 0;
  timeline::Shape sh;
  timeline::make_shape(sh, *in, *opts);
  const timeline::Batch b = timeline::batch_view(*in, x, *out);
  // exactly the doubles the kernel's LDS holds, so a sanitizer build sees an access beyond them
  std::vector<double> tile((size_t)timeline::L_FIXED), dl((size_t)timeline::lds_stage_doubles(in->N));
  timeline::HostLane lane;
  for (int64_t p = 0; p < in->batch; ++p) timeline::run_problem(lane, sh, b, p, tile.data(), dl.data());
  return 0;
}
