// TEST-ONLY host build of the LQR rollout (ltrack_core.h): a serial loop over the problems with the argument checks,
// structs and outputs of htp_obca_ltrack_batch.  Lets CPU tests pin the device code's logic against a numpy
// restatement without a GPU, and the GPU tests compare bit for bit.
#include <cstdint>
#include <cstring>
#include <vector>

#define HTP_HD
#include "ltrack_batch.h"

using namespace htp;

extern "C" int htp_hostsim_obca_ltrack(const htp_obca_batch* in, const double* x, const htp_obca_ltrack_opts* opts,
                                       htp_obca_ltrack_result* out, char* err, int32_t err_len) {
  const char* e = nullptr;
  if (ltrack::check_args(in, x, opts, out, &e)) {
    if (err && err_len > 0) {
      std::strncpy(err, e, (size_t)err_len - 1);
      err[err_len - 1] = 0;
    }
    return -1;
  }
  if (in->batch == 0) return 0;
  ltrack::Shape sh;
  ltrack::make_shape(sh, *in, *opts);
  const ltrack::Batch b = ltrack::batch_view(*in, x, *opts, *out);
  // exactly the doubles the kernel's LDS holds, so a sanitizer build sees an access beyond them
  std::vector<double> sl((size_t)ltrack::L_FIXED), dl((size_t)ltrack::lds_stage_doubles(in->N));
  ltrack::HostLane lane;
  for (int64_t p = 0; p < in->batch; ++p) ltrack::run_problem(lane, sh, b, p, sl.data(), dl.data());
  return 0;
}
