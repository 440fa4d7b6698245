// TEST-ONLY host build of the trajectory audit (audit_core.h): a serial loop over the problems with the
// argument checks, structs and outputs of htp_obca_audit_batch.  Lets CPU tests pin the device code's logic
// against a high-precision evaluation and the oracle without a GPU, and the GPU tests compare bit for bit.
#include <cstdint>
#include <cstring>
#include <vector>

#define HTP_HD
#include "audit_batch.h"

using namespace htp;

extern "C" int htp_hostsim_obca_audit(const htp_obca_batch* in, const double* x, const htp_obca_audit_opts* opts,
                                      htp_obca_audit_result* out, char* err, int32_t err_len) {
  const char* e = nullptr;
  if (audit::check_args(in, x, opts, out, &e)) {
    if (err && err_len > 0) {
      std::strncpy(err, e, (size_t)err_len - 1);
      err[err_len - 1] = 0;
    }
    return -1;
  }
  if (in->batch == 0) return 0;
  audit::Shape sh;
  audit::make_shape(sh, *in, *opts);
  const audit::Batch b = audit::batch_view(*in, x, *out);
  std::vector<double> sl((size_t)audit::L_FIXED), dl((size_t)audit::lds_stage_doubles(in->N));
  audit::HostLane lane;
  for (int64_t p = 0; p < in->batch; ++p) audit::run_problem(lane, sh, b, p, sl.data(), dl.data());
  return 0;
}
