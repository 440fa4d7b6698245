// TEST-ONLY host build of the swept-footprint envelope (envelope_core.h): a serial loop over the problems with
// the argument checks, structs and outputs of htp_obca_envelope_batch.  Lets CPU tests pin the device code's logic
// against a numpy restatement and a high-precision evaluation without a GPU, and the GPU tests compare bit for
// bit.
#include <cstdint>
#include <cstring>
#include <vector>

#define HTP_HD
#include "envelope_batch.h"

using namespace htp;

extern "C" int htp_hostsim_obca_envelope(const htp_obca_batch* in, const double* x, const double* frame,
                                         const htp_obca_envelope_opts* opts, htp_obca_envelope_result* out,
                                         char* err, int32_t err_len) {
  const char* e = nullptr;
  if (envelope::check_args(in, x, frame, opts, out, &e)) {
    if (err && err_len > 0) {
      std::strncpy(err, e, (size_t)err_len - 1);
      err[err_len - 1] = 0;
    }
    return -1;
  }
  if (in->batch == 0) return 0;
  envelope::Shape sh;
  envelope::make_shape(sh, *in, *opts);
  const envelope::Batch b = envelope::batch_view(*in, x, frame, *out);
  // exactly the doubles the kernel's LDS holds, so a sanitizer build sees an access beyond them
  std::vector<double> sl((size_t)envelope::L_FIXED), dl((size_t)envelope::lds_dyn_doubles(in->N, opts->W, opts->H));
  envelope::HostLane lane;
  for (int64_t p = 0; p < in->batch; ++p) envelope::run_problem(lane, sh, b, p, sl.data(), dl.data());
  return 0;
}
