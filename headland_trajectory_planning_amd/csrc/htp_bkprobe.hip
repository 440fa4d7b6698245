// libhtp.so, TEST-ONLY surface: the solver's small dense factorizations (obca_core.h: unpivoted local LDL^T, the
// Bunch-Kaufman forms, chol3 / chol5) on caller blocks, one block per lane of 64-lane workgroups with the LDS laid
// out as the solver lays out its wave's (bk_probe.h).  tests/test_gpu_bk.py compares it with a high-precision
// reference and with the host builds of the same body.
#include <hip/hip_runtime.h>

#include <string>

#define HTP_HD __host__ __device__
#include "../../include/htp.h"
#include "wave_ctx.h"
#include "bk_probe.h"
#include "htp_ctx.h"

using namespace htp;

namespace {

template <int V, int N, int S>
__global__ __launch_bounds__(64) void bk_probe_kernel(int64_t count, int nrhs, int v_in, int v_out,
                                                      const double* __restrict__ K0, const double* __restrict__ rhs,
                                                      double* __restrict__ K, int32_t* __restrict__ ip,
                                                      int32_t* __restrict__ flags, double* __restrict__ x,
                                                      double* __restrict__ x2) {
  __shared__ double lds_[LDS_WAVE_DOUBLES];
  DevWave::ld* lds = (DevWave::ld*)lds_;
  const int64_t idx = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (idx < count)   // lanes past the block count stay inactive inside the wavefront
    bkp::probe_block<DevWave, V, N, S>(bkp::view(v_in, v_out, N, nrhs, idx, K0, rhs, K, ip, flags, x, x2), lds,
                                       (int)threadIdx.x);
}

}  // namespace

extern "C" int htp_bk_probe(htp_ctx* ctx, int32_t variant, int32_t n, int32_t lane_stride, int64_t count,
                            int32_t nrhs, const double* K0, const double* rhs, double* K, int32_t* ip,
                            int32_t* flags, double* x, double* x2, void* stream) {
  if (!ctx) return -1;
  if (count < 0 || nrhs < 0 || nrhs > bkp::MAXRHS) return fail(ctx, "bk probe: bad count or nrhs");
  if (count > 0 && (!K0 || !K || !ip || !flags || !x || !x2 || (nrhs > 0 && !rhs)))
    return fail(ctx, "bk probe: null array");
  if (count > (int64_t)1 << 24) return fail(ctx, "bk probe: too many blocks");
  hipError_t e = hipSuccess;
  const int vi = bkp::in_doubles(variant, n), vo = bkp::out_doubles(variant, n);
  const bool known = bkp::dispatch(variant, n, lane_stride, [&](auto tag) {
    using T = decltype(tag);
    if (count == 0) return;
    e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return;
    hipLaunchKernelGGL((bk_probe_kernel<T::V, T::N, T::S>), dim3((unsigned)((count + 63) / 64)), dim3(64), 0,
                       (hipStream_t)stream, count, (int)nrhs, vi, vo, K0, rhs, K, ip, flags, x, x2);
    e = hipGetLastError();
  });
  if (!known) return fail(ctx, "bk probe: no such (variant, n, lane_stride) instantiation");
  if (e != hipSuccess) return fail(ctx, std::string("bk probe: ") + hipGetErrorString(e));
  return 0;
}
