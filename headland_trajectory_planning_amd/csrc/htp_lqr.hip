// libhtp.so, time-varying LQR gains and error tube of solved OBCA trajectories (lqr_core.h): one problem per
// 64-lane wavefront (one wavefront per workgroup), the whole batch in one launch.  X, U and tau are the only part of
// a problem's x row that is read (coalesced 16-byte loads into LDS); 64 stages at a time are linearised one per
// lane into an LDS tile; the two recursions are serial over the stages with the lanes as the entries of the small
// products.  The gains of a chunk leave as one contiguous run from their LDS tile, and the forward pass reads the
// run back chunk by chunk (the LDS cannot hold the gains of 479 stages beside the trajectory).
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#define HTP_HD __host__ __device__
#include "../../include/htp.h"
#include "htp_ctx.h"
#include "lqr_batch.h"

using namespace htp;

namespace {

typedef double dbl2 __attribute__((ext_vector_type(2)));

struct LqrWave {
  static constexpr int width = 64;
  int lane;
  // the workgroup is one wavefront: LDS accesses are performed in program order, so a cross-lane
  // read-after-write only needs the compiler not to reorder them (wave_ctx.h DevWave::sync)
  __device__ __forceinline__ void sync() const {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  // global memory this wavefront stored is loaded again by other lanes of it: the stores are complete and the
  // vector L1 holds no older copy before the first such load
  __device__ __forceinline__ void gsync() const {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
    __builtin_amdgcn_wave_barrier();
  }
  __device__ __forceinline__ bool any(bool v) const { return __ballot(v ? 1 : 0) != 0ull; }
  // n doubles from HBM (8-byte aligned) into LDS: 16-byte loads over the aligned middle of the run
  __device__ __forceinline__ void load_run(double* dst, const double* src, int n, bool& bad) const {
    const int peel = (int)(((uintptr_t)src >> 3) & 1u) < n ? (int)(((uintptr_t)src >> 3) & 1u) : n;
    const int np = (n - peel) >> 1;
    const dbl2* s2 = (const dbl2*)(src + peel);
    for (int q = lane; q < np; q += 64) {
      const dbl2 v = s2[q];
      dst[peel + 2 * q] = v.x;
      dst[peel + 2 * q + 1] = v.y;
      bad = bad || audit::nonfinite_(v.x) || audit::nonfinite_(v.y);
    }
    if (lane == 0 && peel) { dst[0] = src[0]; bad = bad || audit::nonfinite_(src[0]); }
    if (lane == 1 && peel + 2 * np < n) { dst[n - 1] = src[n - 1]; bad = bad || audit::nonfinite_(src[n - 1]); }
  }
};

__global__ __launch_bounds__(64) void obca_lqr_kernel(lqr::Shape sh, lqr::Batch b, int batch) {
  __shared__ double sl[lqr::L_FIXED];
  extern __shared__ double dl[];
  const int64_t p = blockIdx.x;
  if (p >= batch) return;
  LqrWave c{(int)threadIdx.x};
  lqr::run_problem(c, sh, b, p, sl, dl);
}

int ensure_events(htp_ctx* ctx) {
  if (!ctx->lqr_ev.e0) HIPCHK(hipEventCreate(&ctx->lqr_ev.e0));
  if (!ctx->lqr_ev.e1) HIPCHK(hipEventCreate(&ctx->lqr_ev.e1));
  return 0;
}

int enqueue(htp_ctx* ctx, const lqr::Shape& sh, const lqr::Batch& b, int batch, hipStream_t s) {
  if (ensure_events(ctx)) return -1;
  const size_t dyn = sizeof(double) * (size_t)lqr::lds_stage_doubles(sh.N);
  HIPCHK(hipEventRecord(ctx->lqr_ev.e0, s));
  hipLaunchKernelGGL(obca_lqr_kernel, dim3((unsigned)batch), dim3(64), dyn, s, sh, b, batch);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ctx->lqr_ev.e1, s));
  return 0;
}

}  // namespace

extern "C" {

int htp_obca_lqr_batch_device(htp_ctx* ctx, const htp_obca_batch* in, const double* x, const htp_obca_lqr_opts* opts,
                              htp_obca_lqr_result* out, void* stream) {
  if (!ctx) return -1;
  const char* e = nullptr;
  if (lqr::check_args(in, x, opts, out, &e)) return fail(ctx, e);
  if (in->batch == 0) return 0;
  HIPCHK(hipSetDevice(ctx->device));
  lqr::Shape sh;
  lqr::make_shape(sh, *in, *opts);
  return enqueue(ctx, sh, lqr::batch_view(*in, x, *out), in->batch, (hipStream_t)stream);
}

int htp_obca_lqr_batch(htp_ctx* ctx, const htp_obca_batch* in, const double* x, const htp_obca_lqr_opts* opts,
                       htp_obca_lqr_result* out) {
  if (!ctx) return -1;
  const char* e = nullptr;
  if (lqr::check_args(in, x, opts, out, &e)) return fail(ctx, e);
  if (in->batch == 0) return 0;
  HIPCHK(hipSetDevice(ctx->device));
  lqr::Shape sh;
  lqr::make_shape(sh, *in, *opts);
  // only X, U and tau travel: the rows are packed to [X | U | tau] before the upload
  const size_t B = (size_t)in->batch, N = (size_t)in->N, nxu = 5 * N + 2 * (N - 1), nt = sh.topt ? N - 1 : 0;
  const size_t row = nxu + nt;
  std::vector<double> xp(B * row);
  for (size_t p = 0; p < B; ++p) {
    const double* src = x + p * (size_t)sh.stride;
    for (size_t q = 0; q < nxu; ++q) xp[p * row + q] = src[q];
    for (size_t q = 0; q < nt; ++q) xp[p * row + nxu + q] = src[(size_t)sh.oTAU + q];
  }
  sh.stride = (int64_t)row;
  sh.oTAU = (int)nxu;
  auto al = [](size_t v) { return (v + 255) & ~size_t(255); };
  size_t o = 0;
  const size_t o_x = o; o += al(8 * B * row);
  const size_t o_p = o; o += al(8 * B * NPARAM);
  const size_t o_g = o; o += al(8 * B * (N - 1) * lqr::NGAIN);
  const size_t o_t = o; o += al(8 * B * N * lqr::NTUBE);
  const size_t o_m = o; o += al(8 * B * lqr::NMET);
  const size_t o_w = o; o += al(8 * B);
  const size_t o_f = o; o += al(4 * B);
  const size_t o_c = o; o += al(8 * B * N * lqr::NCTG);
  const size_t o_l = o; o += al(8 * B * (N - 1) * lqr::NLIN);
  char* d = nullptr;
  HIPCHK(hipMalloc((void**)&d, o));
  int rc = 0;
  auto H2D = [&](size_t off, const void* src, size_t n) {
    if (rc == 0 && src && n && hipMemcpy(d + off, src, n, hipMemcpyHostToDevice) != hipSuccess) rc = fail(ctx, "lqr: upload");
  };
  auto D2H = [&](void* dst, size_t off, size_t n) {
    if (rc == 0 && dst && n && hipMemcpy(dst, d + off, n, hipMemcpyDeviceToHost) != hipSuccess)
      rc = fail(ctx, "lqr: download");
  };
  H2D(o_x, xp.data(), 8 * B * row);
  H2D(o_p, in->params, 8 * B * NPARAM);
  // a flagged problem leaves rows unwritten: the caller's arrays go up first, so that what comes back differs from
  // them only where the kernel wrote
  H2D(o_g, out->gains, 8 * B * (N - 1) * lqr::NGAIN);
  H2D(o_t, out->tube, 8 * B * N * lqr::NTUBE);
  H2D(o_w, out->worst, 8 * B);
  H2D(o_c, out->cost_to_go, 8 * B * N * lqr::NCTG);
  H2D(o_l, out->linearisation, 8 * B * (N - 1) * lqr::NLIN);
  const lqr::Batch b{(const double*)(d + o_p), (const double*)(d + o_x), (double*)(d + o_g), (double*)(d + o_t),
                     (double*)(d + o_m), (int32_t*)(d + o_w), (int32_t*)(d + o_f),
                     out->cost_to_go ? (double*)(d + o_c) : nullptr,
                     out->linearisation ? (double*)(d + o_l) : nullptr};
  if (rc == 0) rc = enqueue(ctx, sh, b, in->batch, nullptr);
  if (rc == 0) {
    hipError_t er = hipDeviceSynchronize();
    if (er != hipSuccess) rc = fail(ctx, std::string("lqr kernel: ") + hipGetErrorString(er));
  }
  D2H(out->gains, o_g, 8 * B * (N - 1) * lqr::NGAIN);
  D2H(out->tube, o_t, 8 * B * N * lqr::NTUBE);
  D2H(out->metrics, o_m, 8 * B * lqr::NMET);
  D2H(out->worst, o_w, 8 * B);
  D2H(out->flags, o_f, 4 * B);
  D2H(out->cost_to_go, o_c, 8 * B * N * lqr::NCTG);
  D2H(out->linearisation, o_l, 8 * B * (N - 1) * lqr::NLIN);
  (void)hipFree(d);
  return rc;
}

double htp_obca_lqr_last_ms(htp_ctx* ctx) {
  if (!ctx || !ctx->lqr_ev.e1) return 0.0;
  float ms = 0.f;
  if (hipEventSynchronize(ctx->lqr_ev.e1) != hipSuccess) return 0.0;
  if (hipEventElapsedTime(&ms, ctx->lqr_ev.e0, ctx->lqr_ev.e1) != hipSuccess) return 0.0;
  return (double)ms;
}

}  // extern "C"
