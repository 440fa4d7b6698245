// libhtp.so, uniform-time sampling of solved OBCA trajectories (timeline_core.h): one problem per 64-lane
// wavefront (one wavefront per workgroup), the whole batch in one launch.  X, U and tau are the only part of
// a problem's x row that is read (coalesced 16-byte loads into LDS); the node times and arc lengths are built
// in LDS; the rows are produced 64 at a time, one per lane, into an LDS tile, and the tile leaves as one
// contiguous run of 16-byte stores (no lane stores its own ten doubles at an 80-byte stride).
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#define HTP_HD __host__ __device__
#include "../../include/htp.h"
#include "htp_ctx.h"
#include "timeline_batch.h"

using namespace htp;

namespace {

typedef double dbl2 __attribute__((ext_vector_type(2)));

struct TimelineWave {
  static constexpr int width = 64;
  int lane;
  // the workgroup is one wavefront: LDS accesses are performed in program order, so a cross-lane
  // read-after-write only needs the compiler not to reorder them (wave_ctx.h DevWave::sync)
  __device__ __forceinline__ void sync() const {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
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
  // load_run reversed: n doubles from LDS to HBM (8-byte aligned), 16-byte stores over the aligned middle;
  // every store lies inside dst[0 .. n)
  __device__ __forceinline__ void store_run(double* dst, const double* src, int n) const {
    const int peel = (int)(((uintptr_t)dst >> 3) & 1u) < n ? (int)(((uintptr_t)dst >> 3) & 1u) : n;
    const int np = (n - peel) >> 1;
    dbl2* d2 = (dbl2*)(dst + peel);
    for (int q = lane; q < np; q += 64) {
      dbl2 v;
      v.x = src[peel + 2 * q];
      v.y = src[peel + 2 * q + 1];
      d2[q] = v;
    }
    if (lane == 0 && peel) dst[0] = src[0];
    if (lane == 1 && peel + 2 * np < n) dst[n - 1] = src[n - 1];
  }
};

__global__ __launch_bounds__(64) void obca_timeline_kernel(timeline::Shape sh, timeline::Batch b, int batch) {
  __shared__ double tile[timeline::L_FIXED];
  extern __shared__ double dl[];
  const int64_t p = blockIdx.x;
  if (p >= batch) return;
  TimelineWave c{(int)threadIdx.x};
  timeline::run_problem(c, sh, b, p, tile, dl);
}

int ensure_events(htp_ctx* ctx) {
  if (!ctx->timeline_ev.e0) HIPCHK(hipEventCreate(&ctx->timeline_ev.e0));
  if (!ctx->timeline_ev.e1) HIPCHK(hipEventCreate(&ctx->timeline_ev.e1));
  return 0;
}

int enqueue(htp_ctx* ctx, const timeline::Shape& sh, const timeline::Batch& b, int batch, hipStream_t s) {
  if (ensure_events(ctx)) return -1;
  const size_t dyn = sizeof(double) * (size_t)timeline::lds_stage_doubles(sh.N);
  HIPCHK(hipEventRecord(ctx->timeline_ev.e0, s));
  hipLaunchKernelGGL(obca_timeline_kernel, dim3((unsigned)batch), dim3(64), dyn, s, sh, b, batch);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ctx->timeline_ev.e1, s));
  return 0;
}

}  // namespace

extern "C" {

int htp_obca_timeline_batch_device(htp_ctx* ctx, const htp_obca_batch* in, const double* x,
                                   const htp_obca_timeline_opts* opts, htp_obca_timeline_result* out, void* stream) {
  if (!ctx) return -1;
  const char* e = nullptr;
  if (timeline::check_args(in, x, opts, out, &e)) return fail(ctx, e);
  if (in->batch == 0) return 0;
  HIPCHK(hipSetDevice(ctx->device));
  timeline::Shape sh;
  timeline::make_shape(sh, *in, *opts);
  return enqueue(ctx, sh, timeline::batch_view(*in, x, *out), in->batch, (hipStream_t)stream);
}

int htp_obca_timeline_batch(htp_ctx* ctx, const htp_obca_batch* in, const double* x,
                            const htp_obca_timeline_opts* opts, htp_obca_timeline_result* out) {
  if (!ctx) return -1;
  const char* e = nullptr;
  if (timeline::check_args(in, x, opts, out, &e)) return fail(ctx, e);
  if (in->batch == 0) return 0;
  HIPCHK(hipSetDevice(ctx->device));
  timeline::Shape sh;
  timeline::make_shape(sh, *in, *opts);
  // only X, U and tau travel: the rows are packed to [X | U | tau] before the upload
  const size_t B = (size_t)in->batch, N = (size_t)in->N, nxu = 5 * N + 2 * (N - 1), nt = sh.topt ? N - 1 : 0;
  const size_t row = nxu + nt, cap = (size_t)opts->cap;
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
  const size_t o_r = o; o += al(8 * B * cap * timeline::NCOL);
  const size_t o_s = o; o += al(4 * B * cap);
  const size_t o_c = o; o += al(4 * B);
  const size_t o_f = o; o += al(4 * B);
  const size_t o_d = o; o += al(8 * B);
  char* d = nullptr;
  HIPCHK(hipMalloc((void**)&d, o));
  int rc = 0;
  auto H2D = [&](size_t off, const void* src, size_t n) {
    if (rc == 0 && n && hipMemcpy(d + off, src, n, hipMemcpyHostToDevice) != hipSuccess) rc = fail(ctx, "timeline: upload");
  };
  auto D2H = [&](void* dst, size_t off, size_t n) {
    if (rc == 0 && dst && n && hipMemcpy(dst, d + off, n, hipMemcpyDeviceToHost) != hipSuccess)
      rc = fail(ctx, "timeline: download");
  };
  H2D(o_x, xp.data(), 8 * B * row);
  H2D(o_p, in->params, 8 * B * NPARAM);
  const timeline::Batch b{(const double*)(d + o_p), (const double*)(d + o_x), (double*)(d + o_r),
                          out->stage ? (int32_t*)(d + o_s) : nullptr, (int32_t*)(d + o_c), (int32_t*)(d + o_f),
                          out->duration ? (double*)(d + o_d) : nullptr};
  if (rc == 0) rc = enqueue(ctx, sh, b, in->batch, nullptr);
  if (rc == 0) {
    hipError_t er = hipDeviceSynchronize();
    if (er != hipSuccess) rc = fail(ctx, std::string("timeline kernel: ") + hipGetErrorString(er));
  }
  D2H(out->count, o_c, 4 * B);
  D2H(out->flags, o_f, 4 * B);
  D2H(out->duration, o_d, 8 * B);
  // the caller's rows at or beyond min(count, cap) stay as they are: only the written rows are copied over
  std::vector<double> rows(rc == 0 ? B * cap * timeline::NCOL : 0);
  std::vector<int32_t> stage(rc == 0 && out->stage ? B * cap : 0);
  D2H(rows.data(), o_r, 8 * rows.size());
  D2H(stage.data(), o_s, 4 * stage.size());
  if (rc == 0)
    for (size_t p = 0; p < B; ++p) {
      const size_t n = (size_t)out->count[p] < cap ? (size_t)out->count[p] : cap;
      for (size_t q = 0; q < n * timeline::NCOL; ++q) out->rows[p * cap * timeline::NCOL + q] = rows[p * cap * timeline::NCOL + q];
      if (out->stage)
        for (size_t q = 0; q < n; ++q) out->stage[p * cap + q] = stage[p * cap + q];
    }
  (void)hipFree(d);
  return rc;
}

double htp_obca_timeline_last_ms(htp_ctx* ctx) {
  if (!ctx || !ctx->timeline_ev.e1) return 0.0;
  float ms = 0.f;
  if (hipEventSynchronize(ctx->timeline_ev.e1) != hipSuccess) return 0.0;
  if (hipEventElapsedTime(&ms, ctx->timeline_ev.e0, ctx->timeline_ev.e1) != hipSuccess) return 0.0;
  return (double)ms;
}

}  // extern "C"
