// libhtp.so, closed-loop rollout of solved OBCA trajectories under their LQR gains (ltrack_core.h): the mapping of
// htp_track.hip continued -- one problem per 64-lane wavefront (one wavefront per workgroup), one lane per scenario,
// the whole batch in one launch.  X, U and tau come into LDS by coalesced 16-byte loads; the gains stay in global
// memory: one coalesced pass checks them, and the lane that builds a tick's reference row loads that tick's K_i
// (neighbouring ticks share a stage, hence cache lines) and leaves the rotated law row beside it in the LDS tile,
// which the serial tick loop reads by a broadcast address.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#define HTP_HD __host__ __device__
#include "../../include/htp.h"
#include "htp_ctx.h"
#include "ltrack_batch.h"

using namespace htp;

namespace {

typedef double dbl2 __attribute__((ext_vector_type(2)));

struct LtrackWave {
  static constexpr int width = 64;
  int lane;
  // the workgroup is one wavefront: LDS accesses are performed in program order, so a cross-lane
  // read-after-write only needs the compiler not to reorder them (wave_ctx.h DevWave::sync)
  __device__ __forceinline__ void sync() const {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  __device__ __forceinline__ double minv(double v) const {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = audit::dmin_(v, __shfl_xor(v, o, 64));
    return v;
  }
  // the operands are never NaN (ltrack::err_term), so the butterfly's order does not show
  __device__ __forceinline__ double maxv(double v) const {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = audit::dmax_(v, __shfl_xor(v, o, 64));
    return v;
  }
  __device__ __forceinline__ bool any(bool v) const { return __ballot(v ? 1 : 0) != 0ull; }
  __device__ __forceinline__ int count(bool v) const { return __popcll(__ballot(v ? 1 : 0)); }
  // minimum with its index carried along; equal values keep the lower index, so every lane ends with the
  // same pair whatever the butterfly's order
  __device__ __forceinline__ void min_key(double& v, int& i) const {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double ov = __shfl_xor(v, o, 64);
      const int oi = __shfl_xor(i, o, 64);
      if (ov < v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
  }
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

__global__ __launch_bounds__(64) void obca_ltrack_kernel(ltrack::Shape sh, ltrack::Batch b, int batch) {
  __shared__ double sl[ltrack::L_FIXED];
  extern __shared__ double dl[];
  const int64_t p = blockIdx.x;
  if (p >= batch) return;
  LtrackWave c{(int)threadIdx.x};
  ltrack::run_problem(c, sh, b, p, sl, dl);
}

int ensure_events(htp_ctx* ctx) {
  if (!ctx->ltrack_ev.e0) HIPCHK(hipEventCreate(&ctx->ltrack_ev.e0));
  if (!ctx->ltrack_ev.e1) HIPCHK(hipEventCreate(&ctx->ltrack_ev.e1));
  return 0;
}

int enqueue(htp_ctx* ctx, const ltrack::Shape& sh, const ltrack::Batch& b, int batch, hipStream_t s) {
  if (ensure_events(ctx)) return -1;
  const size_t dyn = sizeof(double) * (size_t)ltrack::lds_stage_doubles(sh.N);
  HIPCHK(hipEventRecord(ctx->ltrack_ev.e0, s));
  hipLaunchKernelGGL(obca_ltrack_kernel, dim3((unsigned)batch), dim3(64), dyn, s, sh, b, batch);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ctx->ltrack_ev.e1, s));
  return 0;
}

}  // namespace

extern "C" {

int htp_obca_ltrack_batch_device(htp_ctx* ctx, const htp_obca_batch* in, const double* x,
                                 const htp_obca_ltrack_opts* opts, htp_obca_ltrack_result* out, void* stream) {
  if (!ctx) return -1;
  const char* e = nullptr;
  if (ltrack::check_args(in, x, opts, out, &e)) return fail(ctx, e);
  if (in->batch == 0) return 0;
  HIPCHK(hipSetDevice(ctx->device));
  ltrack::Shape sh;
  ltrack::make_shape(sh, *in, *opts);
  return enqueue(ctx, sh, ltrack::batch_view(*in, x, *opts, *out), in->batch, (hipStream_t)stream);
}

int htp_obca_ltrack_batch(htp_ctx* ctx, const htp_obca_batch* in, const double* x, const htp_obca_ltrack_opts* opts,
                          htp_obca_ltrack_result* out) {
  if (!ctx) return -1;
  const char* e = nullptr;
  if (ltrack::check_args(in, x, opts, out, &e)) return fail(ctx, e);
  if (in->batch == 0) return 0;
  HIPCHK(hipSetDevice(ctx->device));
  ltrack::Shape sh;
  ltrack::make_shape(sh, *in, *opts);
  // only X, U and tau travel: the rows are packed to [X | U | tau] before the upload
  const size_t B = (size_t)in->batch, N = (size_t)in->N, nxu = 5 * N + 2 * (N - 1), nt = sh.topt ? N - 1 : 0;
  const size_t row = nxu + nt, R = (size_t)opts->R, MT = (size_t)opts->max_ticks;
  std::vector<double> xp(B * row);
  for (size_t p = 0; p < B; ++p) {
    const double* src = x + p * (size_t)sh.stride;
    for (size_t q = 0; q < nxu; ++q) xp[p * row + q] = src[q];
    for (size_t q = 0; q < nt; ++q) xp[p * row + nxu + q] = src[(size_t)sh.oTAU + q];
  }
  sh.stride = (int64_t)row;
  sh.oTAU = (int)nxu;
  auto al = [](size_t v) { return (v + 255) & ~size_t(255); };
  const size_t TEo = (size_t)sh.TEo, TEb = (size_t)sh.TEb, NG = (size_t)ltrack::NGAIN * (N - 1);
  size_t o = 0;
  const size_t o_x = o; o += al(8 * B * row);
  const size_t o_A = o; o += al(16 * B * TEo);
  const size_t o_b = o; o += al(8 * B * TEo);
  const size_t o_G = o; o += al(16 * B * TEb);
  const size_t o_g = o; o += al(8 * B * TEb);
  const size_t o_p = o; o += al(8 * B * NPARAM);
  const size_t o_sc = o; o += al(8 * R * ltrack::NDIST);
  const size_t o_k = o; o += al(8 * B * NG);
  const size_t o_m = o; o += al(8 * B * R * ltrack::NMET);
  const size_t o_w = o; o += al(12 * B * R);
  const size_t o_f = o; o += al(4 * B * R);
  const size_t o_t = o; o += al(4 * B * ltrack::NFLAG);
  const size_t o_ws = o; o += al(4 * B);
  const size_t o_tk = o; o += al(8 * B * MT);
  const size_t o_rf = o; o += al(8 * B * MT * ltrack::NREF);
  const size_t o_te = o; o += al(8 * B * MT * ltrack::NERR);
  char* d = nullptr;
  HIPCHK(hipMalloc((void**)&d, o));
  int rc = 0;
  auto H2D = [&](size_t off, const void* src, size_t n) {
    if (rc == 0 && src && n && hipMemcpy(d + off, src, n, hipMemcpyHostToDevice) != hipSuccess) rc = fail(ctx, "ltrack: upload");
  };
  auto D2H = [&](void* dst, size_t off, size_t n) {
    if (rc == 0 && dst && n && hipMemcpy(dst, d + off, n, hipMemcpyDeviceToHost) != hipSuccess)
      rc = fail(ctx, "ltrack: download");
  };
  H2D(o_x, xp.data(), 8 * B * row);
  H2D(o_A, in->obs_A, 16 * B * TEo);
  H2D(o_b, in->obs_b, 8 * B * TEo);
  H2D(o_G, in->body_G, 16 * B * TEb);
  H2D(o_g, in->body_g, 8 * B * TEb);
  H2D(o_p, in->params, 8 * B * NPARAM);
  H2D(o_sc, opts->scenarios, 8 * R * ltrack::NDIST);
  H2D(o_k, opts->gains, 8 * B * NG);
  // the three per-tick outputs are written up to each problem's own pose count: the caller's arrays go up first,
  // so that what comes back differs from them only where the kernel wrote
  H2D(o_tk, out->tick_clearance, 8 * B * MT);
  H2D(o_rf, out->reference, 8 * B * MT * ltrack::NREF);
  H2D(o_te, out->tick_error, 8 * B * MT * ltrack::NERR);
  const ltrack::Batch b{track::Batch{(const double*)(d + o_A), (const double*)(d + o_b), (const double*)(d + o_G),
                                     (const double*)(d + o_g), (const double*)(d + o_p), (const double*)(d + o_x),
                                     (const double*)(d + o_sc), (double*)(d + o_m), (int32_t*)(d + o_w),
                                     (int32_t*)(d + o_f), (int32_t*)(d + o_t), (int32_t*)(d + o_ws),
                                     out->tick_clearance ? (double*)(d + o_tk) : nullptr,
                                     out->reference ? (double*)(d + o_rf) : nullptr},
                        (const double*)(d + o_k), out->tick_error ? (double*)(d + o_te) : nullptr};
  if (rc == 0) rc = enqueue(ctx, sh, b, in->batch, nullptr);
  if (rc == 0) {
    hipError_t er = hipDeviceSynchronize();
    if (er != hipSuccess) rc = fail(ctx, std::string("ltrack kernel: ") + hipGetErrorString(er));
  }
  D2H(out->metrics, o_m, 8 * B * R * ltrack::NMET);
  D2H(out->worst, o_w, 12 * B * R);
  D2H(out->flags, o_f, 4 * B * R);
  D2H(out->tally, o_t, 4 * B * ltrack::NFLAG);
  D2H(out->worst_scenario, o_ws, 4 * B);
  D2H(out->tick_clearance, o_tk, 8 * B * MT);
  D2H(out->reference, o_rf, 8 * B * MT * ltrack::NREF);
  D2H(out->tick_error, o_te, 8 * B * MT * ltrack::NERR);
  (void)hipFree(d);
  return rc;
}

double htp_obca_ltrack_last_ms(htp_ctx* ctx) {
  if (!ctx || !ctx->ltrack_ev.e1) return 0.0;
  float ms = 0.f;
  if (hipEventSynchronize(ctx->ltrack_ev.e1) != hipSuccess) return 0.0;
  if (hipEventElapsedTime(&ms, ctx->ltrack_ev.e0, ctx->ltrack_ev.e1) != hipSuccess) return 0.0;
  return (double)ms;
}

}  // extern "C"
