// libhtp.so, swept-footprint envelope of solved OBCA trajectories (envelope_core.h): one problem per 64-lane
// wavefront (one wavefront per workgroup), the whole batch in one launch.  X, U and tau are the only part of a
// problem's x row that is read (coalesced 16-byte loads into LDS); the body edges, a chunk of poses with their
// bounding boxes and two bitmaps (the current body's and the union's) sit beside them; the union leaves as one
// contiguous run of 16-byte stores.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#define HTP_HD __host__ __device__
#include "../../include/htp.h"
#include "htp_ctx.h"
#include "envelope_batch.h"

using namespace htp;

namespace {

typedef double dbl2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct EnvelopeWave {
  static constexpr int width = 64;
  int lane;
  // the workgroup is one wavefront: LDS accesses are performed in program order, so a cross-lane
  // read-after-write only needs the compiler not to reorder them (wave_ctx.h DevWave::sync)
  __device__ __forceinline__ void sync() const {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  __device__ __forceinline__ bool any(bool v) const { return __ballot(v ? 1 : 0) != 0ull; }
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
  // a value that is the same in every lane, moved to scalar registers
  __device__ __forceinline__ double uniform(double v) const {
    uint64_t b;
    __builtin_memcpy(&b, &v, 8);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)b), hi = __builtin_amdgcn_readfirstlane((uint32_t)(b >> 32));
    b = ((uint64_t)hi << 32) | lo;
    __builtin_memcpy(&v, &b, 8);
    return v;
  }
  __device__ __forceinline__ int sumi(int v) const {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
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
  // n words from LDS to HBM (4-byte aligned): 16-byte stores over the aligned middle of the run, 4-byte stores
  // for the words in front of and behind it; every store lies inside dst[0 .. n)
  __device__ __forceinline__ void store_words(uint32_t* dst, const uint32_t* src, int n) const {
    const int lead = (int)((4u - (((uintptr_t)dst >> 2) & 3u)) & 3u);
    const int peel = lead < n ? lead : n;
    const int nq = (n - peel) >> 2;
    u32x4* d4 = (u32x4*)(dst + peel);
    for (int q = lane; q < nq; q += 64) {
      u32x4 v;
      v.x = src[peel + 4 * q];
      v.y = src[peel + 4 * q + 1];
      v.z = src[peel + 4 * q + 2];
      v.w = src[peel + 4 * q + 3];
      d4[q] = v;
    }
    if (lane < peel) dst[lane] = src[lane];
    const int done = peel + 4 * nq;
    if (lane < n - done) dst[done + lane] = src[done + lane];
  }
};

__global__ __launch_bounds__(64) void obca_envelope_kernel(envelope::Shape sh, envelope::Batch b, int batch) {
  __shared__ __attribute__((aligned(16))) double sl[envelope::L_FIXED];
  extern __shared__ __attribute__((aligned(16))) double dl[];
  const int64_t p = blockIdx.x;
  if (p >= batch) return;
  EnvelopeWave c{(int)threadIdx.x};
  envelope::run_problem(c, sh, b, p, sl, dl);
}

int ensure_events(htp_ctx* ctx) {
  if (!ctx->envelope_ev.e0) HIPCHK(hipEventCreate(&ctx->envelope_ev.e0));
  if (!ctx->envelope_ev.e1) HIPCHK(hipEventCreate(&ctx->envelope_ev.e1));
  return 0;
}

int enqueue(htp_ctx* ctx, const envelope::Shape& sh, const envelope::Batch& b, int batch, hipStream_t s) {
  if (ensure_events(ctx)) return -1;
  const size_t dyn = sizeof(double) * (size_t)envelope::lds_dyn_doubles(sh.N, sh.W, sh.H);
  HIPCHK(hipEventRecord(ctx->envelope_ev.e0, s));
  hipLaunchKernelGGL(obca_envelope_kernel, dim3((unsigned)batch), dim3(64), dyn, s, sh, b, batch);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ctx->envelope_ev.e1, s));
  return 0;
}

}  // namespace

extern "C" {

int htp_obca_envelope_batch_device(htp_ctx* ctx, const htp_obca_batch* in, const double* x, const double* frame,
                                   const htp_obca_envelope_opts* opts, htp_obca_envelope_result* out, void* stream) {
  if (!ctx) return -1;
  const char* e = nullptr;
  if (envelope::check_args(in, x, frame, opts, out, &e)) return fail(ctx, e);
  if (in->batch == 0) return 0;
  HIPCHK(hipSetDevice(ctx->device));
  envelope::Shape sh;
  envelope::make_shape(sh, *in, *opts);
  return enqueue(ctx, sh, envelope::batch_view(*in, x, frame, *out), in->batch, (hipStream_t)stream);
}

int htp_obca_envelope_batch(htp_ctx* ctx, const htp_obca_batch* in, const double* x, const double* frame,
                            const htp_obca_envelope_opts* opts, htp_obca_envelope_result* out) {
  if (!ctx) return -1;
  const char* e = nullptr;
  if (envelope::check_args(in, x, frame, opts, out, &e)) return fail(ctx, e);
  if (in->batch == 0) return 0;
  HIPCHK(hipSetDevice(ctx->device));
  envelope::Shape sh;
  envelope::make_shape(sh, *in, *opts);
  // only X, U and tau travel: the rows are packed to [X | U | tau] before the upload
  const size_t B = (size_t)in->batch, N = (size_t)in->N, nxu = 5 * N + 2 * (N - 1), nt = sh.topt ? N - 1 : 0;
  const size_t row = nxu + nt, K = (size_t)in->K, TEb = (size_t)sh.TEb;
  const bool raster = opts->W > 0;
  const size_t nw = raster ? (size_t)opts->H * (size_t)(opts->W / 32) : 0;
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
  const size_t o_G = o; o += al(16 * B * TEb);
  const size_t o_g = o; o += al(8 * B * TEb);
  const size_t o_p = o; o += al(8 * B * NPARAM);
  const size_t o_fr = o; o += al(24 * B);
  const size_t o_e = o; o += al(32 * B);
  const size_t o_w = o; o += al(48 * B);
  const size_t o_eb = o; o += al(32 * B * K);
  const size_t o_c = o; o += al(4 * B * (K + 1));
  const size_t o_f = o; o += al(4 * B);
  const size_t o_bm = o; o += al(4 * B * nw);
  char* d = nullptr;
  HIPCHK(hipMalloc((void**)&d, o));
  int rc = 0;
  auto H2D = [&](size_t off, const void* src, size_t n) {
    if (rc == 0 && n && hipMemcpy(d + off, src, n, hipMemcpyHostToDevice) != hipSuccess) rc = fail(ctx, "envelope: upload");
  };
  auto D2H = [&](void* dst, size_t off, size_t n) {
    if (rc == 0 && dst && n && hipMemcpy(dst, d + off, n, hipMemcpyDeviceToHost) != hipSuccess)
      rc = fail(ctx, "envelope: download");
  };
  H2D(o_x, xp.data(), 8 * B * row);
  H2D(o_G, in->body_G, 16 * B * TEb);
  H2D(o_g, in->body_g, 8 * B * TEb);
  H2D(o_p, in->params, 8 * B * NPARAM);
  H2D(o_fr, frame, 24 * B);
  const envelope::Batch b{(const double*)(d + o_G), (const double*)(d + o_g), (const double*)(d + o_p),
                          (const double*)(d + o_x), (const double*)(d + o_fr), (double*)(d + o_e),
                          (int32_t*)(d + o_w), out->extent_body ? (double*)(d + o_eb) : nullptr,
                          (int32_t*)(d + o_c), (raster && out->bitmap) ? (uint32_t*)(d + o_bm) : nullptr,
                          (int32_t*)(d + o_f)};
  if (rc == 0) rc = enqueue(ctx, sh, b, in->batch, nullptr);
  if (rc == 0) {
    hipError_t er = hipDeviceSynchronize();
    if (er != hipSuccess) rc = fail(ctx, std::string("envelope kernel: ") + hipGetErrorString(er));
  }
  D2H(out->extent, o_e, 32 * B);
  D2H(out->where, o_w, 48 * B);
  D2H(out->extent_body, o_eb, 32 * B * K);
  D2H(out->flags, o_f, 4 * B);
  if (raster) {   // without a raster the caller's cells and bitmap stay as they are
    D2H(out->cells, o_c, 4 * B * (K + 1));
    D2H(out->bitmap, o_bm, 4 * B * nw);
  }
  (void)hipFree(d);
  return rc;
}

double htp_obca_envelope_last_ms(htp_ctx* ctx) {
  if (!ctx || !ctx->envelope_ev.e1) return 0.0;
  float ms = 0.f;
  if (hipEventSynchronize(ctx->envelope_ev.e1) != hipSuccess) return 0.0;
  if (hipEventElapsedTime(&ms, ctx->envelope_ev.e0, ctx->envelope_ev.e1) != hipSuccess) return 0.0;
  return (double)ms;
}

}  // extern "C"
