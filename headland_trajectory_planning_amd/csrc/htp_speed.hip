// libhtp.so, maximal speed profile and timed trajectory of planner paths (speed_core.h): one path per 64-lane wavefront
// (one wavefront per workgroup); the workgroups stride over the batch, so the per-path scratch (WS_PER_NODE * cap_path
// doubles in HBM, structure of arrays: lanes over nodes read and write consecutive doubles) exists once per workgroup,
// not once per path.  The fixed-period rows are produced 64 at a time, one per lane, into an LDS tile that leaves as
// one contiguous run of stores.
#include <hip/hip_runtime.h>

#include <string>

#define HTP_HD __host__ __device__
#include "../../include/htp.h"
#include "htp_ctx.h"
#include "wave_ctx.h"
#include "speed_batch.h"

using namespace htp;

namespace {

__global__ __launch_bounds__(64) void speed_profile_kernel(htp_speed_in in, htp_speed_result out, double* ws) {
  __shared__ double tile[spd::TILE];
  DevWave c{(int)threadIdx.x, nullptr, nullptr};
  double* my = ws + (int64_t)blockIdx.x * spd::WS_PER_NODE * in.cap_path;
  for (int64_t b = blockIdx.x; b < in.batch; b += gridDim.x) {
    c.sync();   // the previous path is done with the scratch and the tile
    spd::run_path(c, in, out, b, my, tile);
  }
}

int enqueue(htp_ctx* ctx, const htp_speed_in& in, const htp_speed_result& out, hipStream_t s) {
  if (!ctx->speed_ev.e0) HIPCHK(hipEventCreate(&ctx->speed_ev.e0));
  if (!ctx->speed_ev.e1) HIPCHK(hipEventCreate(&ctx->speed_ev.e1));
  if (ctx->speed_groups == 0) {   // what the device holds at once: more workgroups would only queue behind these
    int per_cu = 0, cus = 0;
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, speed_profile_kernel, 64, 0));
    HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    ctx->speed_groups = per_cu * cus > 0 ? per_cu * cus : 1;
  }
  const size_t per_group = sizeof(double) * spd::WS_PER_NODE * (size_t)in.cap_path;
  int64_t groups = in.max_groups;
  if (groups == 0) {   // the library's choice: what is resident, but no more scratch than SCRATCH_BUDGET for it
    groups = ctx->speed_groups;
    const int64_t fit = (int64_t)(spd::SCRATCH_BUDGET / per_group);
    if (groups > fit) groups = fit > 0 ? fit : 1;
  }
  if (groups > in.batch) groups = in.batch;
  // the scratch is reused: order this launch after the previous one that used it
  if (order_after(ctx, ctx->speed_ev.e1, s)) return -1;
  if (ensure_buffer(ctx, ctx->speed_ws, per_group * (size_t)groups)) return -1;
  HIPCHK(hipEventRecord(ctx->speed_ev.e0, s));
  hipLaunchKernelGGL(speed_profile_kernel, dim3((unsigned)groups), dim3(64), 0, s, in, out, (double*)ctx->speed_ws.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ctx->speed_ev.e1, s));
  return 0;
}

}  // namespace

extern "C" {

int htp_speed_profile_batch_device(htp_ctx* ctx, const htp_speed_in* in, htp_speed_result* out, void* stream) {
  if (!ctx) return -1;
  const char* e = nullptr;
  if (spd::check_args(in, out, &e)) return fail(ctx, e);
  if (in->batch == 0) return 0;
  HIPCHK(hipSetDevice(ctx->device));
  return enqueue(ctx, *in, *out, (hipStream_t)stream);
}

int htp_speed_profile_batch(htp_ctx* ctx, const htp_speed_in* in, htp_speed_result* out) {
  if (!ctx) return -1;
  const char* e = nullptr;
  if (spd::check_args(in, out, &e)) return fail(ctx, e);
  if (in->batch == 0) return 0;
  HIPCHK(hipSetDevice(ctx->device));
  const size_t B = (size_t)in->batch, N = B * (size_t)in->cap_path;
  const size_t R = in->dt > 0.0 ? B * (size_t)in->cap_rows : 0;
  auto al = [](size_t v) { return (v + 255) & ~size_t(255); };
  size_t o = 0;
  const size_t o_p = o; o += al(8 * N * 5);
  const size_t o_n = o; o += al(4 * B);
  const size_t o_ps = o; o += al(4 * B);
  const size_t o_l = o; o += al(8 * B * spd::NLIM);
  const size_t o_st = o; o += al(4 * B);
  const size_t o_f = o; o += al(4 * B);
  const size_t o_sm = o; o += al(8 * B * spd::NSUM);
  const size_t o_nd = o; o += al(8 * N * spd::NNODE);
  const size_t o_a = o; o += al(4 * N);
  const size_t o_c = o; o += al(4 * B);
  const size_t o_r = o; o += al(8 * R * spd::NCOL);
  const size_t o_sg = o; o += al(4 * R);
  char* d = nullptr;
  HIPCHK(hipMalloc((void**)&d, o));
  int rc = 0;
  auto H2D = [&](size_t off, const void* src, size_t n) {
    if (rc == 0 && src && n && hipMemcpy(d + off, src, n, hipMemcpyHostToDevice) != hipSuccess)
      rc = fail(ctx, "[speed] upload");
  };
  auto D2H = [&](void* dst, size_t off, size_t n) {
    if (rc == 0 && dst && n && hipMemcpy(dst, d + off, n, hipMemcpyDeviceToHost) != hipSuccess)
      rc = fail(ctx, "[speed] download");
  };
  H2D(o_p, in->path, 8 * N * 5);
  H2D(o_n, in->n_path, 4 * B);
  H2D(o_ps, in->path_status, 4 * B);
  H2D(o_l, in->limits, 8 * B * spd::NLIM);
  // the caller's outputs travel too: what the kernel leaves unwritten comes back as it was
  H2D(o_sm, out->summary, 8 * B * spd::NSUM);
  H2D(o_nd, out->node, 8 * N * spd::NNODE);
  H2D(o_a, out->active, 4 * N);
  H2D(o_r, out->rows, 8 * R * spd::NCOL);
  H2D(o_sg, out->stage, 4 * R);
  htp_speed_in din = *in;
  din.path = (const double*)(d + o_p);
  din.n_path = (const int32_t*)(d + o_n);
  din.path_status = in->path_status ? (const int32_t*)(d + o_ps) : nullptr;
  din.limits = (const double*)(d + o_l);
  htp_speed_result dout{(int32_t*)(d + o_st), (int32_t*)(d + o_f), (double*)(d + o_sm),
                        out->node ? (double*)(d + o_nd) : nullptr, out->active ? (int32_t*)(d + o_a) : nullptr,
                        (int32_t*)(d + o_c), out->rows ? (double*)(d + o_r) : nullptr,
                        out->stage ? (int32_t*)(d + o_sg) : nullptr};
  if (rc == 0) rc = enqueue(ctx, din, dout, nullptr);
  if (rc == 0) {
    hipError_t er = hipStreamSynchronize(nullptr);   // the launch went to the null stream
    if (er != hipSuccess) rc = fail(ctx, std::string("[speed] kernel: ") + hipGetErrorString(er));
  }
  D2H(out->status, o_st, 4 * B);
  D2H(out->flags, o_f, 4 * B);
  D2H(out->summary, o_sm, 8 * B * spd::NSUM);
  D2H(out->node, o_nd, 8 * N * spd::NNODE);
  D2H(out->active, o_a, 4 * N);
  D2H(out->count, o_c, 4 * B);
  D2H(out->rows, o_r, 8 * R * spd::NCOL);
  D2H(out->stage, o_sg, 4 * R);
  (void)hipFree(d);
  return rc;
}

double htp_speed_profile_last_ms(htp_ctx* ctx) {
  if (!ctx || !ctx->speed_ev.e1) return 0.0;
  float ms = 0.f;
  if (hipEventSynchronize(ctx->speed_ev.e1) != hipSuccess) return 0.0;
  if (hipEventElapsedTime(&ms, ctx->speed_ev.e0, ctx->speed_ev.e1) != hipSuccess) return 0.0;
  return (double)ms;
}

}  // extern "C"
