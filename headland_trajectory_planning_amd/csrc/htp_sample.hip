// libhtp.so, sampled exit / entry pose search of the classic turns (sample_core.h): three launches on one stream.
//   classic_sample_kernel<MASK> .. one (turn, candidate) work item per 64-lane wavefront (one wavefront per
//       workgroup); the workgroups stride over the items, so the planner's HBM scratch (WS_PER_POINT * cap_samples
//       doubles) exists once per workgroup, not once per item.  The turn's polygons are staged in LDS whenever the
//       workgroup moves on to another turn.  Two instances: M_ROWS plans the Dubins and circle-back turns (lanes over
//       path rows), M_WORDS the Reeds-Shepp turns (one word per lane); each passes over the other's items.
//   classic_sample_winner_kernel .. one wavefront per turn reduces the candidate table to the winner.
#include <hip/hip_runtime.h>

#include <string>

#define HTP_HD __host__ __device__
#include "../../include/htp.h"
#include "htp_ctx.h"
#include "wave_ctx.h"
#include "sample_batch.h"

using namespace htp;

namespace {

template <int MASK>
__global__ __launch_bounds__(64) void classic_sample_kernel(htp_classic_sample_in in, double* ws, double* cand_score,
                                                            int32_t* cand_status) {
  __shared__ smp::Scene S;
  __shared__ rs::Path paths[rs::MAXP];
  DevWave c{(int)threadIdx.x, nullptr, nullptr};
  const int64_t total = (int64_t)in.batch * in.cap_cand;
  double* my = ws + (int64_t)blockIdx.x * smp::WS_PER_POINT * in.cap_samples;
  smp::TurnInfo t;
  int64_t cur = -1;
  for (int64_t it = blockIdx.x; it < total; it += gridDim.x) {
    const int64_t b = it / in.cap_cand;
    const int k = (int)(it - b * in.cap_cand);
    if (smp::is_words_turn(in, b) != (MASK == smp::M_WORDS)) continue;
    c.sync();   // the previous item is done with the scratch, the words and the scene
    if (b != cur) {
      smp::turn_info(in, b, t);
      if (t.status == smp::ST_OK) smp::load_scene(c, in, b, t, S);
      cur = b;
    }
    smp::run_item<MASK>(c, in, cand_score, cand_status, b, k, t, S, my, paths);
  }
}

__global__ __launch_bounds__(64) void classic_sample_winner_kernel(htp_classic_sample_in in,
                                                                   htp_classic_sample_result out,
                                                                   const double* cand_score,
                                                                   const int32_t* cand_status) {
  const int64_t b = blockIdx.x;
  if (b >= in.batch) return;
  DevWave c{(int)threadIdx.x, nullptr, nullptr};
  smp::run_winner(c, in, out, cand_score, cand_status, b);
}

int enqueue(htp_ctx* ctx, const htp_classic_sample_in& in, const htp_classic_sample_result& out, hipStream_t s) {
  if (!ctx->sample_ev.e0) HIPCHK(hipEventCreate(&ctx->sample_ev.e0));
  if (!ctx->sample_ev.e1) HIPCHK(hipEventCreate(&ctx->sample_ev.e1));
  if (ctx->sample_groups == 0) {   // what the device holds at once: more workgroups would only queue behind these
    int per_cu = 0, cus = 0;
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, classic_sample_kernel<smp::M_ROWS>, 64, 0));
    HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    ctx->sample_groups = per_cu * cus > 0 ? per_cu * cus : 1;
  }
  const int64_t total = (int64_t)in.batch * in.cap_cand;
  int64_t groups = in.max_groups > 0 ? in.max_groups : ctx->sample_groups;
  if (groups > total) groups = total;
  // the workspaces are reused: order this launch after the previous one that used them
  if (order_after(ctx, ctx->sample_ev.e1, s)) return -1;
  if (ensure_buffer(ctx, ctx->sample_ws, sizeof(double) * smp::WS_PER_POINT * (size_t)in.cap_samples * (size_t)groups))
    return -1;
  double* cs = out.cand_score;
  int32_t* ct = out.cand_status;
  if (!cs) {
    if (ensure_buffer(ctx, ctx->sample_tab, 12 * (size_t)total)) return -1;
    cs = (double*)ctx->sample_tab.p;
    ct = (int32_t*)((char*)ctx->sample_tab.p + 8 * (size_t)total);
  }
  HIPCHK(hipEventRecord(ctx->sample_ev.e0, s));
  hipLaunchKernelGGL(classic_sample_kernel<smp::M_ROWS>, dim3((unsigned)groups), dim3(64), 0, s, in,
                     (double*)ctx->sample_ws.p, cs, ct);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(classic_sample_kernel<smp::M_WORDS>, dim3((unsigned)groups), dim3(64), 0, s, in,
                     (double*)ctx->sample_ws.p, cs, ct);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(classic_sample_winner_kernel, dim3((unsigned)in.batch), dim3(64), 0, s, in, out,
                     (const double*)cs, (const int32_t*)ct);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ctx->sample_ev.e1, s));
  return 0;
}

}  // namespace

extern "C" {

int htp_classic_sample_batch_device(htp_ctx* ctx, const htp_classic_sample_in* in, htp_classic_sample_result* out,
                                    void* stream) {
  if (!ctx) return -1;
  const char* e = nullptr;
  if (smp::check_args(in, out, &e)) return fail(ctx, e);
  if (in->batch == 0) return 0;
  HIPCHK(hipSetDevice(ctx->device));
  return enqueue(ctx, *in, *out, (hipStream_t)stream);
}

int htp_classic_sample_batch(htp_ctx* ctx, const htp_classic_sample_in* in, htp_classic_sample_result* out) {
  if (!ctx) return -1;
  const char* e = nullptr;
  if (smp::check_args(in, out, &e)) return fail(ctx, e);
  if (in->batch == 0) return 0;
  if (smp::check_polygons(in, &e)) return fail(ctx, e);
  HIPCHK(hipSetDevice(ctx->device));
  const size_t B = (size_t)in->batch, T = B * (size_t)in->cap_cand;
  auto al = [](size_t v) { return (v + 255) & ~size_t(255); };
  size_t o = 0;
  const size_t o_p = o; o += al(8 * B * HTP_CT_NPARAM);
  const size_t o_d = o; o += al(4 * B * HTP_SMP_NDESC);
  const size_t o_po = o; o += al(4 * (size_t)(in->npoly + 1));
  const size_t o_v = o; o += al(16 * (size_t)in->nvert);
  const size_t o_sx = o; o += al(8 * B * (size_t)in->cap_s);
  const size_t o_ex = o; o += al(8 * B * (size_t)in->cap_e);
  const size_t o_ns = o; o += al(4 * B);
  const size_t o_ne = o; o += al(4 * B);
  const size_t o_st = o; o += al(4 * B);
  const size_t o_w = o; o += al(8 * B);
  const size_t o_ps = o; o += al(8 * B * HTP_SMP_NPOSE);
  const size_t o_sc = o; o += al(8 * B);
  const size_t o_nf = o; o += al(4 * B);
  const size_t o_cs = o; o += al(8 * T);
  const size_t o_ct = o; o += al(4 * T);
  char* d = nullptr;
  HIPCHK(hipMalloc((void**)&d, o));
  int rc = 0;
  auto H2D = [&](size_t off, const void* src, size_t n) {
    if (rc == 0 && n && hipMemcpy(d + off, src, n, hipMemcpyHostToDevice) != hipSuccess) rc = fail(ctx, "sample: upload");
  };
  auto D2H = [&](void* dst, size_t off, size_t n) {
    if (rc == 0 && dst && n && hipMemcpy(dst, d + off, n, hipMemcpyDeviceToHost) != hipSuccess)
      rc = fail(ctx, "sample: download");
  };
  H2D(o_p, in->params, 8 * B * HTP_CT_NPARAM);
  H2D(o_d, in->desc, 4 * B * HTP_SMP_NDESC);
  H2D(o_po, in->poly_off, 4 * (size_t)(in->npoly + 1));
  H2D(o_v, in->vertices, 16 * (size_t)in->nvert);
  H2D(o_sx, in->start_x, 8 * B * (size_t)in->cap_s);
  H2D(o_ex, in->end_x, 8 * B * (size_t)in->cap_e);
  H2D(o_ns, in->n_start, 4 * B);
  H2D(o_ne, in->n_end, 4 * B);
  htp_classic_sample_in din = *in;
  din.params = (const double*)(d + o_p);
  din.desc = (const int32_t*)(d + o_d);
  din.poly_off = (const int32_t*)(d + o_po);
  din.vertices = (const double*)(d + o_v);
  din.start_x = (const double*)(d + o_sx);
  din.end_x = (const double*)(d + o_ex);
  din.n_start = (const int32_t*)(d + o_ns);
  din.n_end = (const int32_t*)(d + o_ne);
  htp_classic_sample_result dout{(int32_t*)(d + o_st), (int32_t*)(d + o_w), (double*)(d + o_ps), (double*)(d + o_sc),
                                 (int32_t*)(d + o_nf), (double*)(d + o_cs), (int32_t*)(d + o_ct)};
  if (rc == 0) rc = enqueue(ctx, din, dout, nullptr);
  if (rc == 0) {
    hipError_t er = hipDeviceSynchronize();
    if (er != hipSuccess) rc = fail(ctx, std::string("sample kernel: ") + hipGetErrorString(er));
  }
  D2H(out->status, o_st, 4 * B);
  D2H(out->winner, o_w, 8 * B);
  D2H(out->poses, o_ps, 8 * B * HTP_SMP_NPOSE);
  D2H(out->score, o_sc, 8 * B);
  D2H(out->n_feasible, o_nf, 4 * B);
  D2H(out->cand_score, o_cs, 8 * T);
  D2H(out->cand_status, o_ct, 4 * T);
  (void)hipFree(d);
  return rc;
}

double htp_classic_sample_last_ms(htp_ctx* ctx) {
  if (!ctx || !ctx->sample_ev.e1) return 0.0;
  float ms = 0.f;
  if (hipEventSynchronize(ctx->sample_ev.e1) != hipSuccess) return 0.0;
  if (hipEventElapsedTime(&ms, ctx->sample_ev.e0, ctx->sample_ev.e1) != hipSuccess) return 0.0;
  return (double)ms;
}

}  // extern "C"
