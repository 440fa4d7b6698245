// libhtp.so, clearance of pose sequences against OBCA polytopes and the choice of the fastest admissible candidate
// (clear_core.h): one path (one problem) per 64-lane wavefront, one wavefront per workgroup, the workgroups stride over
// the batch.  The scene's edges, the chunk's poses and the per-pose keys are LDS; the rows of a chunk are read as one
// contiguous run, the winner's rows are copied with 16-byte loads and stores.
#include <hip/hip_runtime.h>

#include <string>

#define HTP_HD __host__ __device__
#include "../../include/htp.h"
#include "htp_ctx.h"
#include "clear_batch.h"

using namespace htp;

namespace {

typedef double dbl2 __attribute__((ext_vector_type(2)));

struct ClearWave {
  static constexpr int width = 64;
  int lane;
  // the workgroup is one wavefront: LDS accesses are performed in program order, so a cross-lane
  // read-after-write only needs the compiler not to reorder them (wave_ctx.h DevWave::sync)
  __device__ __forceinline__ void sync() const {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  __device__ __forceinline__ double maxv(double v) const {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = audit::dmax_(v, __shfl_xor(v, o, 64));
    return v;
  }
  __device__ __forceinline__ double minv(double v) const {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = audit::dmin_(v, __shfl_xor(v, o, 64));
    return v;
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
  __device__ __forceinline__ void lds_min(uint64_t* slot, uint64_t key) const {
    atomicMin((unsigned long long*)slot, (unsigned long long)key);
  }
  // n doubles (n even) from HBM to HBM: 16-byte loads and stores where both ends are 16-byte aligned
  __device__ __forceinline__ void copy_run(double* dst, const double* src, int64_t n) const {
    if ((((uintptr_t)dst | (uintptr_t)src) & 15u) == 0 && (n & 1) == 0) {
      const dbl2* s2 = (const dbl2*)src;
      dbl2* d2 = (dbl2*)dst;
      for (int64_t q = lane; q < (n >> 1); q += 64) d2[q] = s2[q];
    } else {
      for (int64_t q = lane; q < n; q += 64) dst[q] = src[q];
    }
  }
};

__global__ __launch_bounds__(64) void pose_clearance_kernel(clr::Shape sh, clr::Batch b, int64_t batch) {
  __shared__ double sl[clr::L_TOTAL];
  ClearWave c{(int)threadIdx.x};
  for (int64_t p = blockIdx.x; p < batch; p += gridDim.x) clr::run_path(c, sh, b, p, sl);
}

__global__ __launch_bounds__(64) void turn_select_kernel(htp_select_in in, htp_select_result out) {
  ClearWave c{(int)threadIdx.x};
  for (int64_t b = blockIdx.x; b < in.batch; b += gridDim.x) clr::select_problem(c, in, out, b);
}

int ensure_events(htp_ctx* ctx, htp_event_pair& ev) {
  if (!ev.e0) HIPCHK(hipEventCreate(&ev.e0));
  if (!ev.e1) HIPCHK(hipEventCreate(&ev.e1));
  return 0;
}

template <class Kern>
int resident_groups(htp_ctx* ctx, Kern k, int& groups) {
  if (groups == 0) {   // what the device holds at once: more workgroups would only queue behind these
    int per_cu = 0, cus = 0;
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k, 64, 0));
    HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    groups = per_cu * cus > 0 ? per_cu * cus : 1;
  }
  return 0;
}

int enqueue_clear(htp_ctx* ctx, const htp_clear_in& in, const htp_clear_result& out, hipStream_t s) {
  if (ensure_events(ctx, ctx->clear_ev)) return -1;
  if (resident_groups(ctx, pose_clearance_kernel, ctx->clear_groups)) return -1;
  clr::Shape sh;
  clr::make_shape(sh, in);
  int64_t groups = in.max_groups ? in.max_groups : ctx->clear_groups;
  if (groups > in.batch) groups = in.batch;
  HIPCHK(hipEventRecord(ctx->clear_ev.e0, s));
  hipLaunchKernelGGL(pose_clearance_kernel, dim3((unsigned)groups), dim3(64), 0, s, sh, clr::batch_view(in, out),
                     (int64_t)in.batch);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ctx->clear_ev.e1, s));
  return 0;
}

int enqueue_select(htp_ctx* ctx, const htp_select_in& in, const htp_select_result& out, hipStream_t s) {
  if (ensure_events(ctx, ctx->select_ev)) return -1;
  if (resident_groups(ctx, turn_select_kernel, ctx->select_groups)) return -1;
  int64_t groups = ctx->select_groups;
  if (groups > in.batch) groups = in.batch;
  HIPCHK(hipEventRecord(ctx->select_ev.e0, s));
  hipLaunchKernelGGL(turn_select_kernel, dim3((unsigned)groups), dim3(64), 0, s, in, out);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ctx->select_ev.e1, s));
  return 0;
}

double elapsed(const htp_event_pair& ev) {
  if (!ev.e1) return 0.0;
  float ms = 0.f;
  if (hipEventSynchronize(ev.e1) != hipSuccess) return 0.0;
  if (hipEventElapsedTime(&ms, ev.e0, ev.e1) != hipSuccess) return 0.0;
  return (double)ms;
}

// The staged entries' device block: regions added with add(), filled from / read back to host arrays.  The block is the
// context's (clear_stage), grown on demand and kept: the entries are synchronous, so the next call finds it free.
struct Staging {
  htp_ctx* ctx;
  const char* tag;
  size_t bytes = 0;
  char* d = nullptr;
  int rc = 0;
  size_t add(size_t n) { const size_t o = bytes; bytes += (n + 255) & ~size_t(255); return o; }
  int alloc() {
    if (ensure_buffer(ctx, ctx->clear_stage, bytes ? bytes : 256)) return -1;
    d = (char*)ctx->clear_stage.p;
    return 0;
  }
  void up(size_t off, const void* src, size_t n) {
    if (rc == 0 && src && n && hipMemcpy(d + off, src, n, hipMemcpyHostToDevice) != hipSuccess)
      rc = fail(ctx, std::string(tag) + " upload");
  }
  void down(void* dst, size_t off, size_t n) {
    if (rc == 0 && dst && n && hipMemcpy(dst, d + off, n, hipMemcpyDeviceToHost) != hipSuccess)
      rc = fail(ctx, std::string(tag) + " download");
  }
  void finish() {   // the launch went to the null stream
    if (rc == 0) {
      hipError_t er = hipStreamSynchronize(nullptr);
      if (er != hipSuccess) rc = fail(ctx, std::string(tag) + " kernel: " + hipGetErrorString(er));
    }
  }
};

}  // namespace

extern "C" {

int htp_pose_clearance_batch_device(htp_ctx* ctx, const htp_clear_in* in, htp_clear_result* out, void* stream) {
  if (!ctx) return -1;
  const char* e = nullptr;
  if (clr::check_args(in, out, &e)) return fail(ctx, e);
  if (in->batch == 0) return 0;
  HIPCHK(hipSetDevice(ctx->device));
  return enqueue_clear(ctx, *in, *out, (hipStream_t)stream);
}

int htp_pose_clearance_batch(htp_ctx* ctx, const htp_clear_in* in, htp_clear_result* out) {
  if (!ctx) return -1;
  const char* e = nullptr;
  if (clr::check_args(in, out, &e)) return fail(ctx, e);
  if (in->batch == 0) return 0;
  HIPCHK(hipSetDevice(ctx->device));
  clr::Shape sh;
  clr::make_shape(sh, *in);
  const size_t B = (size_t)in->batch, NP = B * (size_t)in->cap_poses, NS = (size_t)in->n_scenes;
  const size_t TEo = (size_t)sh.TEo, TEb = (size_t)sh.TEb;
  Staging g{ctx, "[clearance]"};
  const size_t o_p = g.add(8 * NP * (size_t)in->stride), o_n = g.add(4 * B), o_ps = g.add(4 * B), o_sc = g.add(4 * B);
  const size_t o_A = g.add(16 * NS * TEo), o_b = g.add(8 * NS * TEo), o_G = g.add(16 * NS * TEb), o_g = g.add(8 * NS * TEb);
  const size_t o_mg = g.add(8 * NS);
  const size_t o_st = g.add(4 * B), o_f = g.add(4 * B), o_m = g.add(8 * B * clr::NMETRIC), o_w = g.add(16 * B);
  const size_t o_pc = g.add(out->pose_clearance ? 8 * NP : 0);
  if (g.alloc()) return -1;
  g.up(o_p, in->poses, 8 * NP * (size_t)in->stride);
  g.up(o_n, in->n_poses, 4 * B);
  g.up(o_ps, in->pose_status, 4 * B);
  g.up(o_sc, in->scene, 4 * B);
  g.up(o_A, in->obs_A, 16 * NS * TEo);
  g.up(o_b, in->obs_b, 8 * NS * TEo);
  g.up(o_G, in->body_G, 16 * NS * TEb);
  g.up(o_g, in->body_g, 8 * NS * TEb);
  g.up(o_mg, in->margin, 8 * NS);
  // the caller's outputs travel too: what the kernel leaves unwritten comes back as it was
  g.up(o_m, out->metrics, 8 * B * clr::NMETRIC);
  g.up(o_w, out->worst, 16 * B);
  g.up(o_pc, out->pose_clearance, 8 * NP);
  char* d = g.d;
  htp_clear_in din = *in;
  din.poses = (const double*)(d + o_p);
  din.n_poses = (const int32_t*)(d + o_n);
  din.pose_status = in->pose_status ? (const int32_t*)(d + o_ps) : nullptr;
  din.scene = in->scene ? (const int32_t*)(d + o_sc) : nullptr;
  din.obs_A = (const double*)(d + o_A);
  din.obs_b = (const double*)(d + o_b);
  din.body_G = (const double*)(d + o_G);
  din.body_g = (const double*)(d + o_g);
  din.margin = in->margin ? (const double*)(d + o_mg) : nullptr;
  htp_clear_result dout{(int32_t*)(d + o_st), (int32_t*)(d + o_f), (double*)(d + o_m), (int32_t*)(d + o_w),
                        out->pose_clearance ? (double*)(d + o_pc) : nullptr};
  if (g.rc == 0) g.rc = enqueue_clear(ctx, din, dout, nullptr);
  g.finish();
  g.down(out->status, o_st, 4 * B);
  g.down(out->flags, o_f, 4 * B);
  g.down(out->metrics, o_m, 8 * B * clr::NMETRIC);
  g.down(out->worst, o_w, 16 * B);
  g.down(out->pose_clearance, o_pc, 8 * NP);
  return g.rc;
}

double htp_pose_clearance_last_ms(htp_ctx* ctx) { return ctx ? elapsed(ctx->clear_ev) : 0.0; }

int htp_turn_select_batch_device(htp_ctx* ctx, const htp_select_in* in, htp_select_result* out, void* stream) {
  if (!ctx) return -1;
  const char* e = nullptr;
  if (clr::check_select(in, out, &e)) return fail(ctx, e);
  if (in->batch == 0) return 0;
  HIPCHK(hipSetDevice(ctx->device));
  return enqueue_select(ctx, *in, *out, (hipStream_t)stream);
}

int htp_turn_select_batch(htp_ctx* ctx, const htp_select_in* in, htp_select_result* out) {
  if (!ctx) return -1;
  const char* e = nullptr;
  if (clr::check_select(in, out, &e)) return fail(ctx, e);
  if (in->batch == 0) return 0;
  HIPCHK(hipSetDevice(ctx->device));
  const size_t B = (size_t)in->batch, N = B * (size_t)in->C;
  const size_t RB = in->rows ? (size_t)in->cap_rows * clr::NCOL : 0;   // doubles of one path's rows
  Staging g{ctx, "[select]"};
  const size_t o_ss = g.add(4 * N), o_sf = g.add(4 * N), o_sm = g.add(8 * N * clr::NSUM), o_r = g.add(8 * N * RB);
  const size_t o_c = g.add(4 * N), o_cs = g.add(4 * N), o_cf = g.add(4 * N), o_cm = g.add(8 * N * clr::NMETRIC);
  const size_t o_v = g.add(4 * N), o_w = g.add(4 * B), o_s = g.add(8 * B), o_cl = g.add(8 * B), o_or = g.add(8 * B * RB);
  const size_t o_oc = g.add(4 * B);
  if (g.alloc()) return -1;
  g.up(o_ss, in->spd_status, 4 * N);
  g.up(o_sf, in->spd_flags, 4 * N);
  g.up(o_sm, in->spd_summary, 8 * N * clr::NSUM);
  g.up(o_r, in->rows, 8 * N * RB);
  g.up(o_c, in->count, 4 * N);
  g.up(o_cs, in->clr_status, 4 * N);
  g.up(o_cf, in->clr_flags, 4 * N);
  g.up(o_cm, in->clr_metrics, 8 * N * clr::NMETRIC);
  g.up(o_or, out->out_rows, 8 * B * RB);   // rows beyond the winner's count come back as they were
  char* d = g.d;
  htp_select_in din = *in;
  din.spd_status = (const int32_t*)(d + o_ss);
  din.spd_flags = (const int32_t*)(d + o_sf);
  din.spd_summary = (const double*)(d + o_sm);
  din.rows = in->rows ? (const double*)(d + o_r) : nullptr;
  din.count = in->count ? (const int32_t*)(d + o_c) : nullptr;
  din.clr_status = (const int32_t*)(d + o_cs);
  din.clr_flags = (const int32_t*)(d + o_cf);
  din.clr_metrics = in->clr_metrics ? (const double*)(d + o_cm) : nullptr;
  htp_select_result dout{(int32_t*)(d + o_v), (int32_t*)(d + o_w), (double*)(d + o_s),
                         out->clearance ? (double*)(d + o_cl) : nullptr, in->rows ? (double*)(d + o_or) : nullptr,
                         in->rows ? (int32_t*)(d + o_oc) : nullptr};
  if (g.rc == 0) g.rc = enqueue_select(ctx, din, dout, nullptr);
  g.finish();
  g.down(out->verdict, o_v, 4 * N);
  g.down(out->winner, o_w, 4 * B);
  g.down(out->score, o_s, 8 * B);
  g.down(out->clearance, o_cl, 8 * B);
  if (in->rows) {
    g.down(out->out_rows, o_or, 8 * B * RB);
    g.down(out->out_count, o_oc, 4 * B);
  }
  return g.rc;
}

double htp_turn_select_last_ms(htp_ctx* ctx) { return ctx ? elapsed(ctx->select_ev) : 0.0; }

}  // extern "C"
