// libhtp.so, repair of solves that lose the margin between nodes (repair_core.h): pack (scan + gather), merge
// (decide + scatter) and the loop around the solve and the audit.
//   scan     one workgroup of 1024 threads walks the batch 1024 problems at a time: a ballot and a popcount
//            per wavefront, an integer prefix over the 16 wavefront totals in LDS and a running base number
//            the packed problems in ascending order (exact, order-free).
//   gather   PARTS workgroups of 256 threads per slot; every array of a slot is one contiguous run in source
//   scatter  and destination, moved with 16-byte stores over the 16-byte-aligned middle of the destination
//            (one double peeled at either end) and 16-byte loads where the source has the same parity, two
//            8-byte loads per store where not; consecutive lanes touch consecutive 16 bytes, no lane walks a
//            strided row.
//   decide   one thread per slot.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#define HTP_HD __host__ __device__
#include "../../include/htp.h"
#include "htp_ctx.h"
#include "repair_batch.h"

using namespace htp;

namespace {

typedef double dbl2 __attribute__((ext_vector_type(2)));

constexpr int PARTS = 4, GROUP = 256, SCAN = 1024;

struct Group {
  int tid, nth;
  // n doubles (8-byte aligned runs); every access lies inside dst[0 .. n) and src[0 .. n)
  __device__ __forceinline__ void copy(double* dst, const double* src, int n) const {
    const int odd = (int)(((uintptr_t)dst >> 3) & 1u);
    const int peel = odd < n ? odd : n;
    const int np = (n - peel) >> 1;
    dbl2* d2 = (dbl2*)(dst + peel);
    const double* s = src + peel;
    if ((((uintptr_t)s >> 3) & 1u) == 0) {
      const dbl2* s2 = (const dbl2*)s;
      for (int q = tid; q < np; q += nth) d2[q] = s2[q];
    } else {
      for (int q = tid; q < np; q += nth) {
        dbl2 v;
        v.x = s[2 * q];
        v.y = s[2 * q + 1];
        d2[q] = v;
      }
    }
    if (tid == 0 && peel) dst[0] = src[0];
    if (tid == nth - 1 && peel + 2 * np < n) dst[n - 1] = src[n - 1];
  }
  __device__ __forceinline__ void add(int32_t* a, int v) const { atomicAdd(a, v); }
};

__global__ __launch_bounds__(SCAN) void repair_scan_kernel(repair::Shape sh, repair::PackView v) {
  __shared__ int wtot[SCAN / 64];
  const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
  int base = 0;
  for (int64_t c0 = 0; c0 < sh.batch; c0 += SCAN) {
    const int64_t p = c0 + tid;
    int vd = repair::V_NONE;
    if (p < sh.batch) {
      vd = repair::verdict(v, sh, p);
      repair::mark(v, p, vd);
    }
    const bool pk = vd == repair::V_PACK;
    const unsigned long long bal = __ballot(pk ? 1 : 0);
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wtot[w] = __popcll(bal);
    __syncthreads();
    int woff = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < SCAN / 64; ++k) {
      const int t = wtot[k];
      woff += k < w ? t : 0;
      tot += t;
    }
    const int slot = base + woff + before;
    if (pk && slot < sh.cap) v.sl.index[slot] = (int32_t)p;
    base += tot;
    __syncthreads();
  }
  if (tid == 0) *v.sl.count = base;
}

__device__ __forceinline__ int slots_used(const repair::Shape& sh, const int32_t* count) {
  const int n = *count;
  return n < sh.cap ? n : sh.cap;
}

__global__ __launch_bounds__(GROUP) void repair_gather_kernel(repair::Shape sh, repair::PackView v) {
  const int64_t s = blockIdx.x / PARTS;
  if (s >= slots_used(sh, v.sl.count)) return;
  Group c{(int)(blockIdx.x % PARTS) * GROUP + (int)threadIdx.x, PARTS * GROUP};
  repair::gather_slot(c, sh, v, s);
}

__global__ __launch_bounds__(GROUP) void repair_decide_kernel(repair::Shape sh, repair::MergeView v) {
  const int64_t s = (int64_t)blockIdx.x * GROUP + threadIdx.x;
  if (s >= slots_used(sh, v.sl.count)) return;
  Group c{0, 1};
  repair::decide_slot(c, v, s);
}

__global__ __launch_bounds__(GROUP) void repair_scatter_kernel(repair::Shape sh, repair::MergeView v) {
  const int64_t s = blockIdx.x / PARTS;
  if (s >= slots_used(sh, v.sl.count)) return;
  Group c{(int)(blockIdx.x % PARTS) * GROUP + (int)threadIdx.x, PARTS * GROUP};
  repair::scatter_slot(c, sh, v, s);
}

int ensure_pair(htp_ctx* ctx, htp_event_pair& ev) {
  if (!ev.e0) HIPCHK(hipEventCreate(&ev.e0));
  if (!ev.e1) HIPCHK(hipEventCreate(&ev.e1));
  return 0;
}

double pair_ms(htp_event_pair& ev) {
  float ms = 0.f;
  if (!ev.e1 || hipEventSynchronize(ev.e1) != hipSuccess) return 0.0;
  if (hipEventElapsedTime(&ms, ev.e0, ev.e1) != hipSuccess) return 0.0;
  return (double)ms;
}

int enqueue_scan(htp_ctx* ctx, const repair::Shape& sh, const repair::PackView& v, hipStream_t s) {
  if (ensure_pair(ctx, ctx->repair.scan_ev)) return -1;
  HIPCHK(hipEventRecord(ctx->repair.scan_ev.e0, s));
  hipLaunchKernelGGL(repair_scan_kernel, dim3(1), dim3(SCAN), 0, s, sh, v);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ctx->repair.scan_ev.e1, s));
  return 0;
}

// slots: blocks are launched for this many slots; those at or beyond min(count, cap) return at once
int enqueue_gather(htp_ctx* ctx, const repair::Shape& sh, const repair::PackView& v, int slots, hipStream_t s) {
  if (ensure_pair(ctx, ctx->repair.gather_ev)) return -1;
  HIPCHK(hipEventRecord(ctx->repair.gather_ev.e0, s));
  hipLaunchKernelGGL(repair_gather_kernel, dim3((unsigned)slots * PARTS), dim3(GROUP), 0, s, sh, v);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ctx->repair.gather_ev.e1, s));
  return 0;
}

int enqueue_merge(htp_ctx* ctx, const repair::Shape& sh, const repair::MergeView& v, int slots, hipStream_t s) {
  if (ensure_pair(ctx, ctx->repair.merge_ev)) return -1;
  HIPCHK(hipEventRecord(ctx->repair.merge_ev.e0, s));
  hipLaunchKernelGGL(repair_decide_kernel, dim3((unsigned)((slots + GROUP - 1) / GROUP)), dim3(GROUP), 0, s, sh, v);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(repair_scatter_kernel, dim3((unsigned)slots * PARTS), dim3(GROUP), 0, s, sh, v);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ctx->repair.merge_ev.e1, s));
  return 0;
}

int min_i(int a, int b) { return a < b ? a : b; }

// Host arrays staged to device allocations of their own: add() uploads, finish() synchronises and downloads.
struct Stage {
  htp_ctx* ctx;
  int rc = 0;
  struct Entry { void* d; void* h; size_t n; bool down; };
  std::vector<Entry> es;
  explicit Stage(htp_ctx* c) : ctx(c) {}
  Stage(const Stage&) = delete;
  Stage& operator=(const Stage&) = delete;
  ~Stage() {
    for (auto& e : es) (void)hipFree(e.d);
  }
  template <class T>
  T* add(const T* h, size_t count, bool up, bool down) {   // a null (optional) host array stays null
    if (!h || !count || rc) return nullptr;
    const size_t n = count * sizeof(T);
    void* d = nullptr;
    if (hipMalloc(&d, n) != hipSuccess) { rc = fail(ctx, "[repair] device allocation failed"); return nullptr; }
    es.push_back(Entry{d, (void*)h, n, down});
    if (up && hipMemcpy(d, h, n, hipMemcpyHostToDevice) != hipSuccess) rc = fail(ctx, "[repair] upload failed");
    return (T*)d;
  }
  int finish() {
    if (rc) return rc;
    const hipError_t er = hipDeviceSynchronize();
    if (er != hipSuccess) return rc = fail(ctx, std::string("[repair] kernel: ") + hipGetErrorString(er));
    for (auto& e : es)
      if (e.down && hipMemcpy(e.h, e.d, e.n, hipMemcpyDeviceToHost) != hipSuccess) return rc = fail(ctx, "[repair] download failed");
    return 0;
  }
};

struct Sizes {   // doubles (or entries) per problem of every array
  size_t traj, A, b, G, g, u, mu, la, x, N;
};
Sizes sizes_of(const repair::Shape& sh) {
  return Sizes{(size_t)NS * sh.N, (size_t)sh.nA, (size_t)sh.nb, (size_t)sh.nG, (size_t)sh.ng, (size_t)sh.nU,
               (size_t)sh.nMU, (size_t)sh.nLA, (size_t)sh.n_var, (size_t)sh.N};
}

htp_obca_batch stage_inputs(Stage& st, const htp_obca_batch& in, const Sizes& z) {
  const size_t B = (size_t)in.batch;
  htp_obca_batch d = in;
  d.traj = st.add(in.traj, B * z.traj, true, false);
  d.obs_A = st.add(in.obs_A, B * z.A, true, false);
  d.obs_b = st.add(in.obs_b, B * z.b, true, false);
  d.body_G = st.add(in.body_G, B * z.G, true, false);
  d.body_g = st.add(in.body_g, B * z.g, true, false);
  d.params = st.add(in.params, B * NPARAM, true, false);
  d.init_control = d.init_mu = d.init_lambda = nullptr;
  return d;
}

htp_obca_result stage_result(Stage& st, const htp_obca_result& r, size_t rows, const Sizes& z, bool down) {
  htp_obca_result d;
  d.x = st.add(r.x, rows * z.x, true, down);
  d.objective = st.add(r.objective, rows, true, down);
  d.status = st.add(r.status, rows, true, down);
  d.iterations = st.add(r.iterations, rows, true, down);
  d.n_factor = st.add(r.n_factor, rows, true, down);
  d.nlp_error = st.add(r.nlp_error, rows, true, down);
  d.n_resto = st.add(r.n_resto, rows, true, down);
  return d;
}

htp_obca_audit_result stage_audit(Stage& st, const htp_obca_audit_result& a, size_t rows, const Sizes& z, bool up,
                                  bool down) {
  htp_obca_audit_result d;
  d.metrics = st.add(a.metrics, rows * HTP_AUDIT_NMETRIC, up, down);
  d.worst = st.add(a.worst, rows * 4, up, down);
  d.flags = st.add(a.flags, rows, up, down);
  d.stage_clearance = st.add(a.stage_clearance, rows * z.N, up, down);
  return d;
}

htp_obca_repair_state stage_state(Stage& st, const htp_obca_repair_state& s, size_t B, bool up) {
  htp_obca_repair_state d;
  d.state = st.add(s.state, B, up, true);
  d.rounds_used = st.add(s.rounds_used, B, up, true);
  d.extra_iterations = st.add(s.extra_iterations, B, up, true);
  d.dmin_used = st.add(s.dmin_used, B, up, true);
  return d;
}

// the slot arrays travel both ways, so that what the kernels leave alone keeps the caller's bytes
htp_obca_repair_slots stage_slots(Stage& st, const htp_obca_repair_slots& s, const Sizes& z, bool down) {
  const size_t C = (size_t)s.cap;
  htp_obca_repair_slots d = s;
  d.count = st.add(s.count, 1, true, down);
  d.index = st.add(s.index, C, true, down);
  d.adopted = st.add(s.adopted, C, true, true);
  d.traj = st.add(s.traj, C * z.traj, true, down);
  d.obs_A = st.add(s.obs_A, C * z.A, true, down);
  d.obs_b = st.add(s.obs_b, C * z.b, true, down);
  d.body_G = st.add(s.body_G, C * z.G, true, down);
  d.body_g = st.add(s.body_g, C * z.g, true, down);
  d.params = st.add(s.params, C * NPARAM, true, down);
  d.params_audit = st.add(s.params_audit, C * NPARAM, true, down);
  d.init_control = st.add(s.init_control, C * z.u, true, down);
  d.init_mu = st.add(s.init_mu, C * z.mu, true, down);
  d.init_lambda = st.add(s.init_lambda, C * z.la, true, down);
  return d;
}

// The loop's workspace for n slots, carved from ctx->repair.ws.
struct LoopWs {
  htp_obca_repair_slots slots;
  htp_obca_result re;
  htp_obca_audit_result re_audit;
};

int carve(htp_ctx* ctx, const Sizes& z, int n, bool stage, int32_t* count, int32_t* index, LoopWs& w) {
  const size_t C = (size_t)n;
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o += (bytes + 255) & ~size_t(255); return at; };
  const size_t o_ad = take(4 * C), o_tr = take(8 * C * z.traj), o_A = take(8 * C * z.A), o_b = take(8 * C * z.b);
  const size_t o_G = take(8 * C * z.G), o_g = take(8 * C * z.g), o_p = take(8 * C * NPARAM), o_pa = take(8 * C * NPARAM);
  const size_t o_u = take(8 * C * z.u), o_mu = take(8 * C * z.mu), o_la = take(8 * C * z.la);
  const size_t o_x = take(8 * C * z.x), o_obj = take(8 * C), o_st = take(4 * C), o_it = take(4 * C), o_nf = take(4 * C);
  const size_t o_ne = take(8 * C), o_nr = take(4 * C);
  const size_t o_m = take(8 * C * HTP_AUDIT_NMETRIC), o_w = take(16 * C), o_f = take(4 * C), o_sc = take(8 * C * z.N);
  if (ensure(ctx, &ctx->repair.ws.p, &ctx->repair.ws.bytes, o)) return -1;
  char* d = (char*)ctx->repair.ws.p;
  w.slots = htp_obca_repair_slots{n, count, index, (int32_t*)(d + o_ad), (double*)(d + o_tr), (double*)(d + o_A),
                                  (double*)(d + o_b), (double*)(d + o_G), (double*)(d + o_g), (double*)(d + o_p),
                                  (double*)(d + o_pa), (double*)(d + o_u), (double*)(d + o_mu), (double*)(d + o_la)};
  w.re = htp_obca_result{(double*)(d + o_x), (double*)(d + o_obj), (int32_t*)(d + o_st), (int32_t*)(d + o_it),
                         (int32_t*)(d + o_nf), (double*)(d + o_ne), (int32_t*)(d + o_nr)};
  w.re_audit = htp_obca_audit_result{(double*)(d + o_m), (int32_t*)(d + o_w), (int32_t*)(d + o_f),
                                     stage ? (double*)(d + o_sc) : nullptr};
  return 0;
}

}  // namespace

extern "C" {

int htp_obca_repair_pack_batch_device(htp_ctx* ctx, const htp_obca_batch* in, const htp_obca_result* out,
                                      const htp_obca_audit_result* audit, const htp_obca_repair_opts* opts,
                                      htp_obca_repair_state* state, htp_obca_repair_slots* slots, void* stream) {
  if (!ctx) return -1;
  const char* e = nullptr;
  if (repair::check_pack(in, out, audit, opts, state, slots, &e)) return fail(ctx, e);
  if (in->batch == 0) return 0;
  HIPCHK(hipSetDevice(ctx->device));
  repair::Shape sh;
  repair::make_shape(sh, *in, slots->cap, opts->pad, opts->max_raise);
  const repair::PackView v = repair::pack_view(*in, *out, *audit, *state, *slots);
  if (enqueue_scan(ctx, sh, v, (hipStream_t)stream)) return -1;
  return enqueue_gather(ctx, sh, v, min_i(slots->cap, in->batch), (hipStream_t)stream);
}

int htp_obca_repair_merge_batch_device(htp_ctx* ctx, const htp_obca_batch* in, const htp_obca_repair_slots* slots,
                                       const htp_obca_result* re, const htp_obca_audit_result* re_audit,
                                       htp_obca_result* out, htp_obca_audit_result* audit,
                                       htp_obca_repair_state* state, int32_t* tally, void* stream) {
  if (!ctx) return -1;
  const char* e = nullptr;
  if (repair::check_merge(in, slots, re, re_audit, out, audit, state, &e)) return fail(ctx, e);
  if (in->batch == 0) return 0;
  HIPCHK(hipSetDevice(ctx->device));
  repair::Shape sh;
  repair::make_shape(sh, *in, slots->cap, 0.0, 0.0);
  const repair::MergeView v = repair::merge_view(*slots, *re, *re_audit, *out, *audit, *state, tally);
  return enqueue_merge(ctx, sh, v, min_i(slots->cap, in->batch), (hipStream_t)stream);
}

int htp_obca_repair_pack_batch(htp_ctx* ctx, const htp_obca_batch* in, const htp_obca_result* out,
                               const htp_obca_audit_result* audit, const htp_obca_repair_opts* opts,
                               htp_obca_repair_state* state, htp_obca_repair_slots* slots) {
  if (!ctx) return -1;
  const char* e = nullptr;
  if (repair::check_pack(in, out, audit, opts, state, slots, &e)) return fail(ctx, e);
  if (in->batch == 0) return 0;
  HIPCHK(hipSetDevice(ctx->device));
  repair::Shape sh;
  repair::make_shape(sh, *in, slots->cap, opts->pad, opts->max_raise);
  const Sizes z = sizes_of(sh);
  const size_t B = (size_t)in->batch;
  Stage st(ctx);
  const htp_obca_batch din = stage_inputs(st, *in, z);
  htp_obca_result dout{};
  dout.x = st.add(out->x, B * z.x, true, false);
  dout.status = st.add(out->status, B, true, false);
  htp_obca_audit_result daud{};
  daud.metrics = st.add(audit->metrics, B * HTP_AUDIT_NMETRIC, true, false);
  daud.flags = st.add(audit->flags, B, true, false);
  htp_obca_repair_state dst = stage_state(st, *state, B, true);
  htp_obca_repair_slots dsl = stage_slots(st, *slots, z, true);
  if (st.rc) return st.rc;
  const repair::PackView v = repair::pack_view(din, dout, daud, dst, dsl);
  if (enqueue_scan(ctx, sh, v, nullptr) || enqueue_gather(ctx, sh, v, min_i(slots->cap, in->batch), nullptr)) return -1;
  return st.finish();
}

int htp_obca_repair_merge_batch(htp_ctx* ctx, const htp_obca_batch* in, const htp_obca_repair_slots* slots,
                                const htp_obca_result* re, const htp_obca_audit_result* re_audit,
                                htp_obca_result* out, htp_obca_audit_result* audit, htp_obca_repair_state* state,
                                int32_t* tally) {
  if (!ctx) return -1;
  const char* e = nullptr;
  if (repair::check_merge(in, slots, re, re_audit, out, audit, state, &e)) return fail(ctx, e);
  if (in->batch == 0) return 0;
  HIPCHK(hipSetDevice(ctx->device));
  repair::Shape sh;
  repair::make_shape(sh, *in, slots->cap, 0.0, 0.0);
  const Sizes z = sizes_of(sh);
  const size_t B = (size_t)in->batch, C = (size_t)slots->cap;
  Stage st(ctx);
  htp_obca_repair_slots dsl = stage_slots(st, *slots, z, false);
  const htp_obca_result dre = stage_result(st, *re, C, z, false);
  const htp_obca_audit_result dra = stage_audit(st, *re_audit, C, z, true, false);
  const htp_obca_result dout = stage_result(st, *out, B, z, true);
  const htp_obca_audit_result daud = stage_audit(st, *audit, B, z, true, true);
  htp_obca_repair_state dst = stage_state(st, *state, B, true);
  int32_t* dtally = st.add(tally, 3, true, true);
  if (st.rc) return st.rc;
  const repair::MergeView v = repair::merge_view(dsl, dre, dra, dout, daud, dst, dtally);
  if (enqueue_merge(ctx, sh, v, min_i(slots->cap, in->batch), nullptr)) return -1;
  return st.finish();
}

int htp_obca_repair_batch_device(htp_ctx* ctx, const htp_obca_batch* in, htp_obca_result* out,
                                 const htp_obca_repair_opts* opts, htp_obca_audit_result* audit_out,
                                 htp_obca_repair_report* report, void* stream) {
  if (!ctx) return -1;
  const char* e = nullptr;
  if (repair::check_loop(in, out, opts, audit_out, report, &e)) return fail(ctx, e);
  if (in->batch == 0) return 0;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  const size_t B = (size_t)in->batch;
  htp_obca_batch base = *in;
  base.init_control = base.init_mu = base.init_lambda = nullptr;
  if (htp_obca_audit_batch_device(ctx, &base, out->x, &opts->audit, audit_out, stream)) return -1;
  htp_obca_repair_state& rs = report->state;
  HIPCHK(hipMemsetAsync(rs.state, 0, 4 * B, s));
  HIPCHK(hipMemsetAsync(rs.rounds_used, 0, 4 * B, s));
  HIPCHK(hipMemsetAsync(rs.extra_iterations, 0, 4 * B, s));
  HIPCHK(hipMemsetAsync(rs.dmin_used, 0, 8 * B, s));
  HIPCHK(hipMemsetAsync(report->round_counts, 0, 4 * 3 * HTP_REPAIR_MAX_ROUNDS, s));
  // the selection: count, then index [batch]
  if (ensure(ctx, &ctx->repair.sel.p, &ctx->repair.sel.bytes, 256 + 4 * B)) return -1;
  int32_t* count = (int32_t*)ctx->repair.sel.p;
  int32_t* index = (int32_t*)((char*)ctx->repair.sel.p + 256);
  repair::Shape scan_sh;
  repair::make_shape(scan_sh, base, in->batch, opts->pad, opts->max_raise);
  const Sizes z = sizes_of(scan_sh);
  for (int r = 0; r < opts->rounds; ++r) {
    htp_obca_repair_slots sel{};
    sel.cap = in->batch;
    sel.count = count;
    sel.index = index;
    if (enqueue_scan(ctx, scan_sh, repair::pack_view(base, *out, *audit_out, rs, sel), s)) return -1;
    int32_t n = 0;
    HIPCHK(hipMemcpyAsync(&n, count, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (n <= 0) break;
    if (n > in->batch) return fail(ctx, "[repair] selection count out of range");
    LoopWs w;
    if (carve(ctx, z, n, audit_out->stage_clearance != nullptr, count, index, w)) return -1;
    repair::Shape sh = scan_sh;
    sh.cap = n;
    if (enqueue_gather(ctx, sh, repair::pack_view(base, *out, *audit_out, rs, w.slots), n, s)) return -1;
    const htp_obca_batch again = repair::slots_batch(base, w.slots, n, false);
    const htp_obca_batch judged = repair::slots_batch(base, w.slots, n, true);
    if (htp_obca_solve_batch_device(ctx, &again, &w.re, stream)) return -1;
    if (htp_obca_audit_batch_device(ctx, &judged, w.re.x, &opts->audit, &w.re_audit, stream)) return -1;
    const repair::MergeView mv = repair::merge_view(w.slots, w.re, w.re_audit, *out, *audit_out, rs,
                                                    report->round_counts + 3 * r);
    if (enqueue_merge(ctx, sh, mv, n, s)) return -1;
  }
  return 0;
}

int htp_obca_repair_batch(htp_ctx* ctx, const htp_obca_batch* in, htp_obca_result* out,
                          const htp_obca_repair_opts* opts, htp_obca_audit_result* audit_out,
                          htp_obca_repair_report* report) {
  if (!ctx) return -1;
  const char* e = nullptr;
  if (repair::check_loop(in, out, opts, audit_out, report, &e)) return fail(ctx, e);
  if (in->batch == 0) return 0;
  HIPCHK(hipSetDevice(ctx->device));
  repair::Shape sh;
  repair::make_shape(sh, *in, in->batch, opts->pad, opts->max_raise);
  const Sizes z = sizes_of(sh);
  const size_t B = (size_t)in->batch;
  Stage st(ctx);
  const htp_obca_batch din = stage_inputs(st, *in, z);
  htp_obca_result dout = stage_result(st, *out, B, z, true);
  htp_obca_audit_result daud = stage_audit(st, *audit_out, B, z, false, true);
  htp_obca_repair_report drep;
  drep.state = stage_state(st, report->state, B, false);
  drep.round_counts = st.add(report->round_counts, 3 * HTP_REPAIR_MAX_ROUNDS, false, true);
  if (st.rc) return st.rc;
  if (htp_obca_repair_batch_device(ctx, &din, &dout, opts, &daud, &drep, nullptr)) return -1;
  return st.finish();
}

int htp_obca_repair_last_ms(htp_ctx* ctx, double* pack_ms, double* merge_ms) {
  if (!ctx) return -1;
  if (pack_ms) *pack_ms = pair_ms(ctx->repair.scan_ev) + pair_ms(ctx->repair.gather_ev);
  if (merge_ms) *merge_ms = pair_ms(ctx->repair.merge_ev);
  return 0;
}

}  // extern "C"
