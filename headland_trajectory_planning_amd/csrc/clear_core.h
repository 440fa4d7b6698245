// Clearance of one pose sequence against the obstacle / body polytopes of its scene, and the choice of the fastest
// admissible candidate of one problem (include/htp.h, "Clearance of pose sequences").  One path (or
// one problem) per 64-lane wavefront on gfx950 (htp_clear.hip) or a single serial lane (clear_hostsim.cpp, tests
// only); one __host__ __device__ source, so both produce the same doubles:
//   - no contraction (pragma below) and the planner libm (htp_libm.h) for sin, cos and hypot;
//   - the halfspace-to-edge construction, the signed distance and the order-preserving keys are the audit's
//     (audit_core.h, included unedited: build_row, point_edge via signed_distance, key_of), so a pose placed here and
//     by the audit yields the same double;
//   - every reduction is a minimum or a maximum (exact, order-free); the argmin of the clearance carries its (pose,
//     substep, obstacle, body) index and ties go to the lowest index.  There is no sum anywhere.
// The wave context W supplies lane, width, sync, any, minv, maxv, min_key, lds_min (the audit's) and copy_run.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/htp.h"
#include "audit_core.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif

namespace htp {
namespace clr {

constexpr int ER = audit::ER;
constexpr int MAXSUB = HTP_CLR_MAX_SUBSTEPS;
constexpr int CHUNK_PLACED = 128;    // placed poses staged in LDS at once; given poses per chunk = CHUNK_PLACED / S
constexpr int TEO_MAX = audit::TEO_MAX, TEB_MAX = audit::TEB_MAX;
// LDS (doubles): obstacle edges | body edges | polygon (first row, edge count) | placed poses (x, y, cos, sin) |
// the chunk's given poses and the one after them (x, y, yaw) | per-pose clearance keys.  The raw halfspace rows live
// in the placed-pose area until the edges are built.
constexpr int L_EO = 0, L_EB = L_EO + ER * TEO_MAX, L_PI = L_EB + ER * TEB_MAX, L_POSE = L_PI + 2 * (MAXM + MAXK);
constexpr int L_RAW = L_POSE + 4 * CHUNK_PLACED, L_KEY = L_RAW + 3 * (CHUNK_PLACED + 1) + 1;
constexpr int L_TOTAL = L_KEY + CHUNK_PLACED;   // 896 + 224 + 40 + 512 + 388 + 128 = 2188 doubles = 17504 bytes
static_assert(3 * (TEO_MAX + TEB_MAX) <= 4 * CHUNK_PLACED, "raw rows fit the placed-pose area");
static_assert(L_TOTAL == 2188, "the layout DESIGN.md s.3.18 and tests/test_clear_resources_cpu.py state");

constexpr double INF = audit::INF;
constexpr double TWO_PI = 6.283185307179586, PI = 3.141592653589793;   // the speed block's constants
constexpr int NSUM = HTP_SPD_NSUM, NCOL = HTP_TIMELINE_NCOL, NMETRIC = HTP_CLR_NMETRIC;

HTP_HD inline double wrap_(double d) { return d - TWO_PI * floor((d + PI) / TWO_PI); }
// Out of line: inlined, the double-double constants of the libm crowd the scalar registers (as in speed_core.h)
HTP_HD __attribute__((noinline)) inline double hypot_(double x, double y) { return hm::hypot(x, y); }
struct SinCos { double s, c; };   // by value: references to locals would put them in private memory
HTP_HD __attribute__((noinline)) inline SinCos sincos_(double x) {
  SinCos r;
  hm::sincos(x, r.s, r.c);
  return r;
}

// The edge counts (3..8) of up to 16 polygons, four bits each: the launch-uniform shape stays a handful of scalar
// registers across the striding loop over the paths instead of forty.
HTP_HD inline int edges_of(uint64_t packed, int j) { return (int)((packed >> (4 * j)) & 15u); }
HTP_HD inline int first_of(uint64_t packed, int j) {
  int off = 0;
  for (int i = 0; i < j; ++i) off += edges_of(packed, i);
  return off;
}
// the polygon (first row, edge count) that holds `row`
HTP_HD inline void polygon_of(uint64_t packed, int count, int row, int& first, int& cnt) {
  int off = 0;
  first = 0; cnt = 0;
  for (int j = 0; j < count; ++j) {
    const int e = edges_of(packed, j);
    if (row >= off && row < off + e) { first = off; cnt = e; }
    off += e;
  }
}

struct Shape {   // launch-uniform
  int cap, stride, cx, cy, cyaw, M, K, S, n_scenes;
  uint64_t eo, eb;   // edges_of()
  int TEo, TEb;
  double margin_tol;
};

struct Batch {   // device or host pointers
  const double* poses;
  const int32_t *n_poses, *pose_status, *scene;
  const double *obsA, *obsb, *bodyG, *bodyg, *margin;
  int32_t *status, *flags;
  double* metrics;
  int32_t* worst;
  double* pose_clearance;   // nullable
};

inline void make_shape(Shape& s, const htp_clear_in& in) {
  s.cap = in.cap_poses; s.stride = in.stride; s.cx = in.col_x; s.cy = in.col_y; s.cyaw = in.col_yaw;
  s.M = in.M; s.K = in.K; s.S = in.substeps; s.n_scenes = in.n_scenes;
  s.TEo = 0; s.TEb = 0; s.eo = 0; s.eb = 0;
  for (int m = 0; m < in.M; ++m) { s.eo |= (uint64_t)in.obs_edges[m] << (4 * m); s.TEo += in.obs_edges[m]; }
  for (int k = 0; k < in.K; ++k) { s.eb |= (uint64_t)in.body_edges[k] << (4 * k); s.TEb += in.body_edges[k]; }
  s.margin_tol = in.margin_tol;
}

inline Batch batch_view(const htp_clear_in& in, const htp_clear_result& out) {
  return Batch{in.poses, in.n_poses, in.pose_status, in.scene, in.obs_A, in.obs_b, in.body_G, in.body_g, in.margin,
               out.status, out.flags, out.metrics, out.worst, out.pose_clearance};
}

// The serial lane of the test-only host build; the gfx950 wavefront is in htp_clear.hip.
struct HostLane : audit::HostLane {
  void copy_run(double* dst, const double* src, int64_t n) const {
    for (int64_t q = 0; q < n; ++q) dst[q] = src[q];
  }
};

// One path.  sl: L_TOTAL doubles of LDS (8-byte aligned).
template <class W>
HTP_HD inline void run_path(const W& c, const Shape& sh, const Batch& b, int64_t p, double* sl) {
  const int M = sh.M, K = sh.K, S = sh.S, stride = sh.stride;
  double* Eo = sl + L_EO;
  double* Eb = sl + L_EB;
  double* pinfo = sl + L_PI;
  double* pose = sl + L_POSE;
  double* raw = sl + L_RAW;
  uint64_t* keys = (uint64_t*)(sl + L_KEY);
  double* rawO = pose;
  double* rawB = pose + 3 * TEO_MAX;

  // ---- what is decided by the path's own integers, before anything is read through them
  const int n_given = b.n_poses[p];
  const int n = n_given < sh.cap ? n_given : sh.cap;
  const int64_t sc = b.scene ? (int64_t)b.scene[p] : p;
  int st = HTP_CLR_OK;
  if (b.pose_status && b.pose_status[p] != 0) st = HTP_CLR_SKIPPED;
  else if (n < 1 || sc < 0 || sc >= sh.n_scenes) st = HTP_CLR_BAD_INPUT;
  if (st != HTP_CLR_OK) {
    if (c.lane == 0) { b.status[p] = st; b.flags[p] = 0; }
    return;
  }
  const double* P = b.poses + p * (int64_t)sh.cap * stride;

  // ---- the doubles read: the three columns of the n poses, the scene's halfspace rows, its margin
  bool bad = false;
  for (int i = c.lane; i < n; i += c.width) {   // only the three columns: the others may hold anything
    const double* r = P + (int64_t)i * stride;
    bad = bad || audit::nonfinite_(r[sh.cx]) || audit::nonfinite_(r[sh.cy]) || audit::nonfinite_(r[sh.cyaw]);
  }
  c.sync();   // the previous path of this workgroup no longer reads the placed-pose area
  for (int r = c.lane; r < sh.TEo; r += c.width) {
    const double ax = b.obsA[(sc * sh.TEo + r) * 2], ay = b.obsA[(sc * sh.TEo + r) * 2 + 1], bb = b.obsb[sc * sh.TEo + r];
    rawO[3 * r] = ax; rawO[3 * r + 1] = ay; rawO[3 * r + 2] = bb;
    bad = bad || audit::nonfinite_(ax) || audit::nonfinite_(ay) || audit::nonfinite_(bb);
  }
  for (int r = c.lane; r < sh.TEb; r += c.width) {
    const double ax = b.bodyG[(sc * sh.TEb + r) * 2], ay = b.bodyG[(sc * sh.TEb + r) * 2 + 1], bb = b.bodyg[sc * sh.TEb + r];
    rawB[3 * r] = ax; rawB[3 * r + 1] = ay; rawB[3 * r + 2] = bb;
    bad = bad || audit::nonfinite_(ax) || audit::nonfinite_(ay) || audit::nonfinite_(bb);
  }
  const double margin = b.margin ? b.margin[sc] : 0.0;
  bad = bad || audit::nonfinite_(margin);
  bad = c.any(bad);
  c.sync();
  if (bad) {
    if (c.lane == 0) { b.status[p] = HTP_CLR_BAD_INPUT; b.flags[p] = 0; }
    return;
  }

  // ---- polygons, per path (the next path of this workgroup may have another scene): one row per lane, then one
  // polygon per lane compacts its edges in place (as audit::run_problem does)
  for (int r = c.lane; r < sh.TEo + sh.TEb; r += c.width) {
    const bool body = r >= sh.TEo;
    const int rr = body ? r - sh.TEo : r;
    int first, cnt;
    polygon_of(body ? sh.eb : sh.eo, body ? K : M, rr, first, cnt);
    audit::build_row(body ? rawB : rawO, first, cnt, rr, (body ? Eb : Eo) + ER * rr);
  }
  c.sync();
  for (int j = c.lane; j < M + K; j += c.width) {
    const bool body = j >= M;
    const int first = body ? first_of(sh.eb, j - M) : first_of(sh.eo, j);
    const int cnt = body ? edges_of(sh.eb, j - M) : edges_of(sh.eo, j);
    double* E = (body ? Eb : Eo) + ER * first;
    int ne = 0;
    bool pb = false;
    for (int e = 0; e < cnt; ++e) {
      const int rs = (int)E[ER * e + 6];
      if (rs == audit::ROW_EDGE) {
        for (int q = 0; q < ER; ++q) E[ER * ne + q] = E[ER * e + q];
        ++ne;
      } else if (rs != audit::ROW_REDUNDANT) {
        pb = true;
      }
    }
    pinfo[2 * j] = (double)first;
    pinfo[2 * j + 1] = (pb || ne < 3) ? -1.0 : (double)ne;
  }
  c.sync();
  bool polybad = false;
  for (int j = 0; j < M + K; ++j) polybad = polybad || pinfo[2 * j + 1] < 0.0;
  if (polybad) {
    if (c.lane == 0) { b.status[p] = HTP_CLR_BAD_POLYTOPE; b.flags[p] = 0; }
    return;
  }

  // ---- chunks of CP given poses: their three columns into LDS (the rows are read as one contiguous run), the placed
  // poses (x, y, cos, sin), then lanes strided over (pose, substep, obstacle, body)
  double best = INF, node = INF, gap = 0.0, turn = 0.0;
  int bidx = 0x7fffffff;
  const int CP = CHUNK_PLACED / S, MK = M * K;
  for (int i0 = 0; i0 < n; i0 += CP) {
    const int ni = (n - i0 < CP) ? n - i0 : CP;
    const int nl = (n - i0 < CP + 1) ? n - i0 : CP + 1;   // with the pose that closes the chunk's last gap
    c.sync();   // the previous chunk's poses and keys (or the raw rows) are no longer read
    const double* run = P + (int64_t)i0 * stride;
    for (int q = c.lane; q < nl * stride; q += c.width) {
      const int j = q / stride, col = q - j * stride;
      const int w = col == sh.cx ? 0 : col == sh.cy ? 1 : col == sh.cyaw ? 2 : -1;
      if (w >= 0) raw[3 * j + w] = run[q];
    }
    for (int j = c.lane; j < ni; j += c.width) keys[j] = ~(uint64_t)0;
    c.sync();
    for (int t = c.lane; t < ni * S; t += c.width) {
      const int j = t / S, q = t - j * S, i = i0 + j;
      double x = raw[3 * j], y = raw[3 * j + 1], yaw = raw[3 * j + 2];
      if (i < n - 1) {
        const double dx = raw[3 * j + 3] - x, dy = raw[3 * j + 4] - y, dw = wrap_(raw[3 * j + 5] - yaw);
        if (q == 0) {
          gap = audit::dmax_(gap, hypot_(dx, dy));
          turn = audit::dmax_(turn, audit::dabs_(dw));
        } else {
          const double lam = (double)q / (double)S;
          x = x + lam * dx; y = y + lam * dy; yaw = yaw + lam * dw;
        }
      }
      const SinCos h = sincos_(yaw);
      pose[4 * t] = x; pose[4 * t + 1] = y; pose[4 * t + 2] = h.c; pose[4 * t + 3] = h.s;
    }
    c.sync();
    for (int w = c.lane; w < ni * S * MK; w += c.width) {
      const int t = w / MK, mk = w - t * MK, m = mk / K, k = mk - m * K;
      const int j = t / S, q = t - j * S;
      if (q > 0 && i0 + j == n - 1) continue;   // the last pose opens no gap
      const double* Q = pose + 4 * t;
      const double d = audit::signed_distance(Eo + ER * (int)pinfo[2 * m], (int)pinfo[2 * m + 1],
                                              Eb + ER * (int)pinfo[2 * (M + k)], (int)pinfo[2 * (M + k) + 1],
                                              Q[0], Q[1], Q[2], Q[3]);
      const int idx = i0 * S * MK + w;   // = ((i S + q) M + m) K + k, ascending per lane
      if (d < best) { best = d; bidx = idx; }
      if (q == 0) node = audit::dmin_(node, d);
      c.lds_min(keys + j, audit::key_of(d));
    }
    c.sync();
    if (b.pose_clearance)
      for (int j = c.lane; j < ni; j += c.width) b.pose_clearance[p * (int64_t)sh.cap + i0 + j] = audit::of_key(keys[j]);
  }
  c.min_key(best, bidx);
  node = c.minv(node);
  gap = c.maxv(gap);
  turn = c.maxv(turn);
  if (c.lane == 0) {
    double* mt = b.metrics + p * NMETRIC;
    mt[HTP_CLR_CLEARANCE] = best;
    mt[HTP_CLR_CLEARANCE_NODE] = node;
    mt[HTP_CLR_MAX_GAP] = gap;
    mt[HTP_CLR_MAX_TURN] = turn;
    const int t = bidx / MK, mk = bidx - t * MK;
    int32_t* wo = b.worst + p * 4;
    wo[0] = t / S; wo[1] = t % S; wo[2] = mk / K; wo[3] = mk % K;
    int fl = 0;
    if (best < 0.0) fl |= HTP_CLR_F_COLLISION;
    if (b.margin && best < margin - sh.margin_tol) fl |= HTP_CLR_F_MARGIN;
    if (n_given > sh.cap) fl |= HTP_CLR_F_TRUNCATED;
    b.status[p] = HTP_CLR_OK;
    b.flags[p] = fl;
  }
}

// One problem of the selection: every lane evaluates the C verdicts (uniform, no reduction), lane 0 writes them, and
// all lanes copy the winner's rows.
template <class W>
HTP_HD inline void select_problem(const W& c, const htp_select_in& in, const htp_select_result& out, int64_t b) {
  const int64_t B = in.batch;
  int win = -1;
  double tw = 0.0;
  for (int k = 0; k < in.C; ++k) {
    const int64_t j = (int64_t)k * B + b;
    const int ss = in.spd_status[j];
    int v = 0;
    if (ss == HTP_SPD_SKIPPED) v |= HTP_SEL_NOT_PLANNED;
    // any speed status but OK and SKIPPED is BAD (BAD_INPUT today): a value this kernel does not know never wins
    if ((ss != HTP_SPD_OK && ss != HTP_SPD_SKIPPED) || in.clr_status[j] != HTP_CLR_OK) v |= HTP_SEL_BAD;
    if (in.spd_flags[j] & in.reject_speed_flags) v |= HTP_SEL_SPEED_FLAG;
    if (in.clr_flags[j] & in.reject_clear_flags) v |= HTP_SEL_CLEAR_FLAG;
    double T = 0.0;
    if (ss == HTP_SPD_OK) {   // the speed profile writes a summary only of a path it timed
      T = in.spd_summary[j * NSUM + HTP_SPD_S_T];
      if (audit::nonfinite_(T)) v |= HTP_SEL_NONFINITE;
      else if (in.t_max > 0.0 && T > in.t_max) v |= HTP_SEL_TOO_LONG;
    }
    if (c.lane == 0) out.verdict[b * in.C + k] = v;
    if (v == 0 && (win < 0 || T < tw)) { win = k; tw = T; }
  }
  const int64_t jw = (int64_t)win * B + b;
  if (c.lane == 0) {
    out.winner[b] = win;
    out.score[b] = win >= 0 ? tw : __builtin_nan("");
    if (out.clearance) out.clearance[b] = win >= 0 ? in.clr_metrics[jw * NMETRIC + HTP_CLR_CLEARANCE] : __builtin_nan("");
  }
  if (in.rows) {
    const int cnt = win >= 0 ? in.count[jw] : 0;
    if (c.lane == 0) out.out_count[b] = cnt;
    const int m = cnt < in.cap_rows ? cnt : in.cap_rows;
    if (m > 0)
      c.copy_run(out.out_rows + b * (int64_t)in.cap_rows * NCOL, in.rows + jw * (int64_t)in.cap_rows * NCOL,
                 (int64_t)m * NCOL);
  }
}

}  // namespace clr
}  // namespace htp

#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC pop_options
#endif
