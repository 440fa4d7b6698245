// Geometric audit of one solved OBCA trajectory (FORM 0, R/obca_py/optimizer.py layout): signed distance
// between the placed body polygons and the obstacle polygons at the stage nodes and at poses between them,
// the dynamics defect, the variable-bound excess, the start / end miss, path length and time.  One problem
// per 64-lane wavefront on gfx950 (htp_audit.hip) or a single serial lane (audit_hostsim.cpp, tests only);
// one __host__ __device__ source, so both produce the same doubles:
//   - no contraction (pragma below) and the planner libm (htp_libm.h) for sin, cos and tan;
//   - every cross-lane reduction is a min or a max (exact, order-free); the argmin of the clearance carries
//     its (stage, substep, obstacle, body) index and ties go to the lowest index;
//   - the two sums (path length, total time) are added serially by one lane.
// Only X, U and tau of the decision vector are read: the duals and the slack play no part, so the result
// stays meaningful for a solve that has not converged.
//
// Polygons come as halfspaces (rows of any length, any order, possibly redundant).  Each row's line is
// clipped against every other row of its polygon: the surviving parameter interval [lo, hi] is the edge;
// an empty interval marks a redundant row, an unbounded one (or fewer than three edges) a bad polytope.
//
// Signed distance of two closed convex polygons: sep = the maximum over both polygons' unit edge normals
// of the minimum projection gap.  sep > 0: disjoint (in the plane some edge normal separates) and the
// distance is the minimum endpoint-to-segment distance over both directions; otherwise they intersect
// and -penetration depth = sep <= 0.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/htp.h"
#include "htp_common.h"
#include "htp_libm.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif

namespace htp {
namespace audit {

constexpr int MAXSUB = HTP_AUDIT_MAX_SUBSTEPS;
constexpr int MAXN = HTP_AUDIT_MAX_N;
constexpr int CHUNK_POSES = 256;     // poses staged in LDS at once (stages per chunk = CHUNK_POSES / substeps)
constexpr int ER = 7;                // edge record: unit normal (2), offset, start point (2), length, state
constexpr int TEO_MAX = MAXM * MAXE, TEB_MAX = MAXK * MAXE;
// fixed LDS (doubles): obstacle edges | body edges | polygon (first row, edge count) | poses (x, y, cos, sin);
// the raw halfspace rows live in the pose area until the edges are built
constexpr int L_EO = 0, L_EB = L_EO + ER * TEO_MAX, L_PI = L_EB + ER * TEB_MAX, L_POSE = L_PI + 2 * (MAXM + MAXK);
constexpr int L_FIXED = L_POSE + 4 * CHUNK_POSES;
static_assert(3 * (TEO_MAX + TEB_MAX) <= 4 * CHUNK_POSES, "raw rows fit the pose area");
// per-stage LDS (doubles): X 5N | U 2(N-1) | tau N-1 | h N-1 | |v| h N-1 | stage clearance keys N
HTP_HD inline int lds_stage_doubles(int N) { return 11 * N; }
static_assert((L_FIXED + 11 * MAXN) * 8 <= 65536, "LDS of the largest horizon fits a workgroup");

constexpr double INF = __builtin_huge_val();
constexpr double PAR_EPS = 1e-12;    // |n_s . u| below this: rows r and s are parallel
constexpr double LEN_EPS = 1e-9;     // an edge no longer than this is a redundant row touching a vertex
enum RowState { ROW_EDGE = 0, ROW_REDUNDANT = 1, ROW_UNBOUNDED = 2, ROW_ZERO = 3 };

struct Shape {   // launch-uniform
  int N, M, K, topt, S;
  int eo[MAXM], eb[MAXK], offo[MAXM], offb[MAXK];
  int TEo, TEb;
  int64_t stride;       // doubles between two problems' x rows
  int oU, oTAU;         // offsets of U and tau inside a row (X at 0)
  double margin_tol, dyn_tol, bound_tol, term_tol;
};

struct Batch {   // device or host pointers
  const double *traj, *obsA, *obsb, *bodyG, *bodyg, *params, *x;
  double* metrics;
  int32_t* worst;
  int32_t* flags;
  double* stage;   // nullable
};

HTP_HD inline void make_shape(Shape& s, const htp_obca_batch& in, const htp_obca_audit_opts& o) {
  s.N = in.N; s.M = in.M; s.K = in.K; s.topt = in.time_opt ? 1 : 0; s.S = o.substeps;
  s.TEo = 0; s.TEb = 0;
  for (int m = 0; m < MAXM; ++m) { s.eo[m] = 0; s.offo[m] = 0; }
  for (int k = 0; k < MAXK; ++k) { s.eb[k] = 0; s.offb[k] = 0; }
  for (int m = 0; m < in.M; ++m) { s.eo[m] = in.obs_edges[m]; s.offo[m] = s.TEo; s.TEo += s.eo[m]; }
  for (int k = 0; k < in.K; ++k) { s.eb[k] = in.body_edges[k]; s.offb[k] = s.TEb; s.TEb += s.eb[k]; }
  Dims D;
  make_dims(D, in.N, in.M, in.K, in.time_opt, in.obs_edges, in.body_edges);
  s.stride = D.n; s.oU = D.oU; s.oTAU = D.oTAU;
  s.margin_tol = o.margin_tol; s.dyn_tol = o.dyn_tol; s.bound_tol = o.bound_tol; s.term_tol = o.term_tol;
}

HTP_HD inline double dmax_(double a, double b) { return a > b ? a : b; }
HTP_HD inline double dmin_(double a, double b) { return a < b ? a : b; }
HTP_HD inline double dabs_(double a) { return a < 0.0 ? -a : a; }
HTP_HD inline bool nonfinite_(double v) { return !(v - v == 0.0); }

// order-preserving map double -> uint64 (for the per-stage minimum kept in LDS)
HTP_HD inline uint64_t key_of(double v) {
  uint64_t b;
  __builtin_memcpy(&b, &v, 8);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
HTP_HD inline double of_key(uint64_t k) {
  const uint64_t b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  double v;
  __builtin_memcpy(&v, &b, 8);
  return v;
}

struct State { double x, y, v, th, st; };

// kinematic_model (optimizer.py:42-52 of the restatement; R/obca_py/car_model_obca.py): f(state, control)
HTP_HD inline State kin(const State& s, double a, double w, double wb) {
  double sn, cs;
  hm::sincos(s.th, sn, cs);
  return State{s.v * cs, s.v * sn, a, s.v * hm::tan(s.st) / wb, w};
}

// one step of the NLP's integrator: midpoint rule with time_opt (optimizer.py:367-370), else Euler (:372-373)
HTP_HD inline State step(const State& s, double a, double w, double wb, double h, int topt) {
  State f = kin(s, a, w, wb);
  if (topt) {
    const double hh = 0.5 * h;
    const State m{s.x + hh * f.x, s.y + hh * f.y, s.v + hh * f.v, s.th + hh * f.th, s.st + hh * f.st};
    f = kin(m, a, w, wb);
  }
  return State{s.x + h * f.x, s.y + h * f.y, s.v + h * f.v, s.th + h * f.th, s.st + h * f.st};
}

// Row r of the polygon whose raw rows (ax, ay, b) are raw[3 * first .. 3 * (first + cnt)): its edge record.
HTP_HD inline void build_row(const double* raw, int first, int cnt, int r, double* rec) {
  const double ax = raw[3 * r], ay = raw[3 * r + 1], b = raw[3 * r + 2];
  const double nrm = sqrt(ax * ax + ay * ay);
  int state = ROW_EDGE;
  double nx = 0.0, ny = 0.0, bb = 0.0, lo = -INF, hi = INF;
  if (!(nrm > 0.0)) {
    state = ROW_ZERO;
  } else {
    nx = ax / nrm; ny = ay / nrm; bb = b / nrm;
    const double cx = bb * nx, cy = bb * ny, ux = -ny, uy = nx;
    bool empty = false;
    for (int s = first; s < first + cnt; ++s) {
      if (s == r) continue;
      const double sx = raw[3 * s], sy = raw[3 * s + 1], sb = raw[3 * s + 2];
      const double sn = sqrt(sx * sx + sy * sy);
      if (!(sn > 0.0)) continue;
      const double mx = sx / sn, my = sy / sn, mb = sb / sn;
      const double den = mx * ux + my * uy, num = mb - (mx * cx + my * cy);
      if (den > PAR_EPS) hi = dmin_(hi, num / den);
      else if (den < -PAR_EPS) lo = dmax_(lo, num / den);
      else if (num < -PAR_EPS) empty = true;
    }
    if (empty || hi < lo) state = ROW_REDUNDANT;
    else if (lo == -INF || hi == INF) state = ROW_UNBOUNDED;
    else if (hi - lo <= LEN_EPS) state = ROW_REDUNDANT;
  }
  const bool e = state == ROW_EDGE;
  rec[0] = nx; rec[1] = ny; rec[2] = bb;
  rec[3] = e ? bb * nx + lo * -ny : 0.0;
  rec[4] = e ? bb * ny + lo * nx : 0.0;
  rec[5] = e ? hi - lo : 0.0;
  rec[6] = (double)state;
}

// gap and squared distance of point (px, py) against the edge record e (same frame)
HTP_HD inline void point_edge(const double* e, double px, double py, double& g, double& d2) {
  const double nx = e[0], ny = e[1];
  const double pr = nx * px + ny * py - e[2];
  const double al = nx * (py - e[4]) - ny * (px - e[3]);
  const double ex = dmax_(dmax_(-al, al - e[5]), 0.0);
  g = dmin_(g, pr);
  d2 = dmin_(d2, pr * pr + ex * ex);
}

// Signed distance of obstacle polygon (edges Eo[0..no), world frame) and body polygon (edges Eb[0..nb), body
// frame) placed at (x, y) with heading cosine / sine (c, s).
HTP_HD inline double signed_distance(const double* Eo, int no, const double* Eb, int nb, double x, double y, double c,
                                     double s) {
  double sep = -INF, d2 = INF;
  for (int e = 0; e < no; ++e) {          // obstacle edges against the body's vertices, world frame
    const double* E = Eo + ER * e;
    double g = INF;
    for (int j = 0; j < nb; ++j) {
      const double vx = Eb[ER * j + 3], vy = Eb[ER * j + 4];
      point_edge(E, x + (c * vx - s * vy), y + (s * vx + c * vy), g, d2);
    }
    sep = dmax_(sep, g);
  }
  for (int e = 0; e < nb; ++e) {          // body edges against the obstacle's vertices, body frame
    const double* E = Eb + ER * e;
    double g = INF;
    for (int j = 0; j < no; ++j) {
      const double dx = Eo[ER * j + 3] - x, dy = Eo[ER * j + 4] - y;
      point_edge(E, c * dx + s * dy, c * dy - s * dx, g, d2);
    }
    sep = dmax_(sep, g);
  }
  return sep > 0.0 ? sqrt(d2) : sep;
}

// The serial lane of the test-only host build; the gfx950 wavefront is in htp_audit.hip.
struct HostLane {
  static constexpr int width = 1;
  int lane = 0;
  void sync() const {}
  double maxv(double v) const { return v; }
  double minv(double v) const { return v; }
  bool any(bool v) const { return v; }
  void min_key(double&, int&) const {}
  void lds_min(uint64_t* slot, uint64_t key) const { if (key < *slot) *slot = key; }
  void load_run(double* dst, const double* src, int n, bool& bad) const {
    for (int q = 0; q < n; ++q) { dst[q] = src[q]; bad = bad || nonfinite_(src[q]); }
  }
};

// One problem.  sl: L_FIXED doubles of LDS, dl: lds_stage_doubles(N) doubles of LDS (both 8-byte aligned).
template <class W>
HTP_HD inline void run_problem(const W& c, const Shape& sh, const Batch& b, int64_t p, double* sl, double* dl) {
  const int N = sh.N, M = sh.M, K = sh.K, S = sh.S, topt = sh.topt;
  double* X = dl;
  double* U = X + 5 * N;
  double* T = U + 2 * (N - 1);
  double* Hs = T + (N - 1);
  double* Ps = Hs + (N - 1);
  uint64_t* keys = (uint64_t*)(Ps + (N - 1));
  double* Eo = sl + L_EO;
  double* Eb = sl + L_EB;
  double* pinfo = sl + L_PI;
  double* pose = sl + L_POSE;
  double* rawO = pose;
  double* rawB = pose + 3 * TEO_MAX;
  const double* par = b.params + p * NPARAM;
  const double* tr = b.traj + p * (int64_t)N * NS;
  const double NaN = __builtin_nan("");

  // ---- the doubles read: X, U (one run), tau; halfspace rows; the parameters; the init and end states
  bool bad = false;
  const double* xr = b.x + p * sh.stride;
  c.load_run(X, xr, 5 * N + 2 * (N - 1), bad);
  if (topt) c.load_run(T, xr + sh.oTAU, N - 1, bad);
  for (int r = c.lane; r < sh.TEo; r += c.width) {
    const double ax = b.obsA[(p * sh.TEo + r) * 2], ay = b.obsA[(p * sh.TEo + r) * 2 + 1], bb = b.obsb[p * sh.TEo + r];
    rawO[3 * r] = ax; rawO[3 * r + 1] = ay; rawO[3 * r + 2] = bb;
    bad = bad || nonfinite_(ax) || nonfinite_(ay) || nonfinite_(bb);
  }
  for (int r = c.lane; r < sh.TEb; r += c.width) {
    const double ax = b.bodyG[(p * sh.TEb + r) * 2], ay = b.bodyG[(p * sh.TEb + r) * 2 + 1], bb = b.bodyg[p * sh.TEb + r];
    rawB[3 * r] = ax; rawB[3 * r + 1] = ay; rawB[3 * r + 2] = bb;
    bad = bad || nonfinite_(ax) || nonfinite_(ay) || nonfinite_(bb);
  }
  const double dT = par[P_DT], wb = par[P_WHEELBASE], dmin = par[P_DMIN];
  const double vmax = dabs_(par[P_MAXV]), smax = dabs_(par[P_MAXSTEER]);
  const double amax = dabs_(par[P_MAXACC]), wmax = dabs_(par[P_MAXSR]);
  const double xlo = par[P_XLO], xhi = par[P_XHI], ylo = par[P_YLO], yhi = par[P_YHI];
  bad = bad || nonfinite_(dT) || nonfinite_(wb) || nonfinite_(dmin) || nonfinite_(vmax) || nonfinite_(smax) ||
        nonfinite_(amax) || nonfinite_(wmax) || xlo != xlo || xhi != xhi || ylo != ylo || yhi != yhi;   // bounds may be infinite
  for (int k = 0; k < NS; ++k) bad = bad || nonfinite_(tr[k]) || nonfinite_(tr[NS * (N - 1) + k]);
  bad = c.any(bad);
  c.sync();
  if (bad) {
    if (b.stage)
      for (int i = c.lane; i < N; i += c.width) b.stage[p * N + i] = NaN;
    if (c.lane == 0) {
      for (int k = 0; k < HTP_AUDIT_NMETRIC; ++k) b.metrics[p * HTP_AUDIT_NMETRIC + k] = NaN;
      for (int k = 0; k < 4; ++k) b.worst[p * 4 + k] = -1;
      b.flags[p] = HTP_AUDIT_NONFINITE;
    }
    return;
  }

  // ---- polygons: one row per lane, then one polygon per lane compacts its edges in place
  for (int r = c.lane; r < sh.TEo + sh.TEb; r += c.width) {
    const bool body = r >= sh.TEo;
    const int rr = body ? r - sh.TEo : r;
    int first = 0, cnt = 0;
    if (body) {
      for (int k = 0; k < K; ++k)
        if (rr >= sh.offb[k] && rr < sh.offb[k] + sh.eb[k]) { first = sh.offb[k]; cnt = sh.eb[k]; }
    } else {
      for (int m = 0; m < M; ++m)
        if (rr >= sh.offo[m] && rr < sh.offo[m] + sh.eo[m]) { first = sh.offo[m]; cnt = sh.eo[m]; }
    }
    build_row(body ? rawB : rawO, first, cnt, rr, (body ? Eb : Eo) + ER * rr);
  }
  c.sync();
  for (int j = c.lane; j < M + K; j += c.width) {
    const bool body = j >= M;
    const int first = body ? sh.offb[j - M] : sh.offo[j], cnt = body ? sh.eb[j - M] : sh.eo[j];
    double* E = (body ? Eb : Eo) + ER * first;
    int n = 0;
    bool pb = false;
    for (int e = 0; e < cnt; ++e) {
      const int st = (int)E[ER * e + 6];
      if (st == ROW_EDGE) {
        for (int q = 0; q < ER; ++q) E[ER * n + q] = E[ER * e + q];
        ++n;
      } else if (st != ROW_REDUNDANT) {
        pb = true;
      }
    }
    pinfo[2 * j] = (double)first;
    pinfo[2 * j + 1] = (pb || n < 3) ? -1.0 : (double)n;
  }
  c.sync();
  bool polybad = false;
  for (int j = 0; j < M + K; ++j) polybad = polybad || pinfo[2 * j + 1] < 0.0;

  // ---- stages: dynamics defect (optimizer.py:364-377), step lengths; bounds (:292-354); init / end miss
  double defect = 0.0, excess = 0.0, imiss = 0.0, tmiss = 0.0;
  for (int i = c.lane; i < N - 1; i += c.width) {
    const State s{X[5 * i], X[5 * i + 1], X[5 * i + 2], X[5 * i + 3], X[5 * i + 4]};
    const double h = topt ? dT * T[i] : dT;
    const State f = step(s, U[2 * i], U[2 * i + 1], wb, h, topt);
    const double* xn = X + 5 * (i + 1);
    defect = dmax_(defect, dabs_(xn[0] - f.x));
    defect = dmax_(defect, dabs_(xn[1] - f.y));
    defect = dmax_(defect, dabs_(xn[2] - f.v));
    defect = dmax_(defect, dabs_(xn[3] - f.th));
    defect = dmax_(defect, dabs_(xn[4] - f.st));
    Hs[i] = h;
    Ps[i] = dabs_(s.v) * h;
  }
  const double twopi = 6.283185307179586;
  for (int q = c.lane; q < 5 * N; q += c.width) {
    const int k = q % NS;
    const double lo = k == 0 ? xlo : k == 1 ? ylo : k == 2 ? -vmax : k == 3 ? -twopi : -smax;
    const double hi = k == 0 ? xhi : k == 1 ? yhi : k == 2 ? vmax : k == 3 ? twopi : smax;
    excess = dmax_(excess, dmax_(lo - X[q], X[q] - hi));
  }
  for (int q = c.lane; q < 2 * (N - 1); q += c.width) {
    const double hi = (q & 1) ? wmax : amax;
    excess = dmax_(excess, dmax_(-hi - U[q], U[q] - hi));
  }
  if (topt)
    for (int q = c.lane; q < N - 1; q += c.width) excess = dmax_(excess, dmax_(0.05 / dT - T[q], T[q] - 1.0));
  for (int k = c.lane; k < NS; k += c.width) {
    imiss = dmax_(imiss, dabs_(X[k] - tr[k]));
    tmiss = dmax_(tmiss, dabs_(X[NS * (N - 1) + k] - tr[NS * (N - 1) + k]));
  }
  defect = c.maxv(defect);
  excess = c.maxv(excess);
  imiss = c.maxv(imiss);
  tmiss = c.maxv(tmiss);

  // ---- clearance: chunks of stages; poses into LDS, then lanes strided over (pose, obstacle, body)
  double best = INF, node = INF;
  int bidx = 0x7fffffff;
  if (!polybad) {
    for (int i = c.lane; i < N; i += c.width) keys[i] = ~(uint64_t)0;
    const int CS = CHUNK_POSES / S, MK = M * K;
    for (int i0 = 0; i0 < N; i0 += CS) {
      const int ni = (N - i0 < CS) ? N - i0 : CS;
      c.sync();   // the previous chunk's poses (or the raw rows) are no longer read
      for (int t = c.lane; t < ni * S; t += c.width) {
        const int i = i0 + t / S, q = t % S;
        State s{X[5 * i], X[5 * i + 1], X[5 * i + 2], X[5 * i + 3], X[5 * i + 4]};
        if (q > 0 && i < N - 1) s = step(s, U[2 * i], U[2 * i + 1], wb, Hs[i] * (double)q / (double)S, topt);
        double sn, cs;
        hm::sincos(s.th, sn, cs);
        pose[4 * t] = s.x; pose[4 * t + 1] = s.y; pose[4 * t + 2] = cs; pose[4 * t + 3] = sn;
      }
      c.sync();
      for (int w = c.lane; w < ni * S * MK; w += c.width) {
        const int t = w / MK, mk = w % MK, m = mk / K, k = mk % K;
        const int i = i0 + t / S, q = t % S;
        if (q > 0 && i == N - 1) continue;   // the last node starts no interval
        const double* P = pose + 4 * t;
        const double d = signed_distance(Eo + ER * (int)pinfo[2 * m], (int)pinfo[2 * m + 1],
                                         Eb + ER * (int)pinfo[2 * (M + k)], (int)pinfo[2 * (M + k) + 1],
                                         P[0], P[1], P[2], P[3]);
        const int idx = i0 * S * MK + w;   // = ((i S + q) M + m) K + k, ascending per lane
        if (d < best) { best = d; bidx = idx; }
        if (q == 0) node = dmin_(node, d);
        c.lds_min(keys + i, key_of(d));
      }
    }
    c.sync();
    c.min_key(best, bidx);
    node = c.minv(node);
    if (b.stage)
      for (int i = c.lane; i < N; i += c.width) b.stage[p * N + i] = of_key(keys[i]);
  } else if (b.stage) {
    for (int i = c.lane; i < N; i += c.width) b.stage[p * N + i] = NaN;
  }

  c.sync();
  if (c.lane == 0) {
    double plen = 0.0, ttime = 0.0;
    for (int i = 0; i < N - 1; ++i) { plen += Ps[i]; ttime += Hs[i]; }
    double* mt = b.metrics + p * HTP_AUDIT_NMETRIC;
    mt[HTP_AUDIT_CLEARANCE] = polybad ? NaN : best;
    mt[HTP_AUDIT_CLEARANCE_NODE] = polybad ? NaN : node;
    mt[HTP_AUDIT_DYN_DEFECT] = defect;
    mt[HTP_AUDIT_BOUND_EXCESS] = excess;
    mt[HTP_AUDIT_INIT_MISS] = imiss;
    mt[HTP_AUDIT_TERM_MISS] = tmiss;
    mt[HTP_AUDIT_PATH_LENGTH] = plen;
    mt[HTP_AUDIT_TOTAL_TIME] = ttime;
    int32_t* wo = b.worst + p * 4;
    int fl = 0;
    if (polybad) {
      fl |= HTP_AUDIT_BAD_POLYTOPE;
      wo[0] = wo[1] = wo[2] = wo[3] = -1;
    } else {
      const int MK = M * K, t = bidx / MK, mk = bidx % MK;
      wo[0] = t / S; wo[1] = t % S; wo[2] = mk / K; wo[3] = mk % K;
      if (best < 0.0) fl |= HTP_AUDIT_COLLISION;
      if (best < dmin - sh.margin_tol) fl |= HTP_AUDIT_MARGIN;
    }
    if (defect > sh.dyn_tol) fl |= HTP_AUDIT_DYNAMICS;
    if (excess > sh.bound_tol) fl |= HTP_AUDIT_BOUNDS;
    if (sh.term_tol > 0.0 && tmiss > sh.term_tol) fl |= HTP_AUDIT_TERMINAL;
    b.flags[p] = fl;
  }
}

}  // namespace audit
}  // namespace htp

#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC pop_options
#endif
