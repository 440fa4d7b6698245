// Uniform-time sampling of one solved OBCA trajectory (FORM 0, R/obca_py/optimizer.py layout): the node times and
// arc lengths of the NLP's own grid (h_i = dT tau_i), then one row (t, x, y, v, theta, steer, accel, steer_rate,
// curvature, arc) every dt, from the audit's integrator (audit_core.h step) started at the node that opens the
// sample's interval, and one final row at the stored last node.  One problem per 64-lane wavefront on gfx950
// (htp_timeline.hip) or a single serial lane (timeline_hostsim.cpp, tests only); one __host__ __device__ source,
// so both produce the same doubles:
//   - no contraction (pragma below) and the planner libm (htp_libm.h) for sin, cos and tan;
//   - the node times and arc lengths are added left to right by one lane (numpy.cumsum's doubles, and the order
//     in which the audit adds its total time and path length); no scan reassociates them;
//   - a sample's time is the product k dt, never an accumulated sum, and the number of samples is corrected
//     against those products, so a duration that is a multiple of dt gives no duplicate last row.
// Only X, U and tau of the decision vector and the dT and wheelbase parameters are read.
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
namespace timeline {

constexpr int NCOL = HTP_TIMELINE_NCOL;
constexpr int MAXN = HTP_TIMELINE_MAX_N;
constexpr int CHUNK = 64;             // rows staged in LDS at once: one per lane
constexpr int L_FIXED = CHUNK * NCOL; // fixed LDS (doubles): the row tile
enum Col { C_T = 0, C_X, C_Y, C_V, C_TH, C_ST, C_ACC, C_SR, C_CURV, C_ARC };
static_assert(C_ARC + 1 == NCOL, "htp.h timeline columns");
static_assert(MAXN == audit::MAXN, "the audit's horizon limit");
// per-stage LDS (doubles): X 5N | U 2(N-1) | tau, then h N-1 | node times N | node arc lengths N
HTP_HD inline int lds_stage_doubles(int N) { return 10 * N; }
static_assert((L_FIXED + 10 * MAXN) * 8 <= 65536, "LDS of the largest horizon fits a workgroup");
constexpr double MAX_QUOTIENT = 1073741824.0;   // T / dt must stay below 2^30: row numbers are int32

struct Shape {   // launch-uniform
  int N, topt, cap;
  int64_t stride;   // doubles between two problems' x rows
  int oTAU;         // offset of tau inside a row (X at 0, U behind X)
  double dt;
};

struct Batch {   // device or host pointers
  const double *params, *x;
  double* rows;
  int32_t* stage;   // nullable
  int32_t* count;
  int32_t* flags;
  double* duration;   // nullable
};

HTP_HD inline void make_shape(Shape& s, const htp_obca_batch& in, const htp_obca_timeline_opts& o) {
  s.N = in.N; s.topt = in.time_opt ? 1 : 0; s.cap = o.cap; s.dt = o.dt;
  Dims D;
  make_dims(D, in.N, in.M, in.K, in.time_opt, in.obs_edges, in.body_edges);
  s.stride = D.n; s.oTAU = D.oTAU;
}

// The serial lane of the test-only host build; the gfx950 wavefront is in htp_timeline.hip.
struct HostLane : audit::HostLane {
  void store_run(double* dst, const double* src, int n) const {
    for (int q = 0; q < n; ++q) dst[q] = src[q];
  }
};

// count 0, no row: the problem is not sampled
template <class W>
HTP_HD inline void reject(const W& c, const Batch& b, int64_t p, int flag, double duration) {
  if (c.lane == 0) {
    b.count[p] = 0;
    b.flags[p] = flag;
    if (b.duration) b.duration[p] = duration;
  }
}

// One problem.  tile: L_FIXED doubles of LDS, dl: lds_stage_doubles(N) doubles of LDS (both 16-byte aligned).
template <class W>
HTP_HD inline void run_problem(const W& c, const Shape& sh, const Batch& b, int64_t p, double* tile, double* dl) {
  using audit::State;
  const int N = sh.N, topt = sh.topt, cap = sh.cap;
  const double dt = sh.dt;
  double* X = dl;
  double* U = X + 5 * N;
  double* H = U + 2 * (N - 1);
  double* Tn = H + (N - 1);
  double* An = Tn + N;
  const double* par = b.params + p * NPARAM;
  const double NaN = __builtin_nan("");

  // ---- the doubles read: X, U (one run), tau; dT and the wheelbase
  bool bad = false;
  const double* xr = b.x + p * sh.stride;
  c.load_run(X, xr, 5 * N + 2 * (N - 1), bad);
  if (topt) c.load_run(H, xr + sh.oTAU, N - 1, bad);
  const double dT = par[P_DT], wb = par[P_WHEELBASE];
  bad = bad || audit::nonfinite_(dT) || audit::nonfinite_(wb);
  bad = c.any(bad);
  c.sync();
  if (bad) { reject(c, b, p, HTP_TIMELINE_NONFINITE, NaN); return; }

  // ---- step lengths, then the node times and arc lengths: serial sums by one lane
  bool nonpos = false;
  for (int i = c.lane; i < N - 1; i += c.width) {
    const double h = topt ? dT * H[i] : dT;
    H[i] = h;
    nonpos = nonpos || !(h > 0.0);
  }
  nonpos = c.any(nonpos);
  c.sync();
  if (nonpos) { reject(c, b, p, HTP_TIMELINE_BAD_TIME, NaN); return; }
  if (c.lane == 0) {
    double t = 0.0, a = 0.0;
    Tn[0] = 0.0; An[0] = 0.0;
    for (int i = 0; i < N - 1; ++i) {
      const double h = H[i];
      const double ds = audit::dabs_(X[5 * i + 2]) * h;
      t += h; a += ds;
      Tn[i + 1] = t; An[i + 1] = a;
    }
  }
  c.sync();
  const double T = Tn[N - 1];
  const double quot = T / dt;
  if (!(quot < MAX_QUOTIENT)) { reject(c, b, p, HTP_TIMELINE_BAD_TIME, T); return; }

  // ---- regular rows k = 0 .. n-1: n = the smallest n with fl(n dt) >= T (the quotient is only a first guess)
  int n = (int)quot;
  while (n > 0 && (double)(n - 1) * dt >= T) --n;
  while ((double)n * dt < T) ++n;
  const int need = n + 1;
  const int nw = need < cap ? need : cap;

  double* out = b.rows + p * (int64_t)cap * NCOL;
  for (int r0 = 0; r0 < nw; r0 += CHUNK) {
    const int nr = nw - r0 < CHUNK ? nw - r0 : CHUNK;
    c.sync();   // the previous chunk's tile is no longer read
    for (int j = c.lane; j < nr; j += c.width) {
      const int r = r0 + j;
      double* row = tile + NCOL * j;
      int i;
      if (r < n) {
        const double s = (double)r * dt;
        int lo = 0, hi = N - 2;          // the largest i in 0..N-2 with t_i <= s (t_0 = 0 <= s)
        while (lo < hi) {
          const int mid = (lo + hi + 1) >> 1;
          if (Tn[mid] <= s) lo = mid; else hi = mid - 1;
        }
        i = lo;
        const double tau = s - Tn[i];
        const State x0{X[5 * i], X[5 * i + 1], X[5 * i + 2], X[5 * i + 3], X[5 * i + 4]};
        const State f = audit::step(x0, U[2 * i], U[2 * i + 1], wb, tau, topt);
        row[C_T] = s; row[C_X] = f.x; row[C_Y] = f.y; row[C_V] = f.v; row[C_TH] = f.th; row[C_ST] = f.st;
        row[C_ACC] = U[2 * i]; row[C_SR] = U[2 * i + 1];
        row[C_CURV] = hm::tan(f.st) / wb;
        row[C_ARC] = An[i] + audit::dabs_(x0.v) * tau;
      } else {                           // the final row: the stored last node
        i = N - 1;
        const double* xn = X + 5 * i;
        row[C_T] = T; row[C_X] = xn[0]; row[C_Y] = xn[1]; row[C_V] = xn[2]; row[C_TH] = xn[3]; row[C_ST] = xn[4];
        row[C_ACC] = U[2 * (N - 2)]; row[C_SR] = U[2 * (N - 2) + 1];
        row[C_CURV] = hm::tan(xn[4]) / wb;
        row[C_ARC] = An[i];
      }
      if (b.stage) b.stage[p * (int64_t)cap + r] = i;
    }
    c.sync();
    c.store_run(out + (int64_t)r0 * NCOL, tile, nr * NCOL);
  }
  if (c.lane == 0) {
    b.count[p] = need;
    b.flags[p] = need > cap ? HTP_TIMELINE_TRUNCATED : 0;
    if (b.duration) b.duration[p] = T;
  }
}

}  // namespace timeline
}  // namespace htp

#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC pop_options
#endif
