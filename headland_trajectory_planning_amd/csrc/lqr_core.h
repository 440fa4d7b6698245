// Time-varying LQR about one solved OBCA trajectory (include/htp.h holds the definition): the NLP's own integrator
// linearised at every stage, a backward Riccati pass for the gains K_i and the cost-to-go P_i, a forward covariance
// pass through the closed loop for the one-sigma tube, and the control authority the limits leave beside the
// reference.  One problem per 64-lane wavefront on gfx950 (htp_lqr.hip) or a single serial lane (lqr_hostsim.cpp,
// tests only); one __host__ __device__ source, so both produce the same doubles:
//   - no contraction (pragma below) and the planner libm (htp_libm.h);
//   - the linearisation of a stage is one lane's serial work;
//   - inside a stage of either recursion a lane owns one entry of a 5 x 5, 2 x 5 or 5 x 2 product and sums its inner
//     product over k = 0..4 from left to right; nothing is ever summed across lanes;
//   - the running maxima and minima (with their stage, ties to the lowest) are kept by one lane per quantity, in
//     ascending stage order.
// Every step of a stage reads what the step before it left in LDS and writes somewhere else, so the serial lane of
// the host build, which walks the entries of a step one after the other, sees what the 64 lanes see.
// The kinematic model, the state and the helpers are the audit's (audit_core.h, included unedited).
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
namespace lqr {

constexpr int MAXN = HTP_LQR_MAX_N;
constexpr int NMET = HTP_LQR_NMETRIC, NTUBE = HTP_LQR_NTUBE, NGAIN = HTP_LQR_NGAIN, NCTG = HTP_LQR_NCTG;
constexpr int NLIN = HTP_LQR_NLIN;
constexpr int CHUNK = 64;            // stages linearised into the LDS tile at once
// tile row of one stage: A rows (x, y, theta) x columns (v, theta, steer) [9] | B (x, a), (y, a), (theta, a),
// (theta, w) [4] | h | cos theta_i | sin theta_i | pad (an odd stride: sixteen lanes' 8-byte stores of one entry
// fall on distinct banks).  Rows v and steer of A are unit rows, columns x and y unit columns; B (v, a) = B (steer,
// w) = h and the rest of B is 0.
constexpr int TR = 17, T_B = 9, T_H = 13, T_C = 14, T_S = 15;
// fixed LDS (doubles): tile | gains of the chunk | P or Sigma | its unsymmetrised successor | P A or Acl Sigma | P B |
// S and B' P A | A - B K | K Sigma | running extremes (value, stage) | largest |K| per entry | cos, sin of the last
// node, sigma_lat there
constexpr int L_TILE = 0, L_KT = L_TILE + TR * CHUNK, L_P = L_KT + NGAIN * CHUNK, L_RAW = L_P + 26, L_PA = L_RAW + 26;
constexpr int L_PB = L_PA + 26, L_SG = L_PB + 10, L_ACL = L_SG + 14, L_KS = L_ACL + 26, L_RUN = L_KS + 10;
constexpr int NRUN = 7;              // max s_lat, max s_lon, max s_theta, min ratio acc, rate, steer, speed
constexpr int L_KM = L_RUN + 2 * NRUN, L_CS = L_KM + NGAIN, L_FIXED = L_CS + 4;
static_assert(L_FIXED % 2 == 0, "the per-stage LDS behind it stays 16-byte aligned");
static_assert(MAXN == audit::MAXN, "the audit's horizon limit");
// per-stage LDS (doubles): X 5N | U 2(N-1) | tau, then h N-1
HTP_HD inline int lds_stage_doubles(int N) { return 8 * N; }
static_assert((L_FIXED + 8 * MAXN) * 8 <= 65536, "LDS of the largest horizon fits a workgroup");
constexpr double INF = audit::INF;
enum Run { R_SLAT = 0, R_SLON, R_STH, R_ACC, R_RATE, R_STEER, R_SPEED };
static_assert(HTP_LQR_NMETRIC == 10 && HTP_LQR_NTUBE == 7 && HTP_LQR_NGAIN == 10 && HTP_LQR_NCTG == 15 &&
              HTP_LQR_NLIN == 35, "htp.h lqr sizes");

// a diagonal (lon, lat, v, th, st) in the frame of a node
struct Diag { double lon, lat, v, th, st; };

struct Shape {   // launch-uniform
  int N, topt;
  int64_t stride;   // doubles between two problems' x rows
  int oTAU;         // offset of tau inside a row (X at 0, U behind X)
  Diag q, var0, w;  // state weights, initial variances (sig0 squared), noise intensities
  double qf, r_a, r_w;
  double k_sigma;
};

struct Batch {   // device or host pointers
  const double *params, *x;
  double* gains;
  double* tube;
  double* metrics;
  int32_t* worst;
  int32_t* flags;
  double* ctg;   // nullable
  double* lin;   // nullable
};

HTP_HD inline void make_shape(Shape& s, const htp_obca_batch& in, const htp_obca_lqr_opts& o) {
  s.N = in.N; s.topt = in.time_opt ? 1 : 0;
  Dims D;
  make_dims(D, in.N, in.M, in.K, in.time_opt, in.obs_edges, in.body_edges);
  s.stride = D.n; s.oTAU = D.oTAU;
  s.q = Diag{o.q_lon, o.q_lat, o.q_v, o.q_th, o.q_st};
  s.var0 = Diag{o.sig0_lon * o.sig0_lon, o.sig0_lat * o.sig0_lat, o.sig0_v * o.sig0_v, o.sig0_th * o.sig0_th,
                o.sig0_st * o.sig0_st};
  s.w = Diag{o.w_lon, o.w_lat, o.w_v, o.w_th, o.w_st};
  s.qf = o.qf; s.r_a = o.r_a; s.r_w = o.r_w;
  s.k_sigma = o.k_sigma;
}

// The serial lane of the test-only host build; the gfx950 wavefront is in htp_lqr.hip.
struct HostLane : audit::HostLane {
  void gsync() const {}
};

// stage (X_i, U_i, h) -> its tile row.  The Jacobian is evaluated at X_i and, with time_opt, at the midpoint m by
// one loop body, so that the libm has one call site each and everything is inlined into the kernel (a call would
// cost the kernel a stack).
HTP_HD __attribute__((always_inline)) inline void linearise(const double* X5, double a, double w, double wb, double h,
                                                            int topt, double* t) {
  double v = X5[2], th = X5[3], st = X5[4];
  const double hh = 0.5 * h;
  // Fx at the point: rows (x, y, theta) x columns (v, theta, steer) = (g0, g1, 0 | g3, g4, 0 | g6, 0, g8);
  // f6, f8: row theta of Fx(X_i)
  double g0 = 0.0, g1 = 0.0, g3 = 0.0, g4 = 0.0, g6 = 0.0, g8 = 0.0, f6 = 0.0, f8 = 0.0;
#pragma GCC unroll 1
  for (int pass = 0; pass <= topt; ++pass) {
    double sn, cs;
    hm::sincos(th, sn, cs);
    const double cd = hm::cos(st), tn = hm::tan(st);
    g0 = cs; g1 = -v * sn; g3 = sn; g4 = v * cs; g6 = tn / wb; g8 = v / (wb * (cd * cd));
    if (pass == 0) {
      f6 = g6; f8 = g8;
      t[T_C] = cs; t[T_S] = sn;
      // m = X_i + (h / 2) f(X_i, U_i), its v, theta and steer (x and y enter no Jacobian)
      const double mv = v + hh * a, mth = th + hh * (v * tn / wb), mst = st + hh * w;
      v = mv; th = mth; st = mst;
    }
  }
  t[T_H] = h; t[TR - 1] = 0.0;
  if (!topt) {                         // A = I + h Fx(X_i), B = h Fu
    t[0] = h * g0; t[1] = h * g1; t[2] = 0.0;
    t[3] = h * g3; t[4] = h * g4; t[5] = 0.0;
    t[6] = h * g6; t[7] = 1.0; t[8] = h * g8;
    t[T_B] = 0.0; t[T_B + 1] = 0.0; t[T_B + 2] = 0.0; t[T_B + 3] = 0.0;
    return;
  }
  // G = Fx(m) (I + (h / 2) Fx(X_i)): column theta of Fx(m) meets row theta of Fx(X_i) = (f6, 0, f8)
  t[0] = h * (g0 + g1 * (hh * f6)); t[1] = h * g1; t[2] = h * (g1 * (hh * f8));
  t[3] = h * (g3 + g4 * (hh * f6)); t[4] = h * g4; t[5] = h * (g4 * (hh * f8));
  t[6] = h * g6; t[7] = 1.0; t[8] = h * g8;
  // B = h (Fu + (h / 2) Fx(m) Fu): column a is column v of Fx(m), column w its column steer
  t[T_B] = h * (hh * g0); t[T_B + 1] = h * (hh * g3); t[T_B + 2] = h * (hh * g6); t[T_B + 3] = h * (hh * g8);
}

HTP_HD inline double a_at(const double* t, int r, int c) {
  const int rr = r == 0 ? 0 : (r == 1 ? 1 : (r == 3 ? 2 : -1));
  if (rr < 0 || c < 2) return r == c ? 1.0 : 0.0;
  return t[3 * rr + (c - 2)];   // (theta, theta) is stored as 1
}
HTP_HD inline double b_at(const double* t, int r, int c) {   // c: 0 = a, 1 = w
  if (r == 2) return c == 0 ? t[T_H] : 0.0;
  if (r == 4) return c == 1 ? t[T_H] : 0.0;
  if (r == 3) return t[T_B + 2 + c];
  return c == 0 ? t[T_B + r] : 0.0;
}
// Q, W or Sigma_0 in world coordinates: the diagonal (lon, lat, v, th, st) in the frame of heading (cs, sn)
HTP_HD inline double rot_at(const Diag& d, double cs, double sn, int r, int c) {
  if (r < 2 && c < 2) {
    if (r != c) return (cs * sn) * (d.lon - d.lat);
    return r == 0 ? (cs * cs) * d.lon + (sn * sn) * d.lat : (sn * sn) * d.lon + (cs * cs) * d.lat;
  }
  return r != c ? 0.0 : (r == 2 ? d.v : (r == 3 ? d.th : d.st));
}
HTP_HD inline double root_(double v) { return sqrt(v < 0.0 ? 0.0 : v); }
HTP_HD inline double ratio_(double head, double sig) { return (sig == 0.0 && head >= 0.0) ? INF : head / sig; }

// row-major index pairs of the upper triangle of a 5 x 5 matrix
HTP_HD inline void tri_at(int e, int& r, int& c) {
  r = e < 5 ? 0 : (e < 9 ? 1 : (e < 12 ? 2 : (e < 14 ? 3 : 4)));
  c = e - (r == 0 ? 0 : (r == 1 ? 4 : (r == 2 ? 7 : (r == 3 ? 9 : 10))));
}

template <class W>
HTP_HD inline void reject(const W& c, const Batch& b, int64_t p, int flag) {
  const double NaN = __builtin_nan("");
  for (int q = c.lane; q < NMET; q += c.width) b.metrics[p * NMET + q] = NaN;
  if (c.lane == 0) b.flags[p] = flag;
}

// One problem.  sl: L_FIXED doubles of LDS, dl: lds_stage_doubles(N) doubles of LDS (both 16-byte aligned).
template <class W>
HTP_HD inline void run_problem(const W& c, const Shape& sh, const Batch& b, int64_t p, double* sl, double* dl) {
  using audit::dabs_;
  using audit::nonfinite_;
  const int N = sh.N, topt = sh.topt, NST = sh.N - 1;
  double* X = dl;
  double* U = X + 5 * N;
  double* H = U + 2 * (N - 1);
  double* tile = sl + L_TILE;
  double* KT = sl + L_KT;
  double* P = sl + L_P;
  double* RAW = sl + L_RAW;
  double* PA = sl + L_PA;
  double* PB = sl + L_PB;
  double* SG = sl + L_SG;
  double* ACL = sl + L_ACL;
  double* KS = sl + L_KS;
  double* RUN = sl + L_RUN;
  double* KM = sl + L_KM;
  double* CSN = sl + L_CS;
  const double* par = b.params + p * NPARAM;
  const double NaN = __builtin_nan("");
  double* gains = b.gains + p * NST * NGAIN;
  double* tube = b.tube + p * N * NTUBE;
  double* ctg = b.ctg ? b.ctg + p * N * NCTG : nullptr;
  double* lin = b.lin ? b.lin + p * NST * NLIN : nullptr;

  // ---- the doubles read: X, U (one run), tau; the six parameters
  bool bad = false;
  const double* xr = b.x + p * sh.stride;
  c.load_run(X, xr, 5 * N + 2 * (N - 1), bad);
  if (topt) c.load_run(H, xr + sh.oTAU, N - 1, bad);
  const double dT = par[P_DT], wb = par[P_WHEELBASE], smax = par[P_MAXSTEER], vmax = par[P_MAXV];
  const double amax = par[P_MAXACC], wmax = par[P_MAXSR];
  bad = bad || nonfinite_(dT) || nonfinite_(wb) || nonfinite_(smax) || nonfinite_(vmax) || nonfinite_(amax) ||
        nonfinite_(wmax);
  bad = c.any(bad);
  c.sync();
  if (bad) { reject(c, b, p, HTP_LQR_NONFINITE); return; }
  bool nonpos = false;
  for (int i = c.lane; i < NST; i += c.width) {
    const double h = topt ? dT * H[i] : dT;
    H[i] = h;
    nonpos = nonpos || !(h > 0.0);
  }
  nonpos = c.any(nonpos);
  c.sync();
  const bool badlim = !(wb > 0.0) || !(smax > 0.0) || !(vmax > 0.0) || !(amax > 0.0) || !(wmax > 0.0);
  if (nonpos || badlim) {
    reject(c, b, p, (nonpos ? HTP_LQR_BAD_TIME : 0) | (badlim ? HTP_LQR_BAD_LIMIT : 0));
    return;
  }
  const double Rd0 = sh.r_a / (amax * amax), Rd1 = sh.r_w / (wmax * wmax);

  // ---- backward pass: P_{N-1} = qf Q_{N-1}; chunks of stages from the last one down
  {
    double sn, cs;
    hm::sincos(X[5 * (N - 1) + 3], sn, cs);
    if (c.lane == 0) { CSN[0] = cs; CSN[1] = sn; }
    for (int e = c.lane; e < 25; e += c.width) P[e] = sh.qf * rot_at(sh.q, cs, sn, e / 5, e % 5);
    for (int e = c.lane; e < 2 * NRUN; e += c.width) RUN[e] = (e & 1) ? -1.0 : ((e >> 1) >= R_ACC ? INF : -INF);
    for (int e = c.lane; e < NGAIN; e += c.width) KM[e] = 0.0;
  }
  c.sync();
  if (ctg)
    for (int e = c.lane; e < NCTG; e += c.width) {
      int r, q;
      tri_at(e, r, q);
      ctg[(N - 1) * NCTG + e] = P[5 * r + q];
    }
  bool dead = false;                   // wave-uniform: SINGULAR met, the rest of the pass writes NaN
  const int nchunk = (NST + CHUNK - 1) / CHUNK;
  for (int ch = nchunk - 1; ch >= 0; --ch) {
    const int i0 = ch * CHUNK, nr = NST - i0 < CHUNK ? NST - i0 : CHUNK;
    c.sync();   // the previous chunk's tile and gains are no longer read
    for (int j = c.lane; j < nr; j += c.width) {
      const int i = i0 + j;
      linearise(X + 5 * i, U[2 * i], U[2 * i + 1], wb, H[i], topt, tile + TR * j);
    }
    c.sync();
    if (lin)
      for (int t = c.lane; t < nr * NLIN; t += c.width) {
        const int j = t / NLIN, e = t % NLIN;
        const double* tj = tile + TR * j;
        lin[(int64_t)i0 * NLIN + t] = e < 25 ? a_at(tj, e / 5, e % 5) : b_at(tj, (e - 25) / 2, (e - 25) % 2);
      }
    for (int j = nr - 1; j >= 0; --j) {
      const int i = i0 + j;
      const double* tj = tile + TR * j;
      if (!dead) {
        // P A (25 lanes) and P B (10 lanes)
        for (int e = c.lane; e < 35; e += c.width) {
          if (e < 25) {
            const int r = e / 5, q = e % 5;
            double s = P[5 * r] * a_at(tj, 0, q);
            for (int k = 1; k < 5; ++k) s += P[5 * r + k] * a_at(tj, k, q);
            PA[e] = s;
          } else {
            const int r = (e - 25) / 2, q = (e - 25) % 2;
            double s = P[5 * r] * b_at(tj, 0, q);
            for (int k = 1; k < 5; ++k) s += P[5 * r + k] * b_at(tj, k, q);
            PB[e - 25] = s;
          }
        }
        c.sync();
        // S = R + B' (P B) (4 lanes) and G = B' (P A) (10 lanes)
        for (int e = c.lane; e < 14; e += c.width) {
          if (e < 4) {
            const int r = e / 2, q = e % 2;
            double s = b_at(tj, 0, r) * PB[q];
            for (int k = 1; k < 5; ++k) s += b_at(tj, k, r) * PB[2 * k + q];
            SG[e] = (r == q ? (r == 0 ? Rd0 : Rd1) : 0.0) + s;
          } else {
            const int r = (e - 4) / 5, q = (e - 4) % 5;
            double s = b_at(tj, 0, r) * PA[q];
            for (int k = 1; k < 5; ++k) s += b_at(tj, k, r) * PA[5 * k + q];
            SG[e] = s;
          }
        }
        c.sync();
        // K = S^-1 G by the closed-form inverse (10 lanes)
        const double det = SG[0] * SG[3] - SG[1] * SG[2];
        bool sing = !(det > 0.0) || nonfinite_(det);
        for (int e = c.lane; e < NGAIN; e += c.width) {
          const int r = e / 5, q = e % 5;
          const double g0 = SG[4 + q], g1 = SG[9 + q];
          const double k = r == 0 ? (SG[3] * g0 - SG[1] * g1) / det : (SG[0] * g1 - SG[2] * g0) / det;
          KT[NGAIN * j + e] = k;
          sing = sing || nonfinite_(k);
          if (dabs_(k) > KM[e]) KM[e] = dabs_(k);   // this entry's largest magnitude so far
        }
        c.sync();
        // A - B K (25 lanes)
        for (int e = c.lane; e < 25; e += c.width) {
          const int r = e / 5, q = e % 5;
          ACL[e] = a_at(tj, r, q) - (b_at(tj, r, 0) * KT[NGAIN * j + q] + b_at(tj, r, 1) * KT[NGAIN * j + 5 + q]);
        }
        c.sync();
        // Q_i + (P A)' (A - B K) (25 lanes); P is symmetric bit for bit, so (P A)' = A' P
        for (int e = c.lane; e < 25; e += c.width) {
          const int r = e / 5, q = e % 5;
          double s = PA[r] * ACL[q];
          for (int k = 1; k < 5; ++k) s += PA[5 * k + r] * ACL[5 * k + q];
          const double v = rot_at(sh.q, tj[T_C], tj[T_S], r, q) + s;
          RAW[e] = v;
          sing = sing || nonfinite_(v);
        }
        c.sync();
        for (int e = c.lane; e < 25; e += c.width) P[e] = 0.5 * (RAW[e] + RAW[5 * (e % 5) + e / 5]);
        sing = c.any(sing);
        c.sync();
        dead = sing;
      }
      if (dead)
        for (int e = c.lane; e < NGAIN; e += c.width) KT[NGAIN * j + e] = NaN;
      if (ctg)
        for (int e = c.lane; e < NCTG; e += c.width) {
          int r, q;
          tri_at(e, r, q);
          ctg[(int64_t)i * NCTG + e] = dead ? NaN : P[5 * r + q];
        }
    }
    c.sync();
    for (int t = c.lane; t < nr * NGAIN; t += c.width) gains[(int64_t)i0 * NGAIN + t] = KT[t];
  }
  if (dead) {
    for (int t = c.lane; t < N * NTUBE; t += c.width) tube[t] = NaN;
    for (int q = c.lane; q < NMET; q += c.width) b.metrics[p * NMET + q] = NaN;
    if (c.lane == 0) { b.worst[p * 2] = -1; b.worst[p * 2 + 1] = -1; b.flags[p] = HTP_LQR_SINGULAR; }
    return;
  }
  const double trace0 = (((P[0] + P[6]) + P[12]) + P[18]) + P[24];

  // ---- forward pass: Sigma_0 in the frame of X_0; chunks of stages from the first one up
  c.gsync();    // the gains this wavefront stored are read back chunk by chunk
  {
    double sn, cs;
    hm::sincos(X[3], sn, cs);
    for (int e = c.lane; e < 25; e += c.width) P[e] = rot_at(sh.var0, cs, sn, e / 5, e % 5);
  }
  for (int node0 = 0; node0 < N; node0 += CHUNK) {
    const int i0 = node0, nr = NST - i0 < CHUNK ? (NST - i0 > 0 ? NST - i0 : 0) : CHUNK;   // stages of this chunk
    const int nn = N - node0 < CHUNK ? N - node0 : CHUNK;                                  // nodes of this chunk
    c.sync();
    for (int j = c.lane; j < nr; j += c.width) {
      const int i = i0 + j;
      linearise(X + 5 * i, U[2 * i], U[2 * i + 1], wb, H[i], topt, tile + TR * j);
    }
    {
      bool nobad = false;
      if (nr > 0) c.load_run(KT, gains + (int64_t)i0 * NGAIN, nr * NGAIN, nobad);
    }
    c.sync();
    for (int j = 0; j < nn; ++j) {
      const int i = node0 + j;
      const bool last = i == N - 1;
      const double* tj = tile + TR * j;
      const double* Kj = KT + NGAIN * j;
      const double cs = last ? CSN[0] : tj[T_C], sn = last ? CSN[1] : tj[T_S];
      if (!dead) {
        // A - B K (25 lanes) and K Sigma (10 lanes)
        if (!last)
          for (int e = c.lane; e < 35; e += c.width) {
            if (e < 25) {
              const int r = e / 5, q = e % 5;
              ACL[e] = a_at(tj, r, q) - (b_at(tj, r, 0) * Kj[q] + b_at(tj, r, 1) * Kj[5 + q]);
            } else {
              const int r = (e - 25) / 5, q = (e - 25) % 5;
              double s = Kj[5 * r] * P[q];
              for (int k = 1; k < 5; ++k) s += Kj[5 * r + k] * P[5 * k + q];
              KS[e - 25] = s;
            }
          }
        c.sync();
        // the tube row of node i (7 lanes), each lane keeping its quantity's running extreme; (A - B K) Sigma (25)
        bool sing = false;
        for (int e = c.lane; e < 32; e += c.width) {
          if (e < NTUBE) {
            double var;
            if (e == 0) var = cs * (cs * P[0] + sn * P[1]) + sn * (cs * P[5] + sn * P[6]);
            else if (e == 1) var = sn * (sn * P[0] - cs * P[1]) - cs * (sn * P[5] - cs * P[6]);
            else if (e < 5) var = P[6 * e];
            else if (last) var = 0.0;
            else {
              const int r = e - 5;
              var = KS[5 * r] * Kj[5 * r];
              for (int k = 1; k < 5; ++k) var += KS[5 * r + k] * Kj[5 * r + k];
            }
            const double sg = root_(var);
            sing = sing || nonfinite_(sg);
            tube[(int64_t)i * NTUBE + e] = sg;
            if (e == 0) { if (sg > RUN[2 * R_SLON]) { RUN[2 * R_SLON] = sg; RUN[2 * R_SLON + 1] = (double)i; } }
            else if (e == 1) {
              if (sg > RUN[2 * R_SLAT]) { RUN[2 * R_SLAT] = sg; RUN[2 * R_SLAT + 1] = (double)i; }
              if (last) CSN[2] = sg;
            } else if (e == 3) { if (sg > RUN[2 * R_STH]) { RUN[2 * R_STH] = sg; RUN[2 * R_STH + 1] = (double)i; } }
            int k = -1;
            double head = 0.0;
            if (e == 2) { k = R_SPEED; head = vmax - dabs_(X[5 * i + 2]); }
            else if (e == 4) { k = R_STEER; head = smax - dabs_(X[5 * i + 4]); }
            else if (e == 5 && !last) { k = R_ACC; head = amax - dabs_(U[2 * i]); }
            else if (e == 6 && !last) { k = R_RATE; head = wmax - dabs_(U[2 * i + 1]); }
            if (k >= 0) {
              const double rt = ratio_(head, sg);
              if (rt < RUN[2 * k] || RUN[2 * k + 1] < 0.0) { RUN[2 * k] = rt; RUN[2 * k + 1] = (double)i; }
            }
          } else if (!last) {
            const int f = e - NTUBE, r = f / 5, q = f % 5;
            double s = ACL[5 * r] * P[q];
            for (int k = 1; k < 5; ++k) s += ACL[5 * r + k] * P[5 * k + q];
            PA[f] = s;
          }
        }
        c.sync();
        if (!last) {
          // (A - B K) Sigma (A - B K)' + h W_i (25 lanes), then the symmetric part
          for (int e = c.lane; e < 25; e += c.width) {
            const int r = e / 5, q = e % 5;
            double s = PA[5 * r] * ACL[5 * q];
            for (int k = 1; k < 5; ++k) s += PA[5 * r + k] * ACL[5 * q + k];
            const double v = s + tj[T_H] * rot_at(sh.w, cs, sn, r, q);
            RAW[e] = v;
            sing = sing || nonfinite_(v);
          }
          c.sync();
          for (int e = c.lane; e < 25; e += c.width) P[e] = 0.5 * (RAW[e] + RAW[5 * (e % 5) + e / 5]);
        }
        sing = c.any(sing);
        c.sync();
        if (sing) {                    // the row just written is part of "from that node on"
          dead = true;
          for (int e = c.lane; e < NTUBE; e += c.width) tube[(int64_t)i * NTUBE + e] = NaN;
        }
      } else {
        for (int e = c.lane; e < NTUBE; e += c.width) tube[(int64_t)i * NTUBE + e] = NaN;
      }
    }
  }
  c.sync();
  if (dead) {
    for (int q = c.lane; q < NMET; q += c.width) b.metrics[p * NMET + q] = NaN;
    if (c.lane == 0) { b.worst[p * 2] = -1; b.worst[p * 2 + 1] = -1; b.flags[p] = HTP_LQR_SINGULAR; }
    return;
  }
  if (c.lane == 0) {
    double kmax = 0.0;
    for (int e = 0; e < NGAIN; ++e) kmax = KM[e] > kmax ? KM[e] : kmax;
    double* mt = b.metrics + p * NMET;
    mt[HTP_LQR_MAX_SLAT] = RUN[2 * R_SLAT]; mt[HTP_LQR_MAX_SLON] = RUN[2 * R_SLON]; mt[HTP_LQR_MAX_STH] = RUN[2 * R_STH];
    mt[HTP_LQR_END_SLAT] = CSN[2]; mt[HTP_LQR_MAX_GAIN] = kmax; mt[HTP_LQR_TRACE_P0] = trace0;
    mt[HTP_LQR_RATIO_ACC] = RUN[2 * R_ACC]; mt[HTP_LQR_RATIO_RATE] = RUN[2 * R_RATE];
    mt[HTP_LQR_RATIO_STEER] = RUN[2 * R_STEER]; mt[HTP_LQR_RATIO_SPEED] = RUN[2 * R_SPEED];
    b.worst[p * 2] = (int)RUN[2 * R_SLAT + 1];
    b.worst[p * 2 + 1] = (int)RUN[2 * R_RATE + 1];
    int fl = 0;
    if (RUN[2 * R_ACC] < sh.k_sigma) fl |= HTP_LQR_AUTHORITY_ACC;
    if (RUN[2 * R_RATE] < sh.k_sigma) fl |= HTP_LQR_AUTHORITY_RATE;
    if (RUN[2 * R_STEER] < sh.k_sigma) fl |= HTP_LQR_AUTHORITY_STEER;
    if (RUN[2 * R_SPEED] < sh.k_sigma) fl |= HTP_LQR_AUTHORITY_SPEED;
    b.flags[p] = fl;
  }
}

}  // namespace lqr
}  // namespace htp

#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC pop_options
#endif
