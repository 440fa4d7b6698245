// Closed-loop tracking rollout of one solved OBCA trajectory (include/htp.h holds the definition): R disturbance
// scenarios of one problem, each a serial rollout of a kinematic plant under a fixed tracking controller along the
// solved trajectory, with the clearance of the placed bodies measured at every control tick.  One problem per
// 64-lane wavefront on gfx950 (htp_track.hip), one lane per scenario, or a single serial lane (track_hostsim.cpp,
// tests only); one __host__ __device__ source, so both produce the same doubles:
//   - no contraction (pragma below) and the planner libm (htp_libm.h);
//   - a lane's rollout is serial and touches no other lane's state;
//   - everything across lanes is a minimum (with its index, ties to the lowest) or a count.
// The reference signal is the timeline's row (timeline_core.h run_problem), which is not callable on its own: it is
// restated in ref_row below, and tests/test_track_cpu.py holds the two together bit for bit.  The kinematic model,
// the integrator, the edge records and the signed distance are the audit's (audit_core.h, included unedited).
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
namespace track {

constexpr int MAXN = HTP_TRACK_MAX_N;
constexpr int NMET = HTP_TRACK_NMETRIC, NDIST = HTP_TRACK_NDIST, NFLAG = HTP_TRACK_NFLAG, NREF = HTP_TRACK_NREF;
constexpr int CHUNK = 64;            // ticks whose reference rows are staged in LDS at once
constexpr int TR = 7;                // tile row: xr, yr, vr, thr, dr, cos thr, sin thr
constexpr int ER = audit::ER, TEO_MAX = audit::TEO_MAX, TEB_MAX = audit::TEB_MAX;
// fixed LDS (doubles): obstacle edges | body edges | polygon (first row, edge count) | reference tile of CHUNK + 1
// rows (the raw halfspace rows live there until the edges are built) | per-tick minima of the chunk
constexpr int L_EO = 0, L_EB = L_EO + ER * TEO_MAX, L_PI = L_EB + ER * TEB_MAX, L_TILE = L_PI + 2 * (MAXM + MAXK);
constexpr int TILE_DOUBLES = 3 * (TEO_MAX + TEB_MAX);
constexpr int L_TK = L_TILE + TILE_DOUBLES, L_FIXED = L_TK + CHUNK;
static_assert(TR * (CHUNK + 1) <= TILE_DOUBLES, "the reference tile fits the raw-row area");
static_assert(L_FIXED % 2 == 0, "the per-stage LDS behind it stays 16-byte aligned");
static_assert(MAXN == audit::MAXN, "the audit's horizon limit");
// per-stage LDS (doubles): X 5N | U 2(N-1) | tau, then h N-1 | node times N
HTP_HD inline int lds_stage_doubles(int N) { return 9 * N; }
static_assert((L_FIXED + 9 * MAXN) * 8 <= 65536, "LDS of the largest horizon fits a workgroup");
constexpr double MAX_QUOTIENT = 1073741824.0;   // T / dt must stay below 2^30, as the timeline's
constexpr double INF = audit::INF;
constexpr int NOIDX = 0x7fffffff;
enum Dist { D_LAT = 0, D_LON, D_YAW, D_BIAS, D_SLIP, D_YAWGAIN };
static_assert(D_YAWGAIN + 1 == NDIST, "htp.h scenario columns");
static_assert((HTP_TRACK_BAD_TIME << 1) == (1 << NFLAG), "htp.h flag bits");

struct Shape {   // launch-uniform
  int N, M, K, topt, P, R, max_ticks;
  int eo[MAXM], eb[MAXK], offo[MAXM], offb[MAXK];
  int TEo, TEb;
  int64_t stride;   // doubles between two problems' x rows
  int oTAU;         // offset of tau inside a row (X at 0, U behind X)
  double dt, k_lat, k_yaw, k_lon, abort_dist, margin_tol;
};

struct Batch {   // device or host pointers
  const double *obsA, *obsb, *bodyG, *bodyg, *params, *x, *scen;
  double* metrics;
  int32_t* worst;
  int32_t* flags;
  int32_t* tally;
  int32_t* worst_scenario;
  double* tick;        // nullable
  double* reference;   // nullable
};

HTP_HD inline void make_shape(Shape& s, const htp_obca_batch& in, const htp_obca_track_opts& o) {
  s.N = in.N; s.M = in.M; s.K = in.K; s.topt = in.time_opt ? 1 : 0;
  s.P = o.plant_substeps; s.R = o.R; s.max_ticks = o.max_ticks;
  s.TEo = 0; s.TEb = 0;
  for (int m = 0; m < MAXM; ++m) { s.eo[m] = 0; s.offo[m] = 0; }
  for (int k = 0; k < MAXK; ++k) { s.eb[k] = 0; s.offb[k] = 0; }
  for (int m = 0; m < in.M; ++m) { s.eo[m] = in.obs_edges[m]; s.offo[m] = s.TEo; s.TEo += s.eo[m]; }
  for (int k = 0; k < in.K; ++k) { s.eb[k] = in.body_edges[k]; s.offb[k] = s.TEb; s.TEb += s.eb[k]; }
  Dims D;
  make_dims(D, in.N, in.M, in.K, in.time_opt, in.obs_edges, in.body_edges);
  s.stride = D.n; s.oTAU = D.oTAU;
  s.dt = o.dt; s.k_lat = o.k_lat; s.k_yaw = o.k_yaw; s.k_lon = o.k_lon;
  s.abort_dist = o.abort_dist; s.margin_tol = o.margin_tol;
}

// The serial lane of the test-only host build; the gfx950 wavefront is in htp_track.hip.
struct HostLane : audit::HostLane {
  int count(bool v) const { return v ? 1 : 0; }
};

HTP_HD inline double clamp_(double u, double m, bool& bit) {
  if (u < -m) { bit = true; return -m; }
  if (u > m) { bit = true; return m; }
  return u;
}

// ref(k): the timeline's row at s = fl(k dt) for k < n (the same interval rule, the same audit::step), the stored
// last node for k >= n; seven doubles: the five of the state, then cos and sin of its heading
HTP_HD inline void ref_row(int k, int n, int N, int topt, double dt, double wb, const double* X, const double* U,
                           const double* Tn, double* row) {
  audit::State f;
  if (k < n) {
    const double s = (double)k * dt;
    int lo = 0, hi = N - 2;          // the largest i in 0..N-2 with t_i <= s (t_0 = 0 <= s)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (Tn[mid] <= s) lo = mid; else hi = mid - 1;
    }
    const int i = lo;
    const double tau = s - Tn[i];
    const audit::State x0{X[5 * i], X[5 * i + 1], X[5 * i + 2], X[5 * i + 3], X[5 * i + 4]};
    f = audit::step(x0, U[2 * i], U[2 * i + 1], wb, tau, topt);
  } else {
    const double* xn = X + 5 * (N - 1);
    f = audit::State{xn[0], xn[1], xn[2], xn[3], xn[4]};
  }
  double sn, cs;
  hm::sincos(f.th, sn, cs);
  row[0] = f.x; row[1] = f.y; row[2] = f.v; row[3] = f.th; row[4] = f.st; row[5] = cs; row[6] = sn;
}

// the plant's derivative: audit::kin at the slipped speed and the biased steering angle, heading rate scaled
HTP_HD inline audit::State plant_f(const audit::State& q, double a, double w, double wb, double keep, double bias,
                                   double ygain) {
  audit::State f = audit::kin(audit::State{q.x, q.y, keep * q.v, q.th, q.st + bias}, a, w, wb);
  f.th = f.th * ygain;
  return f;
}

// every scenario of a rejected problem: NaN, -1 and the one flag
template <class W>
HTP_HD inline void reject(const W& c, const Shape& sh, const Batch& b, int64_t p, int flag) {
  const double NaN = __builtin_nan("");
  for (int sc = c.lane; sc < sh.R; sc += c.width) {
    const int64_t o = p * sh.R + sc;
    for (int q = 0; q < NMET; ++q) b.metrics[o * NMET + q] = NaN;
    for (int q = 0; q < 3; ++q) b.worst[o * 3 + q] = -1;
    b.flags[o] = flag;
  }
  for (int q = c.lane; q < NFLAG; q += c.width) b.tally[p * NFLAG + q] = ((1 << q) == flag) ? sh.R : 0;
  if (c.lane == 0) b.worst_scenario[p] = -1;
}

// One problem.  sl: L_FIXED doubles of LDS, dl: lds_stage_doubles(N) doubles of LDS (both 16-byte aligned).
template <class W>
HTP_HD inline void run_problem(const W& c, const Shape& sh, const Batch& b, int64_t p, double* sl, double* dl) {
  using audit::State;
  using audit::dabs_;
  using audit::dmax_;
  using audit::nonfinite_;
  const int N = sh.N, M = sh.M, K = sh.K, topt = sh.topt, R = sh.R;
  double* X = dl;
  double* U = X + 5 * N;
  double* H = U + 2 * (N - 1);
  double* Tn = H + (N - 1);
  double* Eo = sl + L_EO;
  double* Eb = sl + L_EB;
  double* pinfo = sl + L_PI;
  double* tile = sl + L_TILE;
  double* tk = sl + L_TK;
  double* rawO = tile;
  double* rawB = tile + 3 * TEO_MAX;
  const double* par = b.params + p * NPARAM;
  const double NaN = __builtin_nan("");

  // ---- the doubles read: X, U (one run), tau; halfspace rows; the parameters
  bool bad = false;
  const double* xr = b.x + p * sh.stride;
  c.load_run(X, xr, 5 * N + 2 * (N - 1), bad);
  if (topt) c.load_run(H, xr + sh.oTAU, N - 1, bad);
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
  bad = bad || nonfinite_(dT) || nonfinite_(wb) || nonfinite_(dmin) || nonfinite_(vmax) || nonfinite_(smax) ||
        nonfinite_(amax) || nonfinite_(wmax);
  bad = c.any(bad);
  c.sync();
  if (bad) { reject(c, sh, b, p, HTP_TRACK_NONFINITE); return; }

  // ---- step lengths and node times, as the timeline's: serial sums by one lane
  bool nonpos = false;
  for (int i = c.lane; i < N - 1; i += c.width) {
    const double h = topt ? dT * H[i] : dT;
    H[i] = h;
    nonpos = nonpos || !(h > 0.0);
  }
  nonpos = c.any(nonpos);
  c.sync();
  if (nonpos) { reject(c, sh, b, p, HTP_TRACK_BAD_TIME); return; }
  if (c.lane == 0) {
    double t = 0.0;
    Tn[0] = 0.0;
    for (int i = 0; i < N - 1; ++i) { t += H[i]; Tn[i + 1] = t; }
  }

  // ---- polygons, as the audit's: one row per lane, then one polygon per lane compacts its edges in place
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
    audit::build_row(body ? rawB : rawO, first, cnt, rr, (body ? Eb : Eo) + ER * rr);
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
      if (st == audit::ROW_EDGE) {
        for (int q = 0; q < ER; ++q) E[ER * n + q] = E[ER * e + q];
        ++n;
      } else if (st != audit::ROW_REDUNDANT) {
        pb = true;
      }
    }
    pinfo[2 * j] = (double)first;
    pinfo[2 * j + 1] = (pb || n < 3) ? -1.0 : (double)n;
  }
  c.sync();
  bool polybad = false;
  for (int j = 0; j < M + K; ++j) polybad = polybad || pinfo[2 * j + 1] < 0.0;

  const double dt = sh.dt;
  const double T = Tn[N - 1];
  const double quot = T / dt;
  if (!(quot < MAX_QUOTIENT)) { reject(c, sh, b, p, HTP_TRACK_BAD_TIME); return; }
  int n = (int)quot;                   // the smallest n with fl(n dt) >= T (the quotient is only a first guess)
  while (n > 0 && (double)(n - 1) * dt >= T) --n;
  while ((double)n * dt < T) ++n;
  const int np = n + 1 < sh.max_ticks ? n + 1 : sh.max_ticks;
  const int pflags = (n + 1 > sh.max_ticks ? HTP_TRACK_TRUNCATED : 0) | (polybad ? HTP_TRACK_BAD_POLYTOPE : 0);
  const double hp = dt / (double)sh.P, hh = 0.5 * hp;

  double wbest = INF;                  // worst scenario so far (wave-uniform)
  int wsc = NOIDX;
  for (int s0 = 0; s0 < R; s0 += c.width) {   // one pass per c.width scenarios
    // ---- this lane's scenario
    const int sc = s0 + c.lane;
    const bool mine = sc < R;
    double keep = 1.0, bias = 0.0, ygain = 1.0;
    State q{0.0, 0.0, 0.0, 0.0, 0.0};
    bool live = false;
    if (mine) {
      const double* d = b.scen + (int64_t)sc * NDIST;
      const double lat0 = d[D_LAT], lon0 = d[D_LON], yaw0 = d[D_YAW], slip = d[D_SLIP];
      bias = d[D_BIAS]; ygain = d[D_YAWGAIN];
      live = !(nonfinite_(lat0) || nonfinite_(lon0) || nonfinite_(yaw0) || nonfinite_(slip) || nonfinite_(bias) ||
               nonfinite_(ygain));
      keep = 1.0 - slip;
      double s0_, c0_;
      hm::sincos(X[3], s0_, c0_);
      q = State{(X[0] + lon0 * c0_) - lat0 * s0_, (X[1] + lon0 * s0_) + lat0 * c0_, X[2], X[3] + yaw0, X[4]};
    }
    bool run = live;
    double clr = INF, mlat = 0.0, mlon = 0.0, mth = 0.0, mdev = 0.0, epos = 0.0, eth = 0.0;
    int bk = -1, bmk = -1, nctl = 0, nsat = 0, fl = 0;

    for (int r0 = 0; r0 < np; r0 += CHUNK) {
      const int nr = np - r0 < CHUNK ? np - r0 : CHUNK;
      const int nrows = r0 + nr < np ? nr + 1 : nr;   // the row behind the chunk is the last tick's r+
      c.sync();   // the previous chunk's tile (or the raw rows) and minima are no longer read
      for (int j = c.lane; j < nrows; j += c.width) ref_row(r0 + j, n, N, topt, dt, wb, X, U, Tn, tile + TR * j);
      c.sync();
      if (b.reference && s0 == 0)
        for (int t = c.lane; t < nr * NREF; t += c.width)
          b.reference[(p * sh.max_ticks + r0) * NREF + t] = tile[TR * (t / NREF) + t % NREF];

      for (int j = 0; j < nr; ++j) {
        const int k = r0 + j;
        const double* rr = tile + TR * j;
        double ck = INF;
        double e_lon = 0.0, e_lat = 0.0, e_th = 0.0;
        if (run) {
          const double xr_ = rr[0], yr_ = rr[1], thr = rr[3], dr = rr[4], cr = rr[5], sr = rr[6];
          const double dx = q.x - xr_, dy = q.y - yr_, dth = q.th - thr;
          e_lon = cr * dx + sr * dy;
          e_lat = cr * dy - sr * dx;
          double sd, cd;
          hm::sincos(dth, sd, cd);
          e_th = hm::atan2(sd, cd);
          if (!polybad) {
            double sn, cs;
            hm::sincos(q.th, sn, cs);
            for (int m = 0; m < M; ++m)
              for (int kk = 0; kk < K; ++kk) {
                const double d = audit::signed_distance(Eo + ER * (int)pinfo[2 * m], (int)pinfo[2 * m + 1],
                                                        Eb + ER * (int)pinfo[2 * (M + kk)], (int)pinfo[2 * (M + kk) + 1],
                                                        q.x, q.y, cs, sn);
                if (d < ck) ck = d;
                if (d < clr) { clr = d; bk = k; bmk = m * K + kk; }   // ascending (k M + m) K + kk: ties keep the lowest
              }
          }
          mlat = dmax_(mlat, dabs_(e_lat));
          mlon = dmax_(mlon, dabs_(e_lon));
          mth = dmax_(mth, dabs_(e_th));
          mdev = dmax_(mdev, dabs_(q.st - dr));
          epos = hm::hypot(e_lon, e_lat);
          eth = dabs_(e_th);
        }
        if (b.tick) {                  // a wave-level step: every lane takes it, the idle ones with +inf
          const double w = c.minv(ck);
          if (c.lane == 0) tk[j] = polybad ? NaN : w;
        }
        if (run && !(epos <= sh.abort_dist)) { fl |= HTP_TRACK_DIVERGED; run = false; }
        if (run && k + 1 < np) {
          const double* rn = tile + TR * (j + 1);
          const double vrn = rn[2], drn = rn[4];
          const double g = vrn < 0.0 ? -1.0 : 1.0;
          bool nobit = false, ba = false, bs = false, bw = false;
          const double v_des = clamp_(vrn - sh.k_lon * e_lon, vmax, nobit);
          const double a = clamp_((v_des - q.v) / dt, amax, ba);
          const double d_des = clamp_((drn - sh.k_lat * e_lat) - (g * sh.k_yaw) * e_th, smax, bs);
          const double w = clamp_((d_des - q.st) / dt, wmax, bw);
          fl |= (ba ? HTP_TRACK_SAT_ACC : 0) | (bs ? HTP_TRACK_SAT_STEER : 0) | (bw ? HTP_TRACK_SAT_RATE : 0);
          ++nctl;
          if (ba || bs || bw) ++nsat;
          for (int u = 0; u < sh.P; ++u) {
            const State f1 = plant_f(q, a, w, wb, keep, bias, ygain);
            const State qm{q.x + hh * f1.x, q.y + hh * f1.y, q.v + hh * f1.v, q.th + hh * f1.th, q.st + hh * f1.st};
            const State f2 = plant_f(qm, a, w, wb, keep, bias, ygain);
            q = State{q.x + hp * f2.x, q.y + hp * f2.y, q.v + hp * f2.v, q.th + hp * f2.th, q.st + hp * f2.st};
          }
          q.st = clamp_(q.st, smax, nobit);
        }
      }
      if (b.tick) {
        c.sync();
        for (int j = c.lane; j < nr; j += c.width) {
          double* o = b.tick + p * sh.max_ticks + r0 + j;
          double v = tk[j];
          // a later pass of scenarios merges into what this same lane wrote in an earlier one (program order)
          if (s0 > 0 && !polybad) { const double e = *o; v = e < v ? e : v; }
          *o = v;
        }
      }
    }

    // ---- this pass's scenarios out; the tally and the worst scenario merge into the earlier passes'
    if (mine) {
      const int64_t o = p * R + sc;
      double* mt = b.metrics + o * NMET;
      int32_t* wo = b.worst + o * 3;
      if (!live) {
        for (int t = 0; t < NMET; ++t) mt[t] = NaN;
        wo[0] = wo[1] = wo[2] = -1;
        fl = HTP_TRACK_NONFINITE;
      } else {
        fl |= pflags;
        if (polybad) {
          mt[HTP_TRACK_CLEARANCE] = NaN;
          wo[0] = wo[1] = wo[2] = -1;
        } else {
          mt[HTP_TRACK_CLEARANCE] = clr;
          wo[0] = bk; wo[1] = bk < 0 ? -1 : bmk / K; wo[2] = bk < 0 ? -1 : bmk % K;
          if (clr < 0.0) fl |= HTP_TRACK_COLLISION;
          if (clr < dmin - sh.margin_tol) fl |= HTP_TRACK_MARGIN;
        }
        mt[HTP_TRACK_MAX_ELAT] = mlat; mt[HTP_TRACK_MAX_ELON] = mlon; mt[HTP_TRACK_MAX_ETH] = mth;
        mt[HTP_TRACK_END_POS] = epos; mt[HTP_TRACK_END_ETH] = eth; mt[HTP_TRACK_MAX_STEER_DEV] = mdev;
        mt[HTP_TRACK_SAT_SHARE] = nctl > 0 ? (double)nsat / (double)nctl : 0.0;
      }
      b.flags[o] = fl;
    }
    for (int t = 0; t < NFLAG; ++t) {
      const int cnt = c.count(mine && ((fl >> t) & 1));
      if (c.lane == 0) b.tally[p * NFLAG + t] = (s0 > 0 ? b.tally[p * NFLAG + t] : 0) + cnt;
    }
    const bool has = mine && live && !polybad && !nonfinite_(clr);
    double cv = has ? clr : INF;
    int ci = has ? sc : NOIDX;
    c.min_key(cv, ci);
    if (ci != NOIDX && (cv < wbest || wsc == NOIDX)) { wbest = cv; wsc = ci; }
  }
  if (c.lane == 0) b.worst_scenario[p] = wsc == NOIDX ? -1 : wsc;
}

}  // namespace track
}  // namespace htp

#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC pop_options
#endif
