// Closed-loop rollout of one solved OBCA trajectory under its time-varying LQR gains (include/htp.h holds the
// definition): the tracking rollout of track_core.h with the fixed three-gain controller replaced by
// u = u_ff - K_i e.  One problem per 64-lane wavefront on gfx950 (htp_ltrack.hip), one lane per scenario, or a single
// serial lane (ltrack_hostsim.cpp, tests only); one __host__ __device__ source, so both produce the same doubles:
//   - no contraction (pragma below) and the planner libm (htp_libm.h);
//   - a lane's rollout is serial and touches no other lane's state;
//   - everything across lanes is a minimum (with its index, ties to the lowest), a maximum or a count.
// The reference row, the plant, the clamp, the rejection and the launch shape are the track's (track_core.h, included
// unedited, and through it audit_core.h); what is new is the law row: the lane that builds tick k's reference row also
// loads K_i of the stage that holds fl(k dt) from global memory and rotates its position columns into that node's
// frame, once, so that the serial tick loop reads ten ready gains by a broadcast LDS address.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/htp.h"
#include "track_core.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif

namespace htp {
namespace ltrack {

using track::CHUNK;
using track::ER;
using track::INF;
using track::MAXN;
using track::NDIST;
using track::NFLAG;
using track::NMET;
using track::NOIDX;
using track::NREF;
using track::TEB_MAX;
using track::TEO_MAX;
using track::Shape;   // launch-uniform, as the track's (its three gains are unused and zero)
using track::D_LAT; using track::D_LON; using track::D_YAW; using track::D_BIAS; using track::D_SLIP; using track::D_YAWGAIN;

constexpr int NGAIN = HTP_LQR_NGAIN, NERR = 3;
// tile row: the track's seven (xr, yr, vr, thr, dr, cos thr, sin thr), then the law row (k_lon, k_lat, K2, K3, K4)
// of a, then of w.  17 is an odd stride, as lqr_core.h's tile: sixteen lanes' 8-byte stores of one entry of their
// rows fall on distinct banks (an even stride would fold them onto half or fewer).  The tick loop reads a row by one
// address for the whole wavefront, which is a broadcast whatever the stride.
constexpr int TR = 17, T_LAW = 7;
// fixed LDS (doubles): obstacle edges | body edges | polygon (first row, edge count) | tile of CHUNK + 1 rows (the raw
// halfspace rows live there until the edges are built) | per-tick minima of the chunk | per-tick error maxima
constexpr int L_EO = 0, L_EB = L_EO + ER * TEO_MAX, L_PI = L_EB + ER * TEB_MAX, L_TILE = L_PI + 2 * (MAXM + MAXK);
constexpr int RAW_DOUBLES = 3 * (TEO_MAX + TEB_MAX);
constexpr int TILE_DOUBLES = (TR * (CHUNK + 1) + 1) & ~1;
static_assert(RAW_DOUBLES <= TILE_DOUBLES, "the raw halfspace rows fit the tile area");
constexpr int L_TK = L_TILE + TILE_DOUBLES, L_TE = L_TK + CHUNK, L_FIXED = L_TE + NERR * CHUNK;
static_assert(L_FIXED % 2 == 0, "the per-stage LDS behind it stays 16-byte aligned");
// per-stage LDS: the track's (X 5N | U 2(N-1) | h N-1 | node times N).  The gains (80 bytes per stage, 38 KB at
// N = 480) stay in global memory.
HTP_HD inline int lds_stage_doubles(int N) { return 9 * N; }
static_assert((L_FIXED + 9 * MAXN) * 8 <= 65536, "LDS of the largest horizon fits a workgroup");

struct Batch {   // device or host pointers
  track::Batch t;
  const double* gains;
  double* tick_error;   // nullable
};

HTP_HD inline void make_shape(Shape& s, const htp_obca_batch& in, const htp_obca_ltrack_opts& o) {
  const htp_obca_track_opts t{o.dt, o.max_ticks, o.plant_substeps, 0.0, 0.0, 0.0, o.abort_dist, o.margin_tol, o.R,
                              o.scenarios};
  track::make_shape(s, in, t);
}

// The serial lane of the test-only host build; the gfx950 wavefront is in htp_ltrack.hip.
using HostLane = track::HostLane;

// the law row of tick k: K_i of the stage i that holds fl(k dt), its position columns rotated into node i's frame
HTP_HD inline void law_row(int k, int N, double dt, const double* X, const double* Tn, const double* G, double* law) {
  const double s = (double)k * dt;
  int lo = 0, hi = N - 2;          // the largest i in 0..N-2 with t_i <= s (ref_row's rule)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (Tn[mid] <= s) lo = mid; else hi = mid - 1;
  }
  const double* K = G + NGAIN * lo;
  double si, ci;
  hm::sincos(X[5 * lo + 3], si, ci);
  for (int r = 0; r < 2; ++r) {
    const double kx = K[5 * r], ky = K[5 * r + 1];
    law[5 * r] = ci * kx + si * ky;
    law[5 * r + 1] = ci * ky - si * kx;
    law[5 * r + 2] = K[5 * r + 2];
    law[5 * r + 3] = K[5 * r + 3];
    law[5 * r + 4] = K[5 * r + 4];
  }
}

// what one scenario adds to a pose's error maximum: the magnitude, a NaN as 0
HTP_HD inline double err_term(double e) {
  const double a = audit::dabs_(e);
  return a > 0.0 ? a : 0.0;
}

// One problem.  sl: L_FIXED doubles of LDS, dl: lds_stage_doubles(N) doubles of LDS (both 16-byte aligned).
template <class W>
HTP_HD inline void run_problem(const W& c, const Shape& sh, const Batch& bb, int64_t p, double* sl, double* dl) {
  using audit::State;
  using audit::dabs_;
  using audit::dmax_;
  using audit::nonfinite_;
  using track::clamp_;
  using track::plant_f;
  const track::Batch& b = bb.t;
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
  double* te = sl + L_TE;
  double* rawO = tile;
  double* rawB = tile + 3 * TEO_MAX;
  const double* par = b.params + p * NPARAM;
  const double* G = bb.gains + p * (int64_t)(NGAIN * (N - 1));
  const double NaN = __builtin_nan("");

  // ---- the doubles read: X, U (one run), tau; halfspace rows; the parameters; every gain (one coalesced pass)
  bool bad = false;
  const double* xr = b.x + p * sh.stride;
  c.load_run(X, xr, 5 * N + 2 * (N - 1), bad);
  if (topt) c.load_run(H, xr + sh.oTAU, N - 1, bad);
  for (int r = c.lane; r < sh.TEo; r += c.width) {
    const double ax = b.obsA[(p * sh.TEo + r) * 2], ay = b.obsA[(p * sh.TEo + r) * 2 + 1], b0 = b.obsb[p * sh.TEo + r];
    rawO[3 * r] = ax; rawO[3 * r + 1] = ay; rawO[3 * r + 2] = b0;
    bad = bad || nonfinite_(ax) || nonfinite_(ay) || nonfinite_(b0);
  }
  for (int r = c.lane; r < sh.TEb; r += c.width) {
    const double ax = b.bodyG[(p * sh.TEb + r) * 2], ay = b.bodyG[(p * sh.TEb + r) * 2 + 1], b0 = b.bodyg[p * sh.TEb + r];
    rawB[3 * r] = ax; rawB[3 * r + 1] = ay; rawB[3 * r + 2] = b0;
    bad = bad || nonfinite_(ax) || nonfinite_(ay) || nonfinite_(b0);
  }
  for (int q = c.lane; q < NGAIN * (N - 1); q += c.width) bad = bad || nonfinite_(G[q]);
  const double dT = par[P_DT], wb = par[P_WHEELBASE], dmin = par[P_DMIN];
  const double vmax = dabs_(par[P_MAXV]), smax = dabs_(par[P_MAXSTEER]);
  const double amax = dabs_(par[P_MAXACC]), wmax = dabs_(par[P_MAXSR]);
  bad = bad || nonfinite_(dT) || nonfinite_(wb) || nonfinite_(dmin) || nonfinite_(vmax) || nonfinite_(smax) ||
        nonfinite_(amax) || nonfinite_(wmax);
  bad = c.any(bad);
  c.sync();
  if (bad) { track::reject(c, sh, b, p, HTP_TRACK_NONFINITE); return; }

  // ---- step lengths and node times, as the track's: serial sums by one lane
  bool nonpos = false;
  for (int i = c.lane; i < N - 1; i += c.width) {
    const double h = topt ? dT * H[i] : dT;
    H[i] = h;
    nonpos = nonpos || !(h > 0.0);
  }
  nonpos = c.any(nonpos);
  c.sync();
  if (nonpos) { track::reject(c, sh, b, p, HTP_TRACK_BAD_TIME); return; }
  if (c.lane == 0) {
    double t = 0.0;
    Tn[0] = 0.0;
    for (int i = 0; i < N - 1; ++i) { t += H[i]; Tn[i + 1] = t; }
  }

  // ---- polygons, as the track's: one row per lane, then one polygon per lane compacts its edges in place
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
  if (!(quot < track::MAX_QUOTIENT)) { track::reject(c, sh, b, p, HTP_TRACK_BAD_TIME); return; }
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
      c.sync();   // the previous chunk's tile (or the raw rows), minima and maxima are no longer read
      for (int j = c.lane; j < nrows; j += c.width) {
        track::ref_row(r0 + j, n, N, topt, dt, wb, X, U, Tn, tile + TR * j);
        if (j < nr) law_row(r0 + j, N, dt, X, Tn, G, tile + TR * j + T_LAW);   // the row behind carries no law
      }
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
        if (bb.tick_error) {           // likewise, the idle lanes with 0 (e_* are 0 unless this lane is at pose k)
          const double m0 = c.maxv(err_term(e_lat)), m1 = c.maxv(err_term(e_lon)), m2 = c.maxv(err_term(e_th));
          if (c.lane == 0) { te[NERR * j] = m0; te[NERR * j + 1] = m1; te[NERR * j + 2] = m2; }
        }
        if (run && !(epos <= sh.abort_dist)) { fl |= HTP_TRACK_DIVERGED; run = false; }
        if (run && k + 1 < np) {
          const double* rn = tile + TR * (j + 1);
          const double* lw = rr + T_LAW;
          const double vr = rr[2], dr = rr[4];
          const double e_v = q.v - vr, e_d = q.st - dr;
          const double fb0 = (((lw[0] * e_lon + lw[1] * e_lat) + lw[2] * e_v) + lw[3] * e_th) + lw[4] * e_d;
          const double fb1 = (((lw[5] * e_lon + lw[6] * e_lat) + lw[7] * e_v) + lw[8] * e_th) + lw[9] * e_d;
          const double a_cmd = (rn[2] - vr) / dt - fb0;
          const double w_cmd = (rn[4] - dr) / dt - fb1;
          bool nobit = false, ba = false, bs = false, bw = false;
          const double v_des = clamp_(q.v + dt * a_cmd, vmax, nobit);
          const double a = clamp_((v_des - q.v) / dt, amax, ba);
          const double d_des = clamp_(q.st + dt * w_cmd, smax, bs);
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
      if (b.tick || bb.tick_error) c.sync();
      if (b.tick) {
        for (int j = c.lane; j < nr; j += c.width) {
          double* o = b.tick + p * sh.max_ticks + r0 + j;
          double v = tk[j];
          // a later pass of scenarios merges into what this same lane wrote in an earlier one (program order)
          if (s0 > 0 && !polybad) { const double e = *o; v = e < v ? e : v; }
          *o = v;
        }
      }
      if (bb.tick_error) {
        for (int t = c.lane; t < nr * NERR; t += c.width) {   // the same t belongs to the same lane in every pass
          double* o = bb.tick_error + (p * sh.max_ticks + r0) * NERR + t;
          double v = te[t];
          if (s0 > 0) { const double e = *o; v = e > v ? e : v; }
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

}  // namespace ltrack
}  // namespace htp

#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC pop_options
#endif
