// Maximal speed profile and timed trajectory of one planner path (include/htp.h, "Maximal speed profile"): node caps
// from the speed, lateral-acceleration and steering-rate limits, stops at gear changes, the largest profile under the
// caps and the two acceleration bounds, interval times with dwells and hops, per-node outputs, a summary and the path
// at a fixed period in the timeline's ten columns.  One path per 64-lane wavefront on gfx950 (htp_speed.hip) or a
// single serial lane (speed_hostsim.cpp, tests only); one __host__ __device__ source over the wave context
// (wave_ctx.h: lane, width, bcast, maxv, isum, uniform, sync), so both produce the same doubles:
//   - no contraction (pragma below), the planner libm (htp_libm.h) for atan and hypot, IEEE sqrt and division;
//   - the two passes of the profile are min-plus scans (scan_min_before): a minimum of doubles is exact and
//     associative, so the wavefront's log-step scan in 64-node chunks with a carried minimum and the serial lane's
//     running minimum are the same numbers;
//   - S, t and the summary's sums are added left to right in node order (scan_add_serial: every lane performs the
//     chunk's additions in the same order from broadcast operands; nothing is reassociated).
// Scratch: WS_PER_NODE * cap_path doubles per path in flight (S, ds, delta, c, kind, w, t), structure of arrays.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/htp.h"
#include "htp_libm.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif

namespace htp {
namespace spd {

constexpr int NLIM = HTP_SPD_NLIM, NNODE = HTP_SPD_NNODE, NKIND = HTP_SPD_NKIND, NSUM = HTP_SPD_NSUM;
constexpr int NCOL = HTP_TIMELINE_NCOL;
constexpr int CHUNK = 64;               // fixed-period rows staged at once: one per lane
constexpr int TILE = CHUNK * NCOL;      // doubles of the row tile (LDS on the device)
constexpr int WS_PER_NODE = 7;          // scratch slots, each cap_path doubles
enum Slot { W_S = 0, W_DS, W_DL, W_C, W_KIND, W_W, W_T };
enum Col { C_T = 0, C_X, C_Y, C_V, C_TH, C_ST, C_ACC, C_SR, C_CURV, C_ARC };
static_assert(C_ARC + 1 == NCOL, "htp.h timeline columns");
static_assert(HTP_SPD_S_TIME_KIND + NKIND == NSUM && HTP_SPD_A_DEC + 1 == NKIND, "htp.h summary layout");
// device scratch the library takes for itself when the caller leaves the workgroup count to it (max_groups = 0)
constexpr size_t SCRATCH_BUDGET = (size_t)256 << 20;
constexpr double MAX_QUOTIENT = 1073741824.0;   // T / dt must stay below 2^30: row numbers are int32
constexpr double TWO_PI = 6.283185307179586, PI = 3.141592653589793;

HTP_HD inline double inf_() { return __builtin_inf(); }
HTP_HD inline double min_(double a, double b) { return b < a ? b : a; }
HTP_HD inline double max_(double a, double b) { return b > a ? b : a; }

// The minimum of v over the lanes before this one, joined with `carry` (the minimum of everything before the chunk);
// afterwards carry also holds this chunk.  Exact, so any evaluation order gives the same double.  All lanes call it.
template <class C>
HTP_HD inline double scan_min_before(const C& c, double v, double& carry) {
  for (int o = 1; o < C::width; o <<= 1) {
    const double u = c.bcast(v, c.lane >= o ? c.lane - o : c.lane);
    if (c.lane >= o) v = min_(v, u);
  }
  const double prev = c.bcast(v, c.lane > 0 ? c.lane - 1 : 0);
  const double before = c.lane > 0 ? min_(carry, prev) : carry;
  carry = c.uniform(min_(carry, c.bcast(v, C::width - 1)));
  return before;
}

// carry + v_0 + .. + v_lane added left to right (lanes 0 .. cnt-1 take part); afterwards carry holds the whole chunk.
// Every lane performs the same cnt additions, so there is one order of summation whatever the width.
template <class C>
HTP_HD inline double scan_add_serial(const C& c, double v, double& carry, int cnt) {
  double mine = carry;
  for (int k = 0; k < cnt; ++k) {
    carry = carry + c.bcast(v, k);
    if (c.lane == k) mine = carry;
  }
  return mine;
}

// The limits row of a path, read where it is used: ten wavefront-uniform doubles held live across the whole path would
// fill a fifth of the scalar registers.
struct Limits {
  const double* p;
  HTP_HD double L() const { return p[HTP_SPD_L_WHEELBASE]; }
  HTP_HD double vf() const { return p[HTP_SPD_L_VFWD]; }
  HTP_HD double vr() const { return p[HTP_SPD_L_VREV]; }
  HTP_HD double acc() const { return p[HTP_SPD_L_ACC]; }
  HTP_HD double dec() const { return p[HTP_SPD_L_DEC]; }
  HTP_HD double alat() const { return p[HTP_SPD_L_ALAT]; }
  HTP_HD double omega() const { return p[HTP_SPD_L_STEER_RATE]; }
  HTP_HD double max_steer() const { return p[HTP_SPD_L_MAXSTEER]; }
  HTP_HD double v0() const { return p[HTP_SPD_L_V0]; }
  HTP_HD double v1() const { return p[HTP_SPD_L_V1]; }
};

// Interval i from its end speeds squared, its length and its steer change.
struct Interval {
  double dt, a, vi, t1, vm;   // a: constant acceleration (a hop: acc, then -dec from t1 on, peak vm)
  int kind;                   // 0 ramp, 1 dwell, 2 hop
};

HTP_HD inline Interval interval_(double wi, double wj, double ds, double dd, const Limits& m) {
  Interval r;
  r.vi = sqrt(wi);
  const double vj = sqrt(wj);
  r.a = 0.0; r.t1 = 0.0; r.vm = 0.0;
  if (ds == 0.0) {
    r.kind = 1;
    r.dt = (m.omega() > 0.0 && dd != 0.0) ? fabs(dd) / m.omega() : 0.0;
  } else if (r.vi + vj > 0.0) {
    r.kind = 0;
    r.dt = 2.0 * ds / (r.vi + vj);
    r.a = (wj - wi) / (2.0 * ds);
  } else {
    r.kind = 2;
    r.vm = sqrt(2.0 * m.acc() * m.dec() * ds / (m.acc() + m.dec()));
    r.t1 = r.vm / m.acc();
    r.dt = r.t1 + r.vm / m.dec();
    r.a = m.acc();
  }
  return r;
}

// Out of line: inlined three times, the double-double constants of the libm crowd the scalar registers
HTP_HD __attribute__((noinline)) inline double atan_(double x) { return hm::atan(x); }
HTP_HD __attribute__((noinline)) inline double hypot_(double x, double y) { return hm::hypot(x, y); }
HTP_HD inline double wrap_(double d) { return d - TWO_PI * floor((d + PI) / TWO_PI); }

// One path.  ws: WS_PER_NODE * cap_path doubles of scratch, tile: TILE doubles (LDS on the device).
template <class C>
HTP_HD inline void run_path(const C& c, const htp_speed_in& in, const htp_speed_result& out, int64_t b, double* ws,
                            double* tile) {
  const int cap = in.cap_path;
  const int n = in.n_path[b];
  const double* P = in.path + b * (int64_t)cap * 5;
  const double* lim = in.limits + b * NLIM;
  const Limits m{lim};

  // ---- status, judged before anything is written
  int st = HTP_SPD_OK;
  if (in.path_status && in.path_status[b] != 0) {
    st = HTP_SPD_SKIPPED;
  } else if (n < 2 || n > cap) {
    st = HTP_SPD_BAD_INPUT;
  } else {
    bool bad = false;
    for (int j = 0; j < NLIM; ++j) bad = bad || hm::nonfinite(lim[j]);
    bad = bad || !(m.L() > 0.0) || !(m.vf() > 0.0) || !(m.vr() > 0.0) || !(m.acc() > 0.0) || !(m.dec() > 0.0) || m.alat() < 0.0 ||
          m.omega() < 0.0 || m.v0() < 0.0 || m.v1() < 0.0;
    for (int i = c.lane; i < n; i += C::width) {
      const double* r = P + 5 * (int64_t)i;
      for (int j = 0; j < 5; ++j) bad = bad || hm::nonfinite(r[j]);
      bad = bad || !(r[4] == 1.0 || r[4] == -1.0);
    }
    if (c.isum(bad ? 1 : 0) > 0) st = HTP_SPD_BAD_INPUT;
  }
  if (st != HTP_SPD_OK) {
    if (c.lane == 0) {
      out.status[b] = st;
      out.flags[b] = 0;
      out.count[b] = 0;
    }
    return;
  }

  double* S = ws + (int64_t)W_S * cap;
  double* DS = ws + (int64_t)W_DS * cap;
  double* DL = ws + (int64_t)W_DL * cap;
  double* Cn = ws + (int64_t)W_C * cap;
  double* KD = ws + (int64_t)W_KIND * cap;
  double* W = ws + (int64_t)W_W * cap;
  double* T = ws + (int64_t)W_T * cap;

  // ---- geometry: delta_i, ds_i (lanes over nodes) and S (serial sum)
  {
    double carry = 0.0;
    if (c.lane == 0) S[0] = 0.0;
    for (int base = 0; base < n; base += C::width) {
      const int i = base + c.lane;
      double ds = 0.0;
      if (i < n) {
        const double* r = P + 5 * (int64_t)i;
        DL[i] = atan_(m.L() * r[3]);
        if (i < n - 1) {
          ds = hypot_(r[5] - r[0], r[6] - r[1]);
          DS[i] = ds;
        }
      }
      const int cnt = n - 1 - base < C::width ? n - 1 - base : C::width;
      const double s = scan_add_serial(c, ds, carry, cnt);
      if (i < n - 1) S[i + 1] = s;
    }
  }
  c.sync();

  // ---- node caps and their kind (lanes over nodes)
  for (int i = c.lane; i < n; i += C::width) {
    const double* r = P + 5 * (int64_t)i;
    const double k = r[3], dir = r[4];
    const bool stop = i < n - 1 && r[9] != dir;
    double vmax = inf_(), sr = inf_(), endp = inf_();
    if (i > 0) {                                   // interval i-1, gear dir_i
      vmax = dir > 0.0 ? m.vf() : m.vr();
      const double dd = DL[i] - DL[i - 1];
      if (m.omega() > 0.0 && dd != 0.0) sr = m.omega() * DS[i - 1] / fabs(dd);
    }
    if (i < n - 1) {                               // interval i, gear dir_{i+1}
      vmax = min_(vmax, r[9] > 0.0 ? m.vf() : m.vr());
      const double dd = DL[i + 1] - DL[i];
      if (m.omega() > 0.0 && dd != 0.0) sr = min_(sr, m.omega() * DS[i] / fabs(dd));
    }
    const double al = (m.alat() > 0.0 && k != 0.0) ? sqrt(m.alat() / fabs(k)) : inf_();
    if (i == 0) endp = m.v0();
    if (i == n - 1) endp = min_(endp, m.v1());
    const double cc = min_(min_(min_(min_(stop ? 0.0 : inf_(), vmax), al), sr), endp);
    int kind = HTP_SPD_A_ENDPOINT;
    if (sr == cc) kind = HTP_SPD_A_STEER_RATE;
    if (al == cc) kind = HTP_SPD_A_ALAT;
    if (vmax == cc) kind = HTP_SPD_A_VMAX;
    if (stop) kind = HTP_SPD_A_STOP;               // 0 is the least a cap can be
    Cn[i] = cc;
    KD[i] = (double)kind;
  }
  c.sync();

  // ---- forward pass: f_i = min(c_i^2, 2 acc S_i + min_{j<i}(c_j^2 - 2 acc S_j))
  {
    const double a2 = 2.0 * m.acc();
    double carry = inf_();
    for (int base = 0; base < n; base += C::width) {
      const int i = base + c.lane;
      const bool act = i < n;
      const double c2 = act ? Cn[i] * Cn[i] : inf_();
      const double sh = act ? a2 * S[i] : 0.0;
      const double before = scan_min_before(c, act ? c2 - sh : inf_(), carry);
      if (act) W[i] = min_(c2, sh + before);
    }
  }
  c.sync();

  // ---- backward pass, from the last node: w_i = min(f_i, min_{j>i}(f_j + 2 dec S_j) - 2 dec S_i); active kind
  {
    const double d2 = 2.0 * m.dec();
    double carry = inf_();
    for (int top = n - 1; top >= 0; top -= C::width) {
      const int i = top - c.lane;
      const bool act = i >= 0;
      const double f = act ? W[i] : inf_();
      const double sh = act ? d2 * S[i] : 0.0;
      const double after = scan_min_before(c, act ? f + sh : inf_(), carry);
      if (act) {
        const double bwd = after - sh;
        const double w = min_(f, bwd);
        const double c2 = Cn[i] * Cn[i];
        if (w != c2) KD[i] = (double)((f < c2 && f < bwd) ? HTP_SPD_A_ACC : HTP_SPD_A_DEC);
        W[i] = w;
      }
    }
  }
  c.sync();

  // ---- interval times; t and the summary's sums, added in node order
  double len_f = 0.0, len_r = 0.0, dwell = 0.0, tk[NKIND];
  for (int j = 0; j < NKIND; ++j) tk[j] = 0.0;
  double peak_v = 0.0;
  int hops = 0;
  {
    double tc = 0.0;
    if (c.lane == 0) T[0] = 0.0;
    for (int base = 0; base < n - 1; base += C::width) {
      const int i = base + c.lane;
      double dt = 0.0, ds = 0.0, code = 0.0;
      if (i < n - 1) {
        ds = DS[i];
        const Interval iv = interval_(W[i], W[i + 1], ds, DL[i + 1] - DL[i], m);
        dt = iv.dt;
        if (iv.kind == 2) { ++hops; peak_v = max_(peak_v, iv.vm); }
        code = KD[i] + (P[5 * (int64_t)(i + 1) + 4] > 0.0 ? 8.0 : 0.0) + (iv.kind == 1 ? 16.0 : 0.0);
      }
      const int cnt = n - 1 - base < C::width ? n - 1 - base : C::width;
      double mine = tc;
      for (int k = 0; k < cnt; ++k) {
        const double dtk = c.bcast(dt, k), dsk = c.bcast(ds, k);
        const int ck = (int)c.bcast(code, k);
        tc = tc + dtk;
        if (c.lane == k) mine = tc;
        len_f = len_f + ((ck & 8) ? dsk : 0.0);
        len_r = len_r + ((ck & 8) ? 0.0 : dsk);
        dwell = dwell + ((ck & 16) ? dtk : 0.0);
        for (int j = 0; j < NKIND; ++j) tk[j] = tk[j] + ((ck & 7) == j ? dtk : 0.0);
      }
      if (i < n - 1) T[i + 1] = mine;
    }
  }
  c.sync();
  const double Ttot = T[n - 1];

  // ---- per-node outputs and the order-independent reductions
  double peak_lat = 0.0, max_dl = 0.0;
  int stops = 0;
  for (int i = c.lane; i < n; i += C::width) {
    const double* r = P + 5 * (int64_t)i;
    const double w = W[i], v = sqrt(w);
    peak_v = max_(peak_v, v);
    peak_lat = max_(peak_lat, w * fabs(r[3]));
    max_dl = max_(max_dl, fabs(DL[i]));
    double g = r[4], a = 0.0, rate = 0.0;
    if (i < n - 1) {
      g = r[9];
      if (g != r[4]) ++stops;
      if (out.node) {
        const double dd = DL[i + 1] - DL[i];
        const Interval iv = interval_(w, W[i + 1], DS[i], dd, m);
        a = iv.a;
        rate = iv.dt > 0.0 ? dd / iv.dt : 0.0;
      }
    }
    if (out.node) {
      double* o = out.node + (b * (int64_t)cap + i) * NNODE;
      o[HTP_SPD_N_S] = S[i];
      o[HTP_SPD_N_T] = T[i];
      o[HTP_SPD_N_V] = g * v;
      o[HTP_SPD_N_ACC] = g * a;
      o[HTP_SPD_N_STEER] = DL[i];
      o[HTP_SPD_N_STEER_RATE] = rate;
      o[HTP_SPD_N_CAP] = Cn[i];
    }
    if (out.active) out.active[b * (int64_t)cap + i] = (int32_t)KD[i];
  }
  peak_v = c.maxv(peak_v);
  peak_lat = c.maxv(peak_lat);
  max_dl = c.maxv(max_dl);
  stops = c.isum(stops);
  hops = c.isum(hops);
  int flags = (hops > 0 ? HTP_SPD_F_HOP : 0) | (max_dl > m.max_steer() ? HTP_SPD_F_STEER_EXCEEDS : 0);

  // ---- fixed-period rows: k dt while k dt < T, then the last node at T
  int need = 0;
  if (in.dt > 0.0) {
    const double dt = in.dt;
    const int capr = in.cap_rows;
    const double quot = Ttot / dt;
    if (!(quot < MAX_QUOTIENT)) {
      flags |= HTP_SPD_F_BAD_TIME;
    } else {
      int nr = (int)quot;   // the smallest nr with fl(nr dt) >= T: the quotient is off by one at the most
      for (int q = 0; q < 2 && nr > 0 && (double)(nr - 1) * dt >= Ttot; ++q) --nr;
      for (int q = 0; q < 2 && (double)nr * dt < Ttot; ++q) ++nr;
      need = nr + 1;
      if (need > capr) flags |= HTP_SPD_F_TRUNCATED;
      const int nw = need < capr ? need : capr;
      double* rows = out.rows + b * (int64_t)capr * NCOL;
      for (int r0 = 0; r0 < nw; r0 += CHUNK) {
        const int nt = nw - r0 < CHUNK ? nw - r0 : CHUNK;
        c.sync();   // the previous chunk's tile is no longer read
        for (int j = c.lane; j < nt; j += C::width) {
          const int r = r0 + j;
          double* row = tile + NCOL * j;
          int i;
          if (r < nr) {
            const double s = (double)r * dt;
            int lo = 0, hi = n - 2;   // the largest i in 0..n-2 with t_i <= s (t_0 = 0 <= s < T, so dt_i > 0)
            while (lo < hi) {
              const int mid = (lo + hi + 1) >> 1;
              if (T[mid] <= s) lo = mid; else hi = mid - 1;
            }
            i = lo;
            const double* p0 = P + 5 * (int64_t)i;
            const double tau = s - T[i], ds = DS[i], dd = DL[i + 1] - DL[i], g = p0[9];
            const Interval iv = interval_(W[i], W[i + 1], ds, dd, m);
            double dist = 0.0, v = 0.0, a = 0.0, lam;
            if (iv.kind == 1) {
              lam = tau / iv.dt;
            } else {
              if (iv.kind == 0) {
                dist = iv.vi * tau + 0.5 * iv.a * tau * tau;
                v = iv.vi + iv.a * tau;
                a = iv.a;
              } else if (tau < iv.t1) {
                dist = 0.5 * m.acc() * tau * tau;
                v = m.acc() * tau;
                a = m.acc();
              } else {
                const double t2 = tau - iv.t1;
                dist = 0.5 * m.acc() * iv.t1 * iv.t1 + iv.vm * t2 - 0.5 * m.dec() * t2 * t2;
                v = iv.vm - m.dec() * t2;
                a = -m.dec();
              }
              lam = dist / ds;
            }
            lam = lam < 0.0 ? 0.0 : (lam > 1.0 ? 1.0 : lam);
            const double k = p0[3] + lam * (p0[8] - p0[3]);
            row[C_T] = s;
            row[C_X] = p0[0] + lam * (p0[5] - p0[0]);
            row[C_Y] = p0[1] + lam * (p0[6] - p0[1]);
            row[C_V] = g * v;
            row[C_TH] = p0[2] + lam * wrap_(p0[7] - p0[2]);
            row[C_ST] = atan_(m.L() * k);
            row[C_ACC] = g * a;
            row[C_SR] = iv.dt > 0.0 ? dd / iv.dt : 0.0;
            row[C_CURV] = k;
            row[C_ARC] = S[i] + dist;
          } else {                     // the final row: the last node, in the last interval's gear
            i = n - 1;
            const double* pn = P + 5 * (int64_t)i;
            const double dd = DL[i] - DL[i - 1];
            const Interval iv = interval_(W[i - 1], W[i], DS[i - 1], dd, m);
            row[C_T] = Ttot;
            row[C_X] = pn[0];
            row[C_Y] = pn[1];
            row[C_V] = pn[4] * sqrt(W[i]);
            row[C_TH] = pn[2];
            row[C_ST] = DL[i];
            row[C_ACC] = pn[4] * (iv.kind == 2 ? -m.dec() : iv.a);
            row[C_SR] = iv.dt > 0.0 ? dd / iv.dt : 0.0;
            row[C_CURV] = pn[3];
            row[C_ARC] = S[i];
          }
          if (out.stage) out.stage[b * (int64_t)capr + r] = i;
        }
        c.sync();
        for (int q = c.lane; q < nt * NCOL; q += C::width) rows[(int64_t)r0 * NCOL + q] = tile[q];
      }
    }
  }

  if (c.lane == 0) {
    double* sm = out.summary + b * NSUM;
    sm[HTP_SPD_S_T] = Ttot;
    sm[HTP_SPD_S_LENGTH] = S[n - 1];
    sm[HTP_SPD_S_LEN_FWD] = len_f;
    sm[HTP_SPD_S_LEN_REV] = len_r;
    sm[HTP_SPD_S_STOPS] = (double)stops;
    sm[HTP_SPD_S_DWELL] = dwell;
    sm[HTP_SPD_S_PEAK_V] = peak_v;
    sm[HTP_SPD_S_PEAK_LAT] = peak_lat;
    sm[HTP_SPD_S_MAX_STEER] = max_dl;
    for (int j = 0; j < NKIND; ++j) sm[HTP_SPD_S_TIME_KIND + j] = tk[j];
    out.status[b] = HTP_SPD_OK;
    out.flags[b] = flags;
    out.count[b] = need;
  }
}

}  // namespace spd
}  // namespace htp

#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC pop_options
#endif
