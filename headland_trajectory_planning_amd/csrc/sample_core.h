// Sampled exit / entry pose search of the classic turns (include/htp.h): one candidate of one turn
// per 64-lane wavefront.  The candidate's path comes from the classic planner (classic_core.h Turn::dubins_full /
// circleback, rs_core.h words) unchanged; this file adds what the sampling variants of
// R/path_planner/safety_forward_path_plan.py:457-790 put on top of it:
//
//   feasible .. check_path_feasibility(car, path, boundary_check=False, aux_check=True)  orchard_geometry_environment.py
//               :423-458: the body at every row, each implement at every second row (car_model.get_path_poly :39-73),
//               against the blockers with ha::Footprint::sat_hit (closed sets)
//   score ..... get_min_distance_to_boundary(car, path, with_aux=True)  :393-412: the least signed distance of a placed
//               corner to the field ring (ring_signed_distance below)
//   winner .... the strict > of the reference's loops: the largest score, ties to the lowest flattened index
//
// Lane-parallel over path rows (Dubins, circle-back) or one Reeds-Shepp word per lane (ScoreSink, the fish-tail's
// CheckSink with the running minimum and the row parity).  The polygons of the turn live in a Scene (LDS on the
// device); the corner arrays have four entries indexed by constants, so nothing here needs private memory.
#pragma once
#include <cmath>
#include <cstdint>

#include "classic_core.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace htp {
namespace smp {

enum { T_DUBINS = 0, T_REEDS_SHEPP = 1, T_CIRCLE_BACK = 2 };
enum { ST_OK = 0, ST_NONE_FEASIBLE = 1, ST_OVERFLOW = 2, ST_BAD_INPUT = 3 };
enum { C_FEASIBLE = 0, C_BLOCKED = 1, C_PLANNER = 2, C_OVERFLOW = 3, C_BAD_INPUT = 4, C_UNUSED = 5 };
constexpr int MAXPOLY = 48, MAXVERT = 256, NCORNER = 4;
constexpr int WS_PER_POINT = ct::SCR_PER_POINT + 5;   // doubles per sample: the Dubins scratch and one path row

HTP_HD inline double inf() { return __builtin_huge_val(); }
HTP_HD inline bool finite_(double v) { return v - v == 0.0; }

// The polygons of one turn, renumbered: 0 the body, 1 .. naux the implements, [blk0, blk1) the blockers, `field` the
// field ring.  off / vert are what ha::Footprint::g reads.
struct Scene {
  double vert[2 * MAXVERT];
  int32_t off[MAXPOLY + 1];
  int32_t naux, blk0, blk1, field;
};

// Signed distance of (X, Y) to the ring V[m]: Euclidean distance to the nearest segment, positive inside (the
// crossing-number rule of ha::Footprint::in_field), negative outside.
HTP_HD inline double ring_signed_distance(const double* V, int m, double X, double Y) {
  bool inside = false;
  double d2 = inf();
  for (int i = 0; i < m; ++i) {
    const int j = (i + 1) == m ? 0 : i + 1;
    const double xi = V[2 * i], yi = V[2 * i + 1], xj = V[2 * j], yj = V[2 * j + 1];
    if ((yi > Y) != (yj > Y)) {
      const double xc = (xj - xi) * (Y - yi) / (yj - yi) + xi;
      if (X < xc) inside = !inside;
    }
    const double ex = xj - xi, ey = yj - yi;
    const double ee = ex * ex + ey * ey;
    double t = ee > 0.0 ? ((X - xi) * ex + (Y - yi) * ey) / ee : 0.0;
    t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
    const double px = (xi + t * ex) - X, py = (yi + t * ey) - Y;
    const double q = px * px + py * py;
    if (q < d2) d2 = q;
  }
  const double d = sqrt(d2);
  return inside ? d : -d;
}

// One path row: the body (and on even rows the implements) at the pose against the blockers; when nothing is hit,
// the corners' signed distances go into dmin.  The rotation is the footprint's (ha::Footprint::pose_hits_t).
HTP_HD inline void eval_pose(const Scene& S, const ha::Footprint& fp, double x, double y, double yaw, bool even,
                             bool& hit, double& dmin) {
  double sn, cs;
  fm::sincos(yaw, sn, cs);
  const int np = even ? 1 + S.naux : 1;
  const double* F = S.vert + 2 * S.off[S.field];
  const int nf = S.off[S.field + 1] - S.off[S.field];
  for (int q = 0; q < np; ++q) {
    const double* B = S.vert + 2 * S.off[q];
    double bx[NCORNER], by[NCORNER];
#pragma unroll
    for (int k = 0; k < NCORNER; ++k) {
      const double vx = B[2 * k], vy = B[2 * k + 1];
      bx[k] = cs * vx + (-sn) * vy + x;
      by[k] = sn * vx + cs * vy + y;
    }
    for (int p = S.blk0; p < S.blk1; ++p)
      if (fp.sat_hit<NCORNER>(bx, by, p)) { hit = true; return; }
#pragma unroll
    for (int k = 0; k < NCORNER; ++k) {
      const double d = ring_signed_distance(F, nf, bx[k], by[k]);
      if (d < dmin) dmin = d;
    }
  }
}

// per-lane check of one Reeds-Shepp word: ct::Turn::CheckSink with the running minimum and the row parity
struct ScoreSink {
  const Scene* S;
  const ha::Footprint* fp;
  double sx, sy, syaw, cq, sq;
  int n, cur = 0;
  double px = 0, py = 0, pyaw = 0;
  bool have = false, hit = false;
  double dmin = inf();
  HTP_HD void test(int k) {
    if (!have || k >= n || hit) return;
    const double gx = cq * px + sq * py + sx, gy = -sq * px + cq * py + sy;
    eval_pose(*S, *fp, gx, gy, rs::pi2pi(pyaw + syaw), (k & 1) == 0, hit, dmin);
  }
  HTP_HD void put(int k, double lx, double ly, double lyaw, double, int) {
    if (k != cur) test(cur);   // index advanced: the previous entry is final
    cur = k; px = lx; py = ly; pyaw = lyaw; have = true;
  }
};

HTP_HD inline ha::Footprint footprint_of(const Scene& S) {
  ha::Footprint fp{};
  fp.g.poly_off = S.off;
  fp.g.vert = S.vert;
  fp.body = S.vert;
  fp.nb = NCORNER;
  fp.blk0 = S.blk0;
  fp.blk1 = S.blk1;
  fp.field = -1;
  fp.lane0 = 0;
  fp.lane1 = 0;
  return fp;
}

// One candidate: sp carries the candidate's poses.  ws: WS_PER_POINT * cap doubles of this wavefront (HBM), paths:
// rs::MAXP slots shared by the wavefront.  Returns C_* (uniform); score is -inf unless C_FEASIBLE.
// MASK: the turn types (1 << T_*) this instance is compiled for -- the device has one kernel for the Reeds-Shepp
// words and one for the Dubins / circle-back rows, so that the second carries none of the first's registers.
constexpr int M_ROWS = (1 << T_DUBINS) | (1 << T_CIRCLE_BACK), M_WORDS = 1 << T_REEDS_SHEPP, M_ALL = M_ROWS | M_WORDS;
template <int MASK, class C>
HTP_HD inline int run_candidate(C& c, const ct::Spec& sp, const Scene& S, double* ws, int cap, rs::Path* paths,
                                double& score) {
  score = -inf();
  const ha::Footprint fp = footprint_of(S);
  if ((MASK & M_WORDS) && sp.type == T_REEDS_SHEPP) {
    const double maxc = 1.0 / sp.radius, step = sp.step;
    rs::PathSet PS{paths, 0, 0};
    if (c.lane == 0 || C::width == 1)
      rs::generate_paths(sp.start[0], sp.start[1], sp.start[2], sp.end[0], sp.end[1], sp.end[2], maxc, PS);
    c.sync();
    const int np_ = c.uniform_i(PS.n), err = c.uniform_i(PS.err);
    if (err || np_ <= 0) return C_PLANNER;
    int bad = 0, ovf = 0, feas = 0;
    double best = -inf();
    const double cq = hm::cos(-sp.start[2]), sq = hm::sin(-sp.start[2]);
    for (int p = c.lane; p < np_; p += C::width) {
      rs::NullSink ns;
      const int n = rs::local_course(paths[p], maxc, step * maxc, ns);
      if (n < 0) { bad = 1; continue; }
      if (n > cap) { ovf = 1; continue; }
      ScoreSink sk{&S, &fp, sp.start[0], sp.start[1], sp.start[2], cq, sq, n};
      rs::local_course(paths[p], maxc, step * maxc, sk);
      sk.test(sk.cur);
      if (!sk.hit) {
        feas = 1;
        if (sk.dmin > best) best = sk.dmin;
      }
    }
    c.sync();
    bad = c.isum(bad);
    ovf = c.isum(ovf);
    feas = c.isum(feas);
    best = c.maxv(best);
    if (bad) return C_PLANNER;
    if (ovf) return C_OVERFLOW;
    if (!feas) return C_BLOCKED;
    score = best;
    return C_FEASIBLE;
  }
  if (!(MASK & M_ROWS) || sp.type == T_REEDS_SHEPP) return C_PLANNER;   // not this instance's type: never reached
  double* rows = ws + (int64_t)ct::SCR_PER_POINT * cap;
  ct::Turn<C> T{c, sp, fp, ws, cap, rows, cap, paths, nullptr};
  if (sp.type == T_DUBINS) {
    const int n = T.dubins_full(sp.start, sp.end, sp.radius, sp.step, 0, false, false);
    if (n >= 0) T.n_out = n;
  } else {
    T.circleback();
  }
  if (T.status == ct::ST_OVERFLOW) return C_OVERFLOW;
  if (T.status != ct::ST_OK || T.n_out < 1) return C_PLANNER;
  c.sync();
  int hit = 0;
  double dmin = inf();
  for (int k = c.lane; k < T.n_out; k += C::width) {
    const double* r = rows + 5 * (int64_t)k;
    bool h = false;
    eval_pose(S, fp, r[0], r[1], r[2], (k & 1) == 0, h, dmin);
    if (h) hit = 1;
  }
  c.sync();
  if (c.isum(hit) != 0) return C_BLOCKED;
  score = c.minv(dmin);
  return C_FEASIBLE;
}

}  // namespace smp
}  // namespace htp
