// Swept-footprint envelope of one solved OBCA trajectory (FORM 0, R/obca_py/optimizer.py layout): the extent of the
// placed body polygons over the audit's poses (the N nodes and S - 1 poses inside every interval) in a caller-given
// frame, with the (stage, substep, body) that attains each side, and the occupancy raster of the swept region on a
// W x H grid of that frame (cells per body, the union, the union's bitmap).  include/htp.h holds the definition.
// One problem per 64-lane wavefront on gfx950 (htp_envelope.hip) or a single serial lane (envelope_hostsim.cpp,
// tests only); one __host__ __device__ source, so both produce the same doubles and the same bits:
//   - no contraction (pragma below) and the planner libm (htp_libm.h) for sin, cos and tan;
//   - the integrator, the halfspace-to-edge construction and the pose staging are audit_core.h's, unedited;
//   - every quantity is a minimum or a maximum with its index (ties to the lowest index), a bit OR or a
//     population count: nothing depends on the order of evaluation.
// Only X, U and tau of the decision vector, the body rows, the frame and the dT and wheelbase parameters are read.
//
// Raster mapping: the bodies one after the other; for body k the poses one after the other; for one pose the
// lanes are strided over the 32-cell words of the rows of the pose's bounding box.  Within one pose every word
// belongs to one lane, and the poses follow each other in the wavefront's program order, so the words are
// updated with a plain read-OR-write: no LDS atomics.  A lane evaluates its word in blocks of eight cells whose
// body-frame coordinates stay in registers while the edges pass by, so an edge is read from LDS once per eight
// cells (a lane per cell would read three doubles per four multiply-adds and be bound by LDS).  Cells that an
// earlier pose of the same body covers are skipped: consecutive poses overlap in all but a sliver.
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

#if defined(__clang__)
#define HTP_ENV_UNROLL _Pragma("unroll")
#define HTP_ENV_NOUNROLL _Pragma("unroll 1")
#else
#define HTP_ENV_UNROLL
#define HTP_ENV_NOUNROLL
#endif

namespace htp {
namespace envelope {

using audit::ER;
using audit::INF;
using audit::State;
constexpr int MAXN = HTP_ENVELOPE_MAX_N;
constexpr int MAXCELLS = HTP_ENVELOPE_MAX_CELLS;
constexpr int CHUNK_POSES = audit::CHUNK_POSES;
constexpr int TEB_MAX = audit::TEB_MAX;
constexpr int BW = MAXCELLS / 32;    // words of one bitmap
constexpr int BLK = 8;               // cells a lane evaluates at once
static_assert(MAXN <= audit::MAXN && MAXN >= 160, "the horizon limit");
// fixed LDS (doubles): body edges | polygon (first row, edge count) | poses (x, y, cos, sin) | per-pose bounding
// box (four uint16 in one double's place) | the bodies' extents (value, index); the raw halfspace rows live in
// the pose area until the edges are built
constexpr int L_EB = 0, L_PI = L_EB + ER * TEB_MAX, L_POSE = L_PI + 2 * MAXK, L_BOX = L_POSE + 4 * CHUNK_POSES;
constexpr int L_SIDE = L_BOX + CHUNK_POSES, L_FIXED = L_SIDE + 8 * MAXK;
static_assert(3 * TEB_MAX <= 4 * CHUNK_POSES, "raw rows fit the pose area");
// LDS asked for at the launch (doubles): body bitmap | union bitmap, each of H W / 32 words rounded up to 16
// bytes, so a small grid leaves room for more wavefronts per compute unit; then, per stage,
// X 5N | U 2(N-1) | tau N-1, then h N-1
HTP_HD inline int lds_stage_doubles(int N) { return 8 * N; }
HTP_HD inline int bitmap_words(int W, int H) { return (H * (W / 32) + 3) & ~3; }
HTP_HD inline int lds_dyn_doubles(int N, int W, int H) { return bitmap_words(W, H) + lds_stage_doubles(N); }
static_assert((L_FIXED + BW + 8 * MAXN) * 8 <= 65536, "LDS of the largest horizon with a full grid fits 64 KB");
constexpr double SLACK = 1e-9;       // see box_of

struct Shape {   // launch-uniform
  int N, K, topt, S, W, H;
  int eb[MAXK], offb[MAXK];
  int TEb;
  int64_t stride;   // doubles between two problems' x rows
  int oTAU;         // offset of tau inside a row (X at 0, U behind X)
  double res;
};

struct Batch {   // device or host pointers
  const double *bodyG, *bodyg, *params, *x, *frame;
  double* extent;
  int32_t* where;
  double* extent_body;   // nullable
  int32_t* cells;        // not written without a raster
  uint32_t* bitmap;      // nullable
  int32_t* flags;
};

HTP_HD inline void make_shape(Shape& s, const htp_obca_batch& in, const htp_obca_envelope_opts& o) {
  s.N = in.N; s.K = in.K; s.topt = in.time_opt ? 1 : 0; s.S = o.substeps; s.W = o.W; s.H = o.H;
  s.res = o.W > 0 ? o.res : 1.0;
  s.TEb = 0;
  for (int k = 0; k < MAXK; ++k) { s.eb[k] = 0; s.offb[k] = 0; }
  for (int k = 0; k < in.K; ++k) { s.eb[k] = in.body_edges[k]; s.offb[k] = s.TEb; s.TEb += s.eb[k]; }
  Dims D;
  make_dims(D, in.N, in.M, in.K, in.time_opt, in.obs_edges, in.body_edges);
  s.stride = D.n; s.oTAU = D.oTAU;
}

// The serial lane of the test-only host build; the gfx950 wavefront is in htp_envelope.hip.
struct HostLane : audit::HostLane {
  int sumi(int v) const { return v; }
  double uniform(double v) const { return v; }
  void store_words(uint32_t* dst, const uint32_t* src, int n) const {
    for (int q = 0; q < n; ++q) dst[q] = src[q];
  }
};

// One side of the extent: the value, negated for a maximum so that both are minima, and the flattened index.
struct Side {
  double v;
  int i;
  HTP_HD inline void take(double nv, int ni) { if (nv < v) { v = nv; i = ni; } }
  HTP_HD inline void merge(const Side& o) { if (o.v < v || (o.v == v && o.i < i)) { v = o.v; i = o.i; } }
};

// Cells [lo, hi] of one axis (n cells of side res) that may hold a covered centre when the polygon spans [u0, u1]
// on that axis.  A covered centre a = (i + 0.5) res lies in [u0, u1] up to the rounding of the cell test, so
// i lies in [floor(u0 / res), floor(u1 / res)]: u0 / res - 0.5 <= i gives i >= floor(u0 / res), and
// i <= u1 / res - 0.5 gives i <= floor(u1 / res).  The box takes one cell more on either side and first widens
// the span by SLACK times the magnitudes that enter the test.  That is enough: the test's ten-odd roundings and
// the rounding of the vertices are below 1e-14 of those magnitudes for a polygon whose rows are further than
// PAR_EPS from parallel, five orders below SLACK, and the quotient's own rounding moves the floor by at most the
// spare cell.  Anything non-finite opens the whole axis.  hi < lo: no cell.
HTP_HD inline void box_of(double u0, double u1, double scale, double res, int n, int& lo, int& hi) {
  const double sl = SLACK * scale;
  const double a0 = floor((u0 - sl) / res) - 1.0, a1 = floor((u1 + sl) / res) + 1.0;
  lo = a0 > 0.0 ? (a0 < (double)n ? (int)a0 : n) : 0;
  hi = a1 < (double)(n - 1) ? (a1 >= 0.0 ? (int)a1 : -1) : n - 1;
}

// The problem is not evaluated: extent NaN, where -1, cells 0, the bitmap zeroed.
template <class W>
HTP_HD inline void reject(const W& c, const Shape& sh, const Batch& b, int64_t p, int flag, uint32_t* zero) {
  const double NaN = __builtin_nan("");
  const int K = sh.K;
  if (b.extent_body)
    for (int q = c.lane; q < 4 * K; q += c.width) b.extent_body[p * 4 * K + q] = NaN;
  if (sh.W > 0) {
    for (int q = c.lane; q <= K; q += c.width) b.cells[p * (K + 1) + q] = 0;
    if (b.bitmap) {
      const int nw = sh.H * (sh.W / 32);
      for (int q = c.lane; q < nw; q += c.width) zero[q] = 0u;
      c.sync();
      c.store_words(b.bitmap + p * (int64_t)nw, zero, nw);
    }
  }
  if (c.lane == 0) {
    for (int q = 0; q < 4; ++q) b.extent[p * 4 + q] = NaN;
    for (int q = 0; q < 12; ++q) b.where[p * 12 + q] = -1;
    b.flags[p] = flag;
  }
}

// One problem.  sl: L_FIXED doubles of LDS, dl: lds_dyn_doubles(N, W, H) doubles of LDS (both 16-byte aligned).
template <class W>
HTP_HD inline void run_problem(const W& c, const Shape& sh, const Batch& b, int64_t p, double* sl, double* dl) {
  const int N = sh.N, K = sh.K, S = sh.S, topt = sh.topt, GW = sh.W, GH = sh.H, WPR = sh.W / 32;
  const bool raster = GW > 0;
  const double res = sh.res;
  const int nwp = bitmap_words(GW, GH);
  uint32_t* bbody = (uint32_t*)dl;
  uint32_t* bunion = bbody + nwp;
  double* X = dl + nwp;
  double* U = X + 5 * N;
  double* T = U + 2 * (N - 1);   // tau, then h
  double* Eb = sl + L_EB;
  double* pinfo = sl + L_PI;
  double* pose = sl + L_POSE;
  double* rawB = pose;
  uint32_t* box = (uint32_t*)(sl + L_BOX);
  double* side = sl + L_SIDE;   // body k: four values (maxima negated), then their four indices
  const double* par = b.params + p * NPARAM;
  const double* fr = b.frame + p * 3;

  // ---- the doubles read: X, U (one run), tau; the body rows; the frame; dT and the wheelbase
  bool bad = false;
  const double* xr = b.x + p * sh.stride;
  c.load_run(X, xr, 5 * N + 2 * (N - 1), bad);
  if (topt) c.load_run(T, xr + sh.oTAU, N - 1, bad);
  for (int r = c.lane; r < sh.TEb; r += c.width) {
    const double ax = b.bodyG[(p * sh.TEb + r) * 2], ay = b.bodyG[(p * sh.TEb + r) * 2 + 1], bb = b.bodyg[p * sh.TEb + r];
    rawB[3 * r] = ax; rawB[3 * r + 1] = ay; rawB[3 * r + 2] = bb;
    bad = bad || audit::nonfinite_(ax) || audit::nonfinite_(ay) || audit::nonfinite_(bb);
  }
  const double dT = c.uniform(par[P_DT]), wb = c.uniform(par[P_WHEELBASE]);
  const double ox = c.uniform(fr[0]), oy = c.uniform(fr[1]), phi = c.uniform(fr[2]);
  bad = bad || audit::nonfinite_(dT) || audit::nonfinite_(wb) || audit::nonfinite_(ox) || audit::nonfinite_(oy) ||
        audit::nonfinite_(phi);
  bad = c.any(bad);
  c.sync();
  if (bad) { reject(c, sh, b, p, HTP_ENVELOPE_NONFINITE, bunion); return; }

  // ---- body polygons: one row per lane, then one polygon per lane compacts its edges in place
  for (int r = c.lane; r < sh.TEb; r += c.width) {
    int first = 0, cnt = 0;
    for (int k = 0; k < K; ++k)
      if (r >= sh.offb[k] && r < sh.offb[k] + sh.eb[k]) { first = sh.offb[k]; cnt = sh.eb[k]; }
    audit::build_row(rawB, first, cnt, r, Eb + ER * r);
  }
  c.sync();
  for (int k = c.lane; k < K; k += c.width) {
    const int first = sh.offb[k], cnt = sh.eb[k];
    double* E = Eb + ER * first;
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
    pinfo[2 * k] = (double)first;
    pinfo[2 * k + 1] = (pb || n < 3) ? -1.0 : (double)n;
  }
  c.sync();
  bool polybad = false;
  for (int k = 0; k < K; ++k) polybad = polybad || pinfo[2 * k + 1] < 0.0;
  if (polybad) { reject(c, sh, b, p, HTP_ENVELOPE_BAD_POLYTOPE, bunion); return; }

  // ---- step lengths, one stage per lane; the bitmaps start empty
  for (int i = c.lane; i < N - 1; i += c.width) T[i] = topt ? dT * T[i] : dT;
  const int nw = GH * WPR;
  for (int q = c.lane; q < nw; q += c.width) { bbody[q] = 0u; bunion[q] = 0u; }
  double sphi_, cphi_;
  hm::sincos(phi, sphi_, cphi_);
  const double sphi = c.uniform(sphi_), cphi = c.uniform(cphi_);
  const double gridmag = c.uniform(audit::dabs_(ox) + audit::dabs_(oy) + ((double)GW + (double)GH) * res);

  const int CS = CHUNK_POSES / S;
  for (int k = 0; k < K; ++k) {
    const double* E = Eb + ER * (int)pinfo[2 * k];
    const int nb = (int)pinfo[2 * k + 1];
    Side umin{INF, 0x7fffffff}, umax{INF, 0x7fffffff}, vmin{INF, 0x7fffffff}, vmax{INF, 0x7fffffff};
    for (int i0 = 0; i0 < N; i0 += CS) {
      const int ni = (N - i0 < CS) ? N - i0 : CS;
      c.sync();   // the previous chunk's poses (or the raw rows) are no longer read
      for (int t = c.lane; t < ni * S; t += c.width) {
        const int i = i0 + t / S, q = t % S;
        State s{X[5 * i], X[5 * i + 1], X[5 * i + 2], X[5 * i + 3], X[5 * i + 4]};
        if (q > 0 && i < N - 1) s = audit::step(s, U[2 * i], U[2 * i + 1], wb, T[i] * (double)q / (double)S, topt);
        double sn, cs;
        hm::sincos(s.th, sn, cs);
        pose[4 * t] = s.x; pose[4 * t + 1] = s.y; pose[4 * t + 2] = cs; pose[4 * t + 3] = sn;
      }
      c.sync();
      // extent of body k at every pose of the chunk, in frame coordinates; its bounding box in cells
      for (int t = c.lane; t < ni * S; t += c.width) {
        const int i = i0 + t / S, q = t % S;
        const double px = pose[4 * t], py = pose[4 * t + 1], cs = pose[4 * t + 2], sn = pose[4 * t + 3];
        double u0 = INF, u1 = -INF, v0 = INF, v1 = -INF;
        const bool real = !(q > 0 && i == N - 1);   // the last node starts no interval
        if (real) {
          for (int j = 0; j < nb; ++j) {
            const double vx = E[ER * j + 3], vy = E[ER * j + 4];
            const double wx = px + (cs * vx - sn * vy), wy = py + (sn * vx + cs * vy);
            const double dx = wx - ox, dy = wy - oy;
            const double u = cphi * dx + sphi * dy, v = cphi * dy - sphi * dx;
            u0 = audit::dmin_(u0, u); u1 = audit::dmax_(u1, u);
            v0 = audit::dmin_(v0, v); v1 = audit::dmax_(v1, v);
          }
          const int idx = ((i0 * S + t) * K) + k;   // = (i S + q) K + k, ascending per lane
          umin.take(u0, idx); umax.take(-u1, idx); vmin.take(v0, idx); vmax.take(-v1, idx);
        }
        if (raster) {
          int ilo = 1, ihi = 0, jlo = 1, jhi = 0;
          if (real) {
            const double scale = gridmag + audit::dabs_(px) + audit::dabs_(py) + (u1 - u0) + (v1 - v0);
            box_of(u0, u1, scale, res, GW, ilo, ihi);
            box_of(v0, v1, scale, res, GH, jlo, jhi);
            if (ihi < ilo || jhi < jlo) { ilo = 1; ihi = 0; jlo = 1; jhi = 0; }
          }
          box[2 * t] = (uint32_t)ilo | ((uint32_t)ihi << 16);   // W, H <= 65 536: an index fits 16 bits
          box[2 * t + 1] = (uint32_t)jlo | ((uint32_t)jhi << 16);
        }
      }
      c.sync();
      if (!raster) continue;
      for (int t = 0; t < ni * S; ++t) {
        const uint32_t bi = box[2 * t], bj = box[2 * t + 1];
        const int ilo = (int)(bi & 0xffffu), ihi = (int)(bi >> 16), jlo = (int)(bj & 0xffffu), jhi = (int)(bj >> 16);
        if (ihi < ilo) continue;
        // the same in every lane: said so, they live in scalar registers
        const double px = c.uniform(pose[4 * t]), py = c.uniform(pose[4 * t + 1]);
        const double pc = c.uniform(pose[4 * t + 2]), ps = c.uniform(pose[4 * t + 3]);
        const int w0 = ilo >> 5, nwd = (ihi >> 5) - w0 + 1, tasks = (jhi - jlo + 1) * nwd;
        for (int task = c.lane; task < tasks; task += c.width) {
          const int j = jlo + task / nwd, w = w0 + task % nwd;
          const double bq = ((double)j + 0.5) * res;
          // cells that an earlier pose of this body already covers are not evaluated again: an OR cannot clear
          // them, and consecutive poses overlap in all but a sliver
          const uint32_t have = bbody[j * WPR + w];
          uint32_t word = 0u;
HTP_ENV_NOUNROLL
          for (int blk = 0; blk < 32; blk += BLK) {
            const int ib = 32 * w + blk;
            if (ib + BLK - 1 < ilo || ib > ihi) continue;
            const uint32_t open = ~(have >> blk) & ((1u << BLK) - 1u);
            if (!open) continue;
            double qx[BLK], qy[BLK];
            uint32_t m = 0u;
HTP_ENV_UNROLL
            for (int z = 0; z < BLK; ++z) {
              const double a = ((double)(ib + z) + 0.5) * res;
              const double wx = ox + (cphi * a - sphi * bq), wy = oy + (sphi * a + cphi * bq);
              const double dx = wx - px, dy = wy - py;
              qx[z] = pc * dx + ps * dy;
              qy[z] = pc * dy - ps * dx;
              m |= (ib + z >= ilo && ib + z <= ihi) ? (1u << z) : 0u;
            }
            m &= open;
HTP_ENV_NOUNROLL
            for (int e = 0; e < nb && m; ++e) {
              const double nx = c.uniform(E[ER * e]), ny = c.uniform(E[ER * e + 1]), bb = c.uniform(E[ER * e + 2]);
HTP_ENV_UNROLL
              for (int z = 0; z < BLK; ++z)
                if (!(nx * qx[z] + ny * qy[z] - bb <= 0.0)) m &= ~(1u << z);
            }
            word |= m << blk;
          }
          if (word) bbody[j * WPR + w] = have | word;
        }
        c.sync();   // the next pose's lanes may own other words
      }
    }
    // ---- body k is complete: its extent, its cells, its bitmap into the union
    c.min_key(umin.v, umin.i); c.min_key(umax.v, umax.i); c.min_key(vmin.v, vmin.i); c.min_key(vmax.v, vmax.i);
    if (b.extent_body && c.lane == 0) {
      double* eb = b.extent_body + (p * K + k) * 4;
      eb[0] = umin.v; eb[1] = -umax.v; eb[2] = vmin.v; eb[3] = -vmax.v;
    }
    if (c.lane == 0) {
      double* sd = side + 8 * k;
      sd[0] = umin.v; sd[1] = umax.v; sd[2] = vmin.v; sd[3] = vmax.v;
      sd[4] = (double)umin.i; sd[5] = (double)umax.i; sd[6] = (double)vmin.i; sd[7] = (double)vmax.i;
    }
    if (raster) {
      c.sync();
      int cnt = 0;
      for (int q = c.lane; q < nw; q += c.width) {
        const uint32_t v = bbody[q];
        cnt += __builtin_popcount(v);
        bunion[q] |= v;
        bbody[q] = 0u;
      }
      cnt = c.sumi(cnt);
      if (c.lane == 0) b.cells[p * (K + 1) + k] = cnt;
    }
  }

  // ---- the union's cells and bitmap; extent, where and the flag
  c.sync();
  Side all[4];
  for (int q = 0; q < 4; ++q) {   // ascending k: a tie keeps the lower flattened index
    all[q] = Side{side[q], (int)side[4 + q]};
    for (int k = 1; k < K; ++k) all[q].merge(Side{side[8 * k + q], (int)side[8 * k + 4 + q]});
  }
  const double e0 = all[0].v, e1 = -all[1].v, e2 = all[2].v, e3 = -all[3].v;
  int fl = 0;
  if (raster) {
    c.sync();
    int cnt = 0;
    for (int q = c.lane; q < nw; q += c.width) cnt += __builtin_popcount(bunion[q]);
    cnt = c.sumi(cnt);
    if (c.lane == 0) b.cells[p * (K + 1) + K] = cnt;
    if (b.bitmap) c.store_words(b.bitmap + p * (int64_t)nw, bunion, nw);
    if (e0 < 0.0 || e2 < 0.0 || e1 > (double)GW * res || e3 > (double)GH * res) fl |= HTP_ENVELOPE_CLIPPED;
  }
  if (c.lane == 0) {
    double* ex = b.extent + p * 4;
    ex[0] = e0; ex[1] = e1; ex[2] = e2; ex[3] = e3;
    int32_t* wo = b.where + p * 12;
    for (int q = 0; q < 4; ++q) {
      const int t = all[q].i / K;
      wo[3 * q] = t / S; wo[3 * q + 1] = t % S; wo[3 * q + 2] = all[q].i % K;
    }
    b.flags[p] = fl;
  }
}

}  // namespace envelope
}  // namespace htp

#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC pop_options
#endif
