// One (turn, candidate) work item and one turn's winner of an htp_classic_sample_in -> its
// htp_classic_sample_result slots; shared by the gfx950 kernels (htp_sample.hip) and the test-only host build
// (sample_hostsim.cpp).
#pragma once
#include "../../include/htp.h"
#include "sample_core.h"

namespace htp {
namespace smp {

static_assert(MAXPOLY == HTP_SMP_MAX_POLY && MAXVERT == HTP_SMP_MAX_VERT, "include/htp.h documents these limits");
static_assert((int)T_CIRCLE_BACK == (int)HTP_SMP_CIRCLE_BACK && (int)ST_BAD_INPUT == (int)HTP_SMP_BAD_INPUT &&
              (int)C_UNUSED == (int)HTP_SMP_C_UNUSED, "include/htp.h documents these values");

// Argument checks of both entries (nothing is dereferenced beyond the structs).
inline int check_args(const htp_classic_sample_in* in, const htp_classic_sample_result* out, const char** msg) {
  if (!in || !out) { *msg = "sample: null argument"; return -1; }
  if (in->batch < 0 || in->npoly < 0 || in->nvert < 0 || in->cap_s < 1 || in->cap_e < 1 || in->cap_cand < 1 ||
      in->cap_samples < 16 || in->max_groups < 0) { *msg = "sample: bad sizes"; return -1; }
  if ((int64_t)in->batch * in->cap_cand > (int64_t)1 << 40) { *msg = "sample: bad sizes"; return -1; }
  if (!in->params || !in->desc || !in->poly_off || !in->vertices || !in->start_x || !in->end_x || !in->n_start ||
      !in->n_end) { *msg = "sample: input missing"; return -1; }
  if (!out->status || !out->winner || !out->poses || !out->score || !out->n_feasible) {
    *msg = "sample: output missing";
    return -1;
  }
  if ((out->cand_score == nullptr) != (out->cand_status == nullptr)) {
    *msg = "sample: the candidate tables come as a pair";
    return -1;
  }
  return 0;
}

// Polygon ids and the CSR table as the kernels need them (host arrays): the staged entry's check.
inline int check_polygons(const htp_classic_sample_in* in, const char** msg) {
  if (in->poly_off[0] != 0 || in->poly_off[in->npoly] != in->nvert || !ha::poly_table_ok(in->poly_off, in->npoly, in->nvert)) {
    *msg = "sample: poly_off";
    return -1;
  }
  for (int64_t b = 0; b < in->batch; ++b) {
    const int32_t* d = in->desc + HTP_SMP_NDESC * b;
    auto ok = [&](int p) { return p >= 0 && p < in->npoly; };
    if (!ok(d[HTP_SMP_D_BODY]) || !ok(d[HTP_SMP_D_FIELD]) || (d[HTP_SMP_D_AUX0] != -1 && !ok(d[HTP_SMP_D_AUX0])) ||
        (d[HTP_SMP_D_AUX1] != -1 && !ok(d[HTP_SMP_D_AUX1])) || d[HTP_SMP_D_BLK0] < 0 ||
        d[HTP_SMP_D_BLK1] < d[HTP_SMP_D_BLK0] || d[HTP_SMP_D_BLK1] > in->npoly) {
      *msg = "sample: polygon ids out of range";
      return -1;
    }
  }
  return 0;
}

HTP_HD inline int poly_len(const htp_classic_sample_in& in, int p) {   // -1: id or range outside the pools
  if (p < 0 || p >= in.npoly) return -1;
  const int o0 = in.poly_off[p], o1 = in.poly_off[p + 1];
  if (o0 < 0 || o1 < o0 || o1 > in.nvert) return -1;
  return o1 - o0;
}

// What one turn is, checked: ST_OK, or the status it ends with before any candidate is planned.  Uniform.
// max_steer is held to (0, 1.5) as in ct::run_problem, but not to its ct::MAX_TURN_RADIUS bound: a steering limit
// that small is planned here, and its candidates end as the planner has them (C_OVERFLOW).
struct TurnInfo {
  int status, type, ns, ne, ncand, naux, aux0, aux1;   // aux0 / aux1: the implements present, in order
  ct::Spec sp;
};

HTP_HD inline void turn_info(const htp_classic_sample_in& in, int64_t b, TurnInfo& t) {
  const double* p = in.params + b * HTP_CT_NPARAM;
  const int32_t* d = in.desc + HTP_SMP_NDESC * b;
  t.status = ST_BAD_INPUT;
  t.ns = in.n_start[b];
  t.ne = in.n_end[b];
  t.ncand = 0;
  t.naux = 0;
  t.type = -1;
  bool fin = true;
  for (int j = 0; j < HTP_CT_NPARAM; ++j) fin = fin && finite_(p[j]);
  if (!fin) return;
  t.type = (int)p[HTP_CT_P_TYPE];
  ct::Spec& sp = t.sp;
  sp.type = t.type;
  sp.side = (int)p[HTP_CT_P_SIDE];
  for (int j = 0; j < 3; ++j) {
    sp.start[j] = p[HTP_CT_P_SX + j];
    sp.end[j] = p[HTP_CT_P_EX + j];
  }
  sp.wb = p[HTP_CT_P_WB];
  sp.max_steer = p[HTP_CT_P_MAXSTEER];
  sp.radius = p[HTP_CT_P_RADIUS];
  sp.step = p[HTP_CT_P_STEP];
  if (t.type != T_DUBINS && t.type != T_REEDS_SHEPP && t.type != T_CIRCLE_BACK) return;
  if (sp.side != ct::NEAR_SIDE && sp.side != ct::FAR_SIDE) return;
  if (!(sp.wb > 0.0) || !(sp.step > 0.0) || !(sp.radius > 0.0) || !(sp.max_steer > 0.0) || !(sp.max_steer < 1.5)) return;
  if (t.ns < 1 || t.ns > in.cap_s || t.ne < 1 || t.ne > in.cap_e) return;
  if (t.type == T_CIRCLE_BACK && t.ne != 1) return;
  // polygons: 4-vertex body and implements, blockers and field ring of 3 or more, all within the Scene
  if (poly_len(in, d[HTP_SMP_D_BODY]) != NCORNER) return;
  t.aux0 = t.aux1 = -1;
  if (d[HTP_SMP_D_AUX0] != -1) {
    if (poly_len(in, d[HTP_SMP_D_AUX0]) != NCORNER) return;
    t.aux0 = d[HTP_SMP_D_AUX0];
    t.naux = 1;
  }
  if (d[HTP_SMP_D_AUX1] != -1) {
    if (poly_len(in, d[HTP_SMP_D_AUX1]) != NCORNER) return;
    if (t.naux == 0) t.aux0 = d[HTP_SMP_D_AUX1];
    else t.aux1 = d[HTP_SMP_D_AUX1];
    ++t.naux;
  }
  const int b0 = d[HTP_SMP_D_BLK0], b1 = d[HTP_SMP_D_BLK1];
  if (b0 < 0 || b1 < b0 || b1 > in.npoly || b1 - b0 > MAXPOLY - 4) return;
  const int nf = poly_len(in, d[HTP_SMP_D_FIELD]);
  if (nf < 3) return;
  int nv = NCORNER * (1 + t.naux) + nf;
  for (int q = b0; q < b1; ++q) {
    const int m = poly_len(in, q);
    if (m < 3) return;
    nv += m;
    if (nv > MAXVERT) return;
  }
  if (nv > MAXVERT) return;
  if ((int64_t)t.ns * t.ne > in.cap_cand) { t.status = ST_OVERFLOW; return; }
  t.ncand = t.ns * t.ne;
  t.status = ST_OK;
}

// The polygons of a checked turn into the Scene (lanes over vertices; lane 0 writes the table).
template <class C>
HTP_HD inline void load_scene(C& c, const htp_classic_sample_in& in, int64_t b, const TurnInfo& t, Scene& S) {
  const int32_t* d = in.desc + HTP_SMP_NDESC * b;
  const int nblk = d[HTP_SMP_D_BLK1] - d[HTP_SMP_D_BLK0];
  const int npoly = 1 + t.naux + nblk + 1;
  int o = 0;
  for (int q = 0; q < npoly; ++q) {
    int id;
    if (q == 0) id = d[HTP_SMP_D_BODY];
    else if (q <= t.naux) id = q == 1 ? t.aux0 : t.aux1;
    else if (q < 1 + t.naux + nblk) id = d[HTP_SMP_D_BLK0] + (q - 1 - t.naux);
    else id = d[HTP_SMP_D_FIELD];
    const int s0 = in.poly_off[id], m = in.poly_off[id + 1] - s0;
    for (int k = c.lane; k < 2 * m; k += C::width) S.vert[2 * o + k] = in.vertices[2 * (int64_t)s0 + k];
    if (c.lane == 0) S.off[q] = o;
    o += m;
  }
  if (c.lane == 0) {
    S.off[npoly] = o;
    S.naux = t.naux;
    S.blk0 = 1 + t.naux;
    S.blk1 = 1 + t.naux + nblk;
    S.field = npoly - 1;
  }
  c.sync();
}

// Which of the two device kernels plans turn b: the words kernel takes the turns whose type parameter is exactly
// Reeds-Shepp, the rows kernel every other turn (the malformed ones included: their slots end C_UNUSED).
HTP_HD inline bool is_words_turn(const htp_classic_sample_in& in, int64_t b) {
  return in.params[b * HTP_CT_NPARAM + HTP_CT_P_TYPE] == (double)T_REEDS_SHEPP;
}

// Candidate k of turn b (t, S already those of turn b) -> its table slots.
template <int MASK, class C>
HTP_HD inline void run_item(C& c, const htp_classic_sample_in& in, double* cand_score, int32_t* cand_status, int64_t b,
                            int k, const TurnInfo& t, const Scene& S, double* ws, rs::Path* paths) {
  int st = C_UNUSED;
  double score = -inf();
  if (t.status == ST_OK && k < t.ncand) {
    const int i = k / t.ne, j = k - i * t.ne;
    const double sx = in.start_x[b * in.cap_s + i], ex = in.end_x[b * in.cap_e + j];
    if (!finite_(sx) || !finite_(ex)) {
      st = C_BAD_INPUT;
    } else {
      ct::Spec sp = t.sp;
      sp.start[0] = sx;
      sp.end[0] = ex;
      st = run_candidate<MASK>(c, sp, S, ws, in.cap_samples, paths, score);
    }
  }
  if (c.lane == 0) {
    cand_score[b * in.cap_cand + k] = score;
    cand_status[b * in.cap_cand + k] = st;
  }
}

// The winner of turn b from its table slots: (score, index) by max with the lowest index on ties, from two
// order-independent reductions (a maximum of doubles without NaN, then a minimum of indices).
template <class C>
HTP_HD inline void run_winner(C& c, const htp_classic_sample_in& in, const htp_classic_sample_result& out,
                              const double* cand_score, const int32_t* cand_status, int64_t b) {
  TurnInfo t;
  turn_info(in, b, t);
  const double* sc = cand_score + b * in.cap_cand;
  const int32_t* cs = cand_status + b * in.cap_cand;
  int nfeas = 0, novf = 0;
  double best = -inf();
  const double none = 4.0e9;
  double first = none;   // lowest feasible index of this lane (indices are exact in a double)
  for (int k = c.lane; k < t.ncand; k += C::width) {
    if (cs[k] == C_OVERFLOW) novf = 1;
    if (cs[k] != C_FEASIBLE) continue;
    ++nfeas;
    if (first == none) first = (double)k;
    if (sc[k] > best) best = sc[k];
  }
  nfeas = c.isum(nfeas);
  novf = c.isum(novf);
  int win = -1;
  if (nfeas > 0) {
    if (t.type == T_CIRCLE_BACK) {
      win = (int)c.minv(first);
    } else {
      best = c.maxv(best);
      double at = none;
      for (int k = c.lane; k < t.ncand; k += C::width)
        if (cs[k] == C_FEASIBLE && sc[k] == best) { at = (double)k; break; }
      win = (int)c.minv(at);
    }
  }
  if (c.lane != 0) return;
  int status = t.status;
  if (status == ST_OK) status = novf ? ST_OVERFLOW : (nfeas > 0 ? ST_OK : ST_NONE_FEASIBLE);
  int rep = win;   // the candidate whose poses are reported
  if (rep < 0 && t.status == ST_OK && t.type == T_CIRCLE_BACK) rep = t.ncand - 1;
  double* po = out.poses + b * HTP_SMP_NPOSE;
  const double nan = inf() - inf();
  for (int j = 0; j < HTP_SMP_NPOSE; ++j) po[j] = nan;
  out.winner[2 * b] = -1;
  out.winner[2 * b + 1] = -1;
  if (rep >= 0) {
    const int i = rep / t.ne, j = rep - i * t.ne;
    const double sx = in.start_x[b * in.cap_s + i], ex = in.end_x[b * in.cap_e + j];
    po[0] = sx; po[1] = t.sp.start[1]; po[2] = t.sp.start[2];
    po[3] = ex; po[4] = t.sp.end[1]; po[5] = t.sp.end[2];
    po[6] = fabs(sx - t.sp.start[0]);
    po[7] = fabs(ex - t.sp.end[0]);
    out.winner[2 * b] = i;
    out.winner[2 * b + 1] = j;
  }
  out.status[b] = status;
  out.score[b] = win >= 0 ? sc[win] : -inf();
  out.n_feasible[b] = nfeas;
}

}  // namespace smp
}  // namespace htp
