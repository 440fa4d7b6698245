// Repair of solved OBCA trajectories that lose the margin between nodes (include/htp.h, the repair section):
// the selection rule, the raised margin, the gather of a re-solve batch and the merge of its results, one
// source for the gfx950 kernels (htp_repair.hip) and the serial host build (repair_hostsim.cpp).
//
//   pack   scan:   every problem is judged (verdict): packed, given up, or left alone; the packed ones are
//                  numbered in ascending problem order (the device counts with ballots and integer prefix
//                  sums, the host build with a serial counter: the same integers).
//          gather: slot s receives a complete htp_obca_batch row of problem index[s]: traj' (rows 1..N-2 =
//                  X_i of the solve's x, rows 0 and N-1 the original init_traj rows, which are the NLP's start
//                  and end state), init_control = U, init_mu / init_lambda = the mu / lambda blocks of x, the
//                  polygon rows, params_audit = the original parameters and params = the same with the raised
//                  margin and both init flags set.
//   merge  decide:  slot s is adopted or not (adopt_rule), the per-problem state is updated.
//          scatter: an adopted slot replaces the x row, the result fields and the audit rows of its problem.
//
// The solver has no input for tau (obca_core.h set_bounds_and_x0 starts every time scale at 1, as the
// reference's optimizer.py does), so a re-solve starts at tau = 1 whatever the first solve found.
//
// All of it is copy work and integer logic; the one floating-point expression (next_margin) is evaluated left
// to right in doubles with contraction off, so device and host build agree bit for bit.
#pragma once
#include <cstdint>

#include "../../include/htp.h"
#include "htp_common.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif

namespace htp {
namespace repair {

constexpr int FLAGGED = HTP_AUDIT_COLLISION | HTP_AUDIT_MARGIN;
constexpr int UNUSABLE = HTP_AUDIT_NONFINITE | HTP_AUDIT_BAD_POLYTOPE;
constexpr int RETIRED = HTP_REPAIR_RESOLVE_FAILED | HTP_REPAIR_GAVE_UP;
enum Verdict { V_NONE = 0, V_PACK = 1, V_GIVE_UP = 2 };

struct Shape {   // launch-uniform
  int batch, N, cap;
  int64_t n_var;                     // doubles between two problems' x rows
  int oU, oMU, oLAM;                 // offsets of U, mu and lambda inside a row (X at 0)
  int nU, nMU, nLA;                  // doubles of U, mu and lambda per problem
  int nA, nb, nG, ng;                // doubles of obs_A, obs_b, body_G and body_g per problem
  double pad, max_raise;
};

struct Slots {   // htp_obca_repair_slots
  int32_t *count, *index, *adopted;
  double *traj, *obsA, *obsb, *bodyG, *bodyg, *params, *params_audit, *init_u, *init_mu, *init_la;
};

struct State {   // htp_obca_repair_state
  int32_t *state, *rounds, *extra;
  double* dmin_used;
};

struct PackView {   // device or host pointers
  const double *traj, *obsA, *obsb, *bodyG, *bodyg, *params, *x;
  const int32_t* status;
  const double* metrics;
  const int32_t* flags;
  State st;
  Slots sl;
};

struct ResultView {   // htp_obca_result
  double *x, *objective;
  int32_t *status, *iterations, *n_factor;
  double* nlp_error;
  int32_t* n_resto;   // nullable
};

struct AuditView {   // htp_obca_audit_result
  double* metrics;
  int32_t *worst, *flags;
  double* stage;      // nullable
};

struct MergeView {
  Slots sl;
  ResultView re, out;      // the re-solve (slot-major) and the adopted results (problem-major)
  AuditView re_audit, audit;
  State st;
  int32_t* tally;          // nullable [3]: slots merged, adopted, clean against the original margin
};

HTP_HD inline void make_shape(Shape& s, const htp_obca_batch& in, int cap, double pad, double max_raise) {
  Dims D;
  make_dims(D, in.N, in.M, in.K, in.time_opt, in.obs_edges, in.body_edges);
  s.batch = in.batch; s.N = in.N; s.cap = cap;
  s.n_var = D.n; s.oU = D.oU; s.oMU = D.oMU; s.oLAM = D.oLAM;
  s.nU = NC * (in.N - 1); s.nMU = in.N * D.mu_count; s.nLA = in.N * D.lam_count;
  s.nA = 2 * D.TEo; s.nb = D.TEo; s.nG = 2 * D.TEb; s.ng = D.TEb;
  s.pad = pad; s.max_raise = max_raise;
}

// the margin the adopted result of problem p was last re-solved with (the original one before any round)
HTP_HD inline double current_margin(const PackView& v, int64_t p) {
  return v.st.rounds[p] > 0 ? v.st.dmin_used[p] : v.params[p * NPARAM + P_DMIN];
}

// dmin_cur + (dmin_orig - clearance_cur) + pad, left to right
HTP_HD inline double next_margin(const PackView& v, const Shape& sh, int64_t p) {
  const double orig = v.params[p * NPARAM + P_DMIN];
  const double deficit = orig - v.metrics[p * HTP_AUDIT_NMETRIC + HTP_AUDIT_CLEARANCE];
  double m = current_margin(v, p) + deficit;
  m = m + sh.pad;
  return m;
}

HTP_HD inline int verdict(const PackView& v, const Shape& sh, int64_t p) {
  const int st = v.status[p], fl = v.flags[p];
  if (st != HTP_STATUS_SUCCESS && st != HTP_STATUS_ACCEPTABLE) return V_NONE;
  if (!(fl & FLAGGED) || (fl & UNUSABLE) || (v.st.state[p] & RETIRED)) return V_NONE;
  // a margin that is not <= the limit (NaN included) is not tried
  return next_margin(v, sh, p) <= v.params[p * NPARAM + P_DMIN] + sh.max_raise ? V_PACK : V_GIVE_UP;
}

HTP_HD inline void mark(const PackView& v, int64_t p, int vd) {
  if (vd != V_NONE) v.st.state[p] |= HTP_REPAIR_CANDIDATE | (vd == V_GIVE_UP ? HTP_REPAIR_GAVE_UP : 0);
}

// Slot s of the re-solve batch.  c: a group of c.nth threads, this one c.tid; c.copy(dst, src, n) moves one
// contiguous run with the whole group.
template <class W>
HTP_HD inline void gather_slot(const W& c, const Shape& sh, const PackView& v, int64_t s) {
  const int64_t p = v.sl.index[s];
  const int N = sh.N, nt = NS * N;
  const double* x = v.x + p * sh.n_var;
  double* tr = v.sl.traj + s * nt;
  c.copy(tr, v.traj + p * nt, NS);
  if (N > 2) c.copy(tr + NS, x + NS, NS * (N - 2));
  c.copy(tr + nt - NS, v.traj + p * nt + nt - NS, NS);
  c.copy(v.sl.init_u + s * sh.nU, x + sh.oU, sh.nU);
  c.copy(v.sl.init_mu + s * (int64_t)sh.nMU, x + sh.oMU, sh.nMU);
  c.copy(v.sl.init_la + s * (int64_t)sh.nLA, x + sh.oLAM, sh.nLA);
  c.copy(v.sl.obsA + s * sh.nA, v.obsA + p * sh.nA, sh.nA);
  c.copy(v.sl.obsb + s * sh.nb, v.obsb + p * sh.nb, sh.nb);
  c.copy(v.sl.bodyG + s * sh.nG, v.bodyG + p * sh.nG, sh.nG);
  c.copy(v.sl.bodyg + s * sh.ng, v.bodyg + p * sh.ng, sh.ng);
  c.copy(v.sl.params_audit + s * NPARAM, v.params + p * NPARAM, NPARAM);
  // params: one entry per thread, so the three rewritten entries need no ordering against a group copy
  for (int k = c.tid; k < NPARAM; k += c.nth) {
    double val = v.params[p * NPARAM + k];
    if (k == P_DMIN) val = next_margin(v, sh, p);
    if (k == P_HAS_INIT_CONTROL || k == P_HAS_INIT_DUAL) val = 1.0;
    v.sl.params[s * NPARAM + k] = val;
  }
}

HTP_HD inline bool adopt_rule(const MergeView& v, int64_t s, int64_t p) {
  const int st = v.re.status[s], fl = v.re_audit.flags[s];
  if (st != HTP_STATUS_SUCCESS && st != HTP_STATUS_ACCEPTABLE) return false;
  if (fl & UNUSABLE) return false;
  if ((fl & ~FLAGGED) & ~v.audit.flags[p]) return false;
  return v.re_audit.metrics[s * HTP_AUDIT_NMETRIC + HTP_AUDIT_CLEARANCE] >
         v.audit.metrics[p * HTP_AUDIT_NMETRIC + HTP_AUDIT_CLEARANCE];
}

// One thread per slot: the decision and the state of its problem.  c.add is an integer atomic on the device.
template <class W>
HTP_HD inline void decide_slot(const W& c, const MergeView& v, int64_t s) {
  const int64_t p = v.sl.index[s];
  const int st = v.re.status[s];
  const bool ok = st == HTP_STATUS_SUCCESS || st == HTP_STATUS_ACCEPTABLE;
  const bool adopt = adopt_rule(v, s, p);
  const bool clean = adopt && !(v.re_audit.flags[s] & FLAGGED);
  v.sl.adopted[s] = adopt ? 1 : 0;
  v.st.dmin_used[p] = v.sl.params[s * NPARAM + P_DMIN];
  v.st.rounds[p] += 1;
  v.st.extra[p] += v.re.iterations[s];
  v.st.state[p] |= HTP_REPAIR_CANDIDATE | (adopt ? HTP_REPAIR_IMPROVED : 0) | (clean ? HTP_REPAIR_REPAIRED : 0) |
                   (ok ? 0 : HTP_REPAIR_RESOLVE_FAILED);
  if (v.tally) {
    c.add(v.tally + 0, 1);
    if (adopt) c.add(v.tally + 1, 1);
    if (clean) c.add(v.tally + 2, 1);
  }
}

template <class W>
HTP_HD inline void scatter_slot(const W& c, const Shape& sh, const MergeView& v, int64_t s) {
  if (!v.sl.adopted[s]) return;
  const int64_t p = v.sl.index[s];
  c.copy(v.out.x + p * sh.n_var, v.re.x + s * sh.n_var, (int)sh.n_var);
  c.copy(v.audit.metrics + p * HTP_AUDIT_NMETRIC, v.re_audit.metrics + s * HTP_AUDIT_NMETRIC, HTP_AUDIT_NMETRIC);
  if (v.audit.stage && v.re_audit.stage) c.copy(v.audit.stage + p * sh.N, v.re_audit.stage + s * sh.N, sh.N);
  if (c.tid == 0) {
    v.out.objective[p] = v.re.objective[s];
    v.out.status[p] = v.re.status[s];
    v.out.iterations[p] = v.re.iterations[s];
    v.out.n_factor[p] = v.re.n_factor[s];
    v.out.nlp_error[p] = v.re.nlp_error[s];
    if (v.out.n_resto && v.re.n_resto) v.out.n_resto[p] = v.re.n_resto[s];
    for (int k = 0; k < 4; ++k) v.audit.worst[p * 4 + k] = v.re_audit.worst[s * 4 + k];
    v.audit.flags[p] = v.re_audit.flags[s];
  }
}

// The serial lane of the test-only host build; the gfx950 groups are in htp_repair.hip.
struct HostLane {
  int tid = 0, nth = 1;
  void copy(double* dst, const double* src, int n) const {
    for (int q = 0; q < n; ++q) dst[q] = src[q];
  }
  void add(int32_t* a, int v) const { *a += v; }
};

// Serial pack and merge over views of host arrays (the host build; also the meaning of the device kernels).
inline void pack_serial(const Shape& sh, const PackView& v) {
  HostLane c;
  int n = 0;
  for (int64_t p = 0; p < sh.batch; ++p) {
    const int vd = verdict(v, sh, p);
    mark(v, p, vd);
    if (vd != V_PACK) continue;
    if (n < sh.cap) v.sl.index[n] = (int32_t)p;
    ++n;
  }
  *v.sl.count = n;
  for (int s = 0; s < (n < sh.cap ? n : sh.cap); ++s) gather_slot(c, sh, v, s);
}

inline void merge_serial(const Shape& sh, const MergeView& v) {
  HostLane c;
  const int n = *v.sl.count < sh.cap ? *v.sl.count : sh.cap;
  for (int s = 0; s < n; ++s) decide_slot(c, v, s);
  for (int s = 0; s < n; ++s) scatter_slot(c, sh, v, s);
}

}  // namespace repair
}  // namespace htp

#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC pop_options
#endif
