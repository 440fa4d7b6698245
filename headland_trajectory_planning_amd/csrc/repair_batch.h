// The repair section's C structs -> the repair core's launch shape and pointer views, with the argument checks
// of the C ABI; shared by the gfx950 library (htp_repair.hip) and the test-only host build (repair_hostsim.cpp).
#pragma once
#include "../../include/htp.h"
#include "repair_core.h"

namespace htp {
namespace repair {

inline int check_shape(const htp_obca_batch* in, const char** err) {
  if (!in) { *err = "[repair] null argument"; return -1; }
  if (in->batch < 0) { *err = "[repair] batch must be >= 0"; return -1; }
  if (in->N < 2) { *err = "[repair] N must be >= 2"; return -1; }
  if (in->N > HTP_AUDIT_MAX_N) { *err = "[repair] N must be <= HTP_AUDIT_MAX_N (480)"; return -1; }
  if (in->M < 1 || in->M > MAXM) { *err = "[repair] M must be in [1, 16]"; return -1; }
  if (in->K < 1 || in->K > MAXK) { *err = "[repair] K must be in [1, 4]"; return -1; }
  if (!in->obs_edges || !in->body_edges) { *err = "[repair] null argument (edge counts)"; return -1; }
  for (int m = 0; m < in->M; ++m)
    if (in->obs_edges[m] < 3 || in->obs_edges[m] > MAXE) { *err = "[repair] obstacle edges must be in [3, 8]"; return -1; }
  for (int k = 0; k < in->K; ++k)
    if (in->body_edges[k] < 3 || in->body_edges[k] > MAXE) { *err = "[repair] body edges must be in [3, 8]"; return -1; }
  return 0;
}

inline int check_raise(const htp_obca_repair_opts* o, const char** err) {
  if (!o) { *err = "[repair] null argument"; return -1; }
  if (!(o->pad >= 0.0) || !(o->pad - o->pad == 0.0)) { *err = "[repair] pad must be finite and >= 0"; return -1; }
  if (!(o->max_raise > 0.0) || !(o->max_raise - o->max_raise == 0.0)) { *err = "[repair] max_raise must be finite and > 0"; return -1; }
  return 0;
}

inline bool inputs_ok(const htp_obca_batch* in) {
  return in->traj && in->obs_A && in->obs_b && in->body_G && in->body_g && in->params;
}
inline bool state_ok(const htp_obca_repair_state* s) {
  return s->state && s->rounds_used && s->extra_iterations && s->dmin_used;
}
inline bool result_ok(const htp_obca_result* r) {
  return r->x && r->objective && r->status && r->iterations && r->n_factor && r->nlp_error;
}
inline bool audit_ok(const htp_obca_audit_result* a) { return a->metrics && a->worst && a->flags; }
inline bool slots_ok(const htp_obca_repair_slots* s) {
  return s->count && s->index && s->adopted && s->traj && s->obs_A && s->obs_b && s->body_G && s->body_g &&
         s->params && s->params_audit && s->init_control && s->init_mu && s->init_lambda;
}

// 0 = OK; -1 with *err set: nothing may be launched
inline int check_pack(const htp_obca_batch* in, const htp_obca_result* out, const htp_obca_audit_result* audit,
                      const htp_obca_repair_opts* o, const htp_obca_repair_state* st,
                      const htp_obca_repair_slots* sl, const char** err) {
  if (!in || !out || !audit || !o || !st || !sl) { *err = "[repair] null argument"; return -1; }
  if (check_shape(in, err) || check_raise(o, err)) return -1;
  if (sl->cap < 1) { *err = "[repair] cap must be >= 1"; return -1; }
  if (in->batch == 0) return 0;
  if (!inputs_ok(in)) { *err = "[repair] null argument (input array)"; return -1; }
  if (!out->x || !out->status) { *err = "[repair] null argument (x, status)"; return -1; }
  if (!audit->metrics || !audit->flags) { *err = "[repair] null argument (audit array)"; return -1; }
  if (!state_ok(st)) { *err = "[repair] null argument (state array)"; return -1; }
  if (!slots_ok(sl)) { *err = "[repair] null argument (slot array)"; return -1; }
  return 0;
}

inline int check_merge(const htp_obca_batch* in, const htp_obca_repair_slots* sl, const htp_obca_result* re,
                       const htp_obca_audit_result* re_audit, const htp_obca_result* out,
                       const htp_obca_audit_result* audit, const htp_obca_repair_state* st, const char** err) {
  if (!in || !sl || !re || !re_audit || !out || !audit || !st) { *err = "[repair] null argument"; return -1; }
  if (check_shape(in, err)) return -1;
  if (sl->cap < 1) { *err = "[repair] cap must be >= 1"; return -1; }
  if (in->batch == 0) return 0;
  if (!slots_ok(sl)) { *err = "[repair] null argument (slot array)"; return -1; }
  if (!result_ok(re) || !result_ok(out)) { *err = "[repair] null argument (result array)"; return -1; }
  if (!audit_ok(re_audit) || !audit_ok(audit)) { *err = "[repair] null argument (audit array)"; return -1; }
  if (!state_ok(st)) { *err = "[repair] null argument (state array)"; return -1; }
  return 0;
}

inline int check_loop(const htp_obca_batch* in, const htp_obca_result* out, const htp_obca_repair_opts* o,
                      const htp_obca_audit_result* audit, const htp_obca_repair_report* rep, const char** err) {
  if (!in || !out || !o || !audit || !rep) { *err = "[repair] null argument"; return -1; }
  if (check_shape(in, err) || check_raise(o, err)) return -1;
  if (o->rounds < 1 || o->rounds > HTP_REPAIR_MAX_ROUNDS) { *err = "[repair] rounds must be in [1, HTP_REPAIR_MAX_ROUNDS (8)]"; return -1; }
  const htp_obca_audit_opts& a = o->audit;
  if (a.substeps < 1 || a.substeps > HTP_AUDIT_MAX_SUBSTEPS) { *err = "[repair] audit substeps must be in [1, HTP_AUDIT_MAX_SUBSTEPS (16)]"; return -1; }
  if (!(a.margin_tol >= 0.0) || !(a.dyn_tol >= 0.0) || !(a.bound_tol >= 0.0) || !(a.term_tol >= 0.0)) {
    *err = "[repair] audit tolerances must be >= 0";
    return -1;
  }
  if (in->batch == 0) return 0;
  if (!inputs_ok(in)) { *err = "[repair] null argument (input array)"; return -1; }
  if (!result_ok(out)) { *err = "[repair] null argument (result array)"; return -1; }
  if (!audit_ok(audit)) { *err = "[repair] null argument (audit array)"; return -1; }
  if (!state_ok(&rep->state) || !rep->round_counts) { *err = "[repair] null argument (report array)"; return -1; }
  return 0;
}

inline State state_view(const htp_obca_repair_state& s) {
  return State{s.state, s.rounds_used, s.extra_iterations, s.dmin_used};
}
inline Slots slots_view(const htp_obca_repair_slots& s) {
  return Slots{s.count, s.index, s.adopted, s.traj, s.obs_A, s.obs_b, s.body_G, s.body_g,
               s.params, s.params_audit, s.init_control, s.init_mu, s.init_lambda};
}
inline ResultView result_view(const htp_obca_result& r) {
  return ResultView{r.x, r.objective, r.status, r.iterations, r.n_factor, r.nlp_error, r.n_resto};
}
inline AuditView audit_view(const htp_obca_audit_result& a) {
  return AuditView{a.metrics, a.worst, a.flags, a.stage_clearance};
}
inline PackView pack_view(const htp_obca_batch& in, const htp_obca_result& out, const htp_obca_audit_result& audit,
                          const htp_obca_repair_state& st, const htp_obca_repair_slots& sl) {
  return PackView{in.traj, in.obs_A, in.obs_b, in.body_G, in.body_g, in.params, out.x, out.status,
                  audit.metrics, audit.flags, state_view(st), slots_view(sl)};
}
inline MergeView merge_view(const htp_obca_repair_slots& sl, const htp_obca_result& re,
                            const htp_obca_audit_result& re_audit, const htp_obca_result& out,
                            const htp_obca_audit_result& audit, const htp_obca_repair_state& st, int32_t* tally) {
  return MergeView{slots_view(sl), result_view(re), result_view(out), audit_view(re_audit), audit_view(audit),
                   state_view(st), tally};
}

// the packed slots as the batch a solve or an audit takes (params_audit for the audit)
inline htp_obca_batch slots_batch(const htp_obca_batch& in, const htp_obca_repair_slots& s, int32_t count, bool audit) {
  htp_obca_batch b = in;
  b.batch = count;
  b.traj = s.traj; b.obs_A = s.obs_A; b.obs_b = s.obs_b; b.body_G = s.body_G; b.body_g = s.body_g;
  b.params = audit ? s.params_audit : s.params;
  b.init_control = s.init_control; b.init_mu = s.init_mu; b.init_lambda = s.init_lambda;
  return b;
}

}  // namespace repair
}  // namespace htp
