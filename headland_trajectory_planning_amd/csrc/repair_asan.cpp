// TEST-ONLY stand-alone program: pack and merge of the host build of the repair steps (repair_hostsim.cpp) on
// crafted batches with exactly-sized heap buffers, meant to be built with
// -fsanitize=address,undefined -fno-sanitize-recover=all: any access beyond an input row, a slot or a result row
// aborts it.  Exits 0 when every run returned what it must.
#include <cstdio>
#include <vector>

#include "repair_hostsim.cpp"

namespace {

// kind: 0 no candidate, 1 all candidates, 2 candidates at 0 and B-1 only, 3 mixed (a failed status, a
// NONFINITE and a BAD_POLYTOPE problem and one at the max_raise limit among candidates)
int run(int N, int batch, int kind, int cap) {
  const int32_t eo[2] = {4, 3}, eb[2] = {4, 5};
  const int M = 2, K = 2;
  Dims D;
  make_dims(D, N, M, K, 1, eo, eb);
  const size_t B = (size_t)batch, C = (size_t)cap, nv = (size_t)D.n;
  const size_t nt = 5 * (size_t)N, nU = 2 * (size_t)(N - 1), nMU = (size_t)N * D.mu_count, nLA = (size_t)N * D.lam_count;
  const size_t nA = 2 * (size_t)D.TEo, nb = (size_t)D.TEo, nG = 2 * (size_t)D.TEb, ng = (size_t)D.TEb;
  auto fill = [](std::vector<double>& v, double a) { for (size_t q = 0; q < v.size(); ++q) v[q] = a + 1e-3 * (double)q; };
  std::vector<double> traj(B * nt), A(B * nA), b(B * nb), G(B * nG), g(B * ng), par(B * NPARAM), x(B * nv);
  fill(traj, 1.0); fill(A, 2.0); fill(b, 3.0); fill(G, 4.0); fill(g, 5.0); fill(par, 6.0); fill(x, 7.0);
  std::vector<double> obj(B, 1.0), nerr(B, 1e-9), met(B * HTP_AUDIT_NMETRIC, 0.5), stc(B * (size_t)N, 0.5);
  std::vector<int32_t> status(B, 0), iters(B, 50), nfac(B, 60), nresto(B, 0), worst(B * 4, 0), flags(B, 0);
  std::vector<int32_t> state(B, 0), rounds(B, 0), extra(B, 0);
  std::vector<double> dused(B, 0.0);
  int want = 0, gave_up = 0;
  for (int p = 0; p < batch; ++p) {
    par[(size_t)p * NPARAM + P_DMIN] = 0.1;
    bool cand = kind == 1 || (kind == 2 && (p == 0 || p == batch - 1)) || (kind == 3 && p % 2 == 0);
    double clr = cand ? 0.04 + 0.001 * (p % 7) : 0.2;
    if (cand) flags[p] = HTP_AUDIT_MARGIN;
    if (kind == 3 && cand) {
      const int sub = (p / 2) % 5;
      if (sub == 1) { status[p] = HTP_STATUS_MAX_ITER; cand = false; }
      if (sub == 2) { flags[p] |= HTP_AUDIT_NONFINITE; cand = false; }
      if (sub == 3) { flags[p] |= HTP_AUDIT_BAD_POLYTOPE; cand = false; }
      if (sub == 4) { clr = -0.6; flags[p] |= HTP_AUDIT_COLLISION; cand = false; ++gave_up; }
    }
    met[(size_t)p * HTP_AUDIT_NMETRIC + HTP_AUDIT_CLEARANCE] = clr;
    want += cand;
  }
  htp_obca_batch in{};
  in.batch = batch; in.N = N; in.M = M; in.K = K; in.time_opt = 1; in.obs_edges = eo; in.body_edges = eb;
  in.traj = traj.data(); in.obs_A = A.data(); in.obs_b = b.data(); in.body_G = G.data(); in.body_g = g.data();
  in.params = par.data();
  htp_obca_result out{x.data(), obj.data(), status.data(), iters.data(), nfac.data(), nerr.data(), nresto.data()};
  htp_obca_audit_result aud{met.data(), worst.data(), flags.data(), stc.data()};
  htp_obca_repair_state st{state.data(), rounds.data(), extra.data(), dused.data()};
  std::vector<int32_t> count(1, -1), index(C, -1), adopted(C, -1);
  std::vector<double> s_traj(C * nt), s_A(C * nA), s_b(C * nb), s_G(C * nG), s_g(C * ng), s_p(C * NPARAM),
      s_pa(C * NPARAM), s_u(C * nU), s_mu(C * nMU), s_la(C * nLA);
  htp_obca_repair_slots sl{cap, count.data(), index.data(), adopted.data(), s_traj.data(), s_A.data(), s_b.data(),
                           s_G.data(), s_g.data(), s_p.data(), s_pa.data(), s_u.data(), s_mu.data(), s_la.data()};
  htp_obca_repair_opts o{};
  o.rounds = 3; o.pad = 0.01; o.max_raise = 0.5;
  char err[128];
  if (htp_hostsim_repair_pack(&in, &out, &aud, &o, &st, &sl, err, 128) != 0) { std::printf("error: %s\n", err); return 1; }
  if (count[0] != want) { std::printf("count %d, expected %d\n", count[0], want); return 1; }
  const int used = want < cap ? want : cap;
  int given = 0;
  for (int p = 0; p < batch; ++p) given += (state[p] & HTP_REPAIR_GAVE_UP) != 0;
  if (given != gave_up) return 1;
  for (int s = 0; s < used; ++s) {
    const size_t p = (size_t)index[s];
    if (s && index[s] <= index[s - 1]) return 1;
    for (int k = 0; k < 5; ++k)
      if (s_traj[s * nt + k] != traj[p * nt + k] || s_traj[s * nt + nt - 5 + k] != traj[p * nt + nt - 5 + k]) return 1;
    if (N > 2 && s_traj[s * nt + 5] != x[p * nv + 5]) return 1;
    if (s_mu[s * nMU + nMU - 1] != x[p * nv + D.oLAM - 1] || s_la[s * nLA + nLA - 1] != x[p * nv + D.oTAU - 1]) return 1;
    if (!(s_p[(size_t)s * NPARAM + P_DMIN] > 0.1) || s_pa[(size_t)s * NPARAM + P_DMIN] != 0.1) return 1;
  }
  // a made-up re-solve: even slots improve and come out clean, every third one fails
  std::vector<double> rx(C * nv), robj(C, 2.0), rerr(C, 1e-8), rmet(C * HTP_AUDIT_NMETRIC, 0.3), rstc(C * (size_t)N, 0.3);
  std::vector<int32_t> rst(C, 0), rit(C, 30), rnf(C, 33), rnr(C, 0), rworst(C * 4, 1), rfl(C, 0);
  fill(rx, 9.0);
  int want_adopt = 0;
  for (int s = 0; s < cap; ++s) {
    const bool better = s % 2 == 0, failed = s % 3 == 2;
    rmet[(size_t)s * HTP_AUDIT_NMETRIC + HTP_AUDIT_CLEARANCE] = better ? 0.3 : 0.01;
    if (!better) rfl[s] = HTP_AUDIT_MARGIN;
    if (failed) rst[s] = HTP_STATUS_INFEASIBLE;
    want_adopt += s < used && better && !failed;
  }
  htp_obca_result re{rx.data(), robj.data(), rst.data(), rit.data(), rnf.data(), rerr.data(), rnr.data()};
  htp_obca_audit_result ra{rmet.data(), rworst.data(), rfl.data(), rstc.data()};
  std::vector<int32_t> tally(3, 0);
  if (htp_hostsim_repair_merge(&in, &sl, &re, &ra, &out, &aud, &st, tally.data(), err, 128) != 0) {
    std::printf("error: %s\n", err);
    return 1;
  }
  if (tally[0] != used || tally[1] != want_adopt || tally[2] != want_adopt) return 1;
  for (int s = 0; s < used; ++s) {
    const size_t p = (size_t)index[s];
    if (rounds[p] != 1 || extra[p] != 30 || dused[p] != s_p[(size_t)s * NPARAM + P_DMIN]) return 1;
    if (adopted[s] && (x[p * nv + nv - 1] != rx[(size_t)s * nv + nv - 1] || status[p] != 0 || flags[p] != 0)) return 1;
  }
  std::printf("N %d batch %d kind %d cap %d: ok (%d packed of %d, %d adopted)\n", N, batch, kind, cap, used, want, want_adopt);
  return 0;
}

}  // namespace

int main() {
  int rc = 0;
  rc |= run(7, 9, 0, 9);       // no candidate
  rc |= run(7, 9, 1, 9);       // all candidates
  rc |= run(7, 9, 2, 9);       // candidates at problems 0 and B-1
  rc |= run(7, 23, 3, 23);     // failed status, NONFINITE, BAD_POLYTOPE, max_raise among candidates
  rc |= run(7, 23, 1, 5);      // cap < count
  rc |= run(2, 3, 1, 3);       // no interior rows
  rc |= run(80, 6, 1, 2);      // a long horizon, cap < count
  return rc;
}
