// TEST-ONLY host build of the solver core (serial single-lane context) with the path counters of
// HTP_TEST_STATS: what a test input exercises, not what it returns.  stats[4 p ..] of problem p = the most
// pivoted local blocks met in one factor sweep, the factor sweeps with at least one, the second-order
// corrections taken, the restoration phases entered.  Built by tests/_stats_host.py; the product never loads it.
#include <cstdlib>
#include <vector>

#define HTP_HD
#define HTP_TEST_STATS 1
#include "wave_ctx.h"
#include "obca_batch.h"

using namespace htp;

extern "C" int htp_hostsim_obca_stats(const htp_obca_batch* in, htp_obca_result* out, int32_t* stats) {
  const char* e = nullptr;
  if (check_shape(in, &e)) return -1;
  Options o = default_options();
  o.wall_rate = 1e9;
  Dims D;
  make_dims(D, in->N, in->M, in->K, in->time_opt, in->obs_edges, in->body_edges);
  Layout L = make_layout(D);
  std::vector<double> ws((size_t)L.total);
  std::vector<double> lds(4 * NBMAX * NBMAX + 8 + 128);
  std::vector<int> ilds(2 * NBMAX);
  BatchView b{in->traj, in->obs_A, in->obs_b, in->body_G, in->body_g, in->params,
              in->init_control, in->init_mu, in->init_lambda};
  for (int p = 0; p < in->batch; ++p) {
    HostLane c;
    c.lds = lds.data();
    c.ildsp = ilds.data();
    ProblemIn pin = problem_view(b, D, p);
    ObcaSolver<HostLane, MAXE, MAXE> S(c, D, L, o, pin, ws.data());
    Result r{};
    S.run(r);
    for (int q = 0; q < D.n; ++q) out->x[(size_t)p * D.n + q] = ws[L.x + q];
    if (out->objective) out->objective[p] = r.objective;
    if (out->status) out->status[p] = r.status;
    if (out->iterations) out->iterations[p] = r.iters;
    if (out->n_factor) out->n_factor[p] = r.n_factor;
    if (out->nlp_error) out->nlp_error[p] = r.nlp_error;
    if (out->n_resto) out->n_resto[p] = r.n_resto;
    stats[4 * p] = S.stat_piv_max;
    stats[4 * p + 1] = S.stat_piv_sweeps;
    stats[4 * p + 2] = S.stat_soc;
    stats[4 * p + 3] = r.n_resto;
  }
  return 0;
}
