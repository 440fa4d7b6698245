// TEST-ONLY stand-alone program: the serial host build of the OBCA solver (HostLane) on the two smallest shapes
// of tests/_step_cases.py -- N 4, M 1 (every vector shorter than one sweep trip) and N 11, M 6 (66 local blocks)
// -- with exactly-sized heap buffers, meant to be built with -fsanitize=address,undefined
// -fno-sanitize-recover=all: any access beyond a workspace array, an input row or a result row aborts it.
// A half turn past a wall of boxes; exits 0 when every solve ended with a finite iterate.
#include <cmath>
#include <cstdio>
#include <vector>

#define HTP_HD
#include "wave_ctx.h"
#include "obca_batch.h"

using namespace htp;

namespace {

int run(int N, int M) {
  const int K = 1;
  std::vector<int32_t> eo((size_t)M, 4), eb((size_t)K, 4);
  const double dT = 0.4, wheelbase = 1.9, R = 3.4;
  std::vector<double> traj((size_t)N * 5), A((size_t)M * 8), b((size_t)M * 4), G(8), g(4), par(NPARAM, 0.0);
  const double pi = 3.141592653589793;
  const double ds = pi * R / (N - 1), v = ds / dT < 0.9 ? ds / dT : 0.9;
  for (int i = 0; i < N; ++i) {
    const double phi = pi * i / (N - 1);
    traj[5 * i] = -R * std::sin(phi);
    traj[5 * i + 1] = R * (1.0 - std::cos(phi));
    traj[5 * i + 2] = (i == 0 || i == N - 1) ? 0.0 : v;
    traj[5 * i + 3] = -pi - phi;
    traj[5 * i + 4] = i == 0 ? 0.0 : -std::atan(wheelbase / R);
  }
  const double rows[8] = {0.0, -1.0, 1.0, 0.0, 0.0, 1.0, -1.0, 0.0};
  for (int m = 0; m < M; ++m) {   // boxes [x0, x0 + 2] x [y0, y0 + 1] left of the turn
    const double x0 = -R - 6.0 - 3.0 * (m / 3), y0 = -4.0 + 5.0 * (m % 3);
    for (int k = 0; k < 8; ++k) A[(size_t)m * 8 + k] = rows[k];
    b[(size_t)m * 4] = -y0; b[(size_t)m * 4 + 1] = x0 + 2.0; b[(size_t)m * 4 + 2] = y0 + 1.0; b[(size_t)m * 4 + 3] = -x0;
  }
  const double Gr[8] = {0.0, -1.3513514, 1.0, 0.0, 0.0, 1.3513514, -1.8181818, 0.0}, gr[4] = {1.0, 2.85, 1.0, 1.0};
  for (int k = 0; k < 8; ++k) G[k] = Gr[k];
  for (int k = 0; k < 4; ++k) g[k] = gr[k];
  par[P_DT] = dT; par[P_Q00] = 1.0; par[P_Q11] = 1.0; par[P_R00] = 0.1; par[P_R11] = 0.1; par[P_W00] = 10.0;
  par[P_W11] = 0.1; par[P_WHEELBASE] = wheelbase; par[P_MAXSTEER] = 0.55; par[P_MAXV] = 1.0; par[P_MAXACC] = 1.0;
  par[P_MAXSR] = 0.7; par[P_DMIN] = 0.1; par[P_XLO] = -INFINITY; par[P_XHI] = INFINITY; par[P_YLO] = -INFINITY;
  par[P_YHI] = INFINITY;
  htp_obca_batch in{};
  in.batch = 1; in.N = N; in.M = M; in.K = K; in.time_opt = 1; in.obs_edges = eo.data(); in.body_edges = eb.data();
  in.traj = traj.data(); in.obs_A = A.data(); in.obs_b = b.data(); in.body_G = G.data(); in.body_g = g.data();
  in.params = par.data();
  const char* e = nullptr;
  if (check_shape(&in, &e)) { std::printf("bad shape: %s\n", e ? e : "?"); return 1; }
  Options o = default_options();
  o.wall_rate = 1e9;
  o.max_iter = 300;
  Dims D;
  make_dims(D, N, M, K, 1, eo.data(), eb.data());
  Layout L = make_layout(D);
  std::vector<double> ws((size_t)L.total);
  std::vector<double> lds(4 * NBMAX * NBMAX + 8 + 128);
  std::vector<int> ilds(2 * NBMAX);
  BatchView bv{in.traj, in.obs_A, in.obs_b, in.body_G, in.body_g, in.params, nullptr, nullptr, nullptr};
  HostLane c;
  c.lds = lds.data();
  c.ildsp = ilds.data();
  ProblemIn pin = problem_view(bv, D, 0);
  ObcaSolver<HostLane, MAXE, MAXE> S(c, D, L, o, pin, ws.data());
  Result r{};
  S.run(r);
  bool finite = std::isfinite(r.objective);
  for (int q = 0; q < D.n; ++q) finite = finite && std::isfinite(ws[(size_t)L.x + q]);
  std::printf("N %d M %d: status %d iterations %d factorizations %d restorations %d objective %.6g%s\n", N, M, r.status,
              r.iters, r.n_factor, r.n_resto, r.objective, finite ? "" : " (not finite)");
  return finite && r.status >= 0 && r.status <= ST_TINYSTEP ? 0 : 1;
}

}  // namespace

int main() {
  int rc = 0;
  rc |= run(4, 1);
  rc |= run(11, 6);
  return rc;
}
