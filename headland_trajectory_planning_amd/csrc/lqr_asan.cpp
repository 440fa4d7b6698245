// TEST-ONLY stand-alone program: the host build of the time-varying LQR (lqr_hostsim.cpp) over the shapes of the
// tests, with exactly-sized heap buffers and the x rows one double off 16-byte alignment, meant to be built with
// -fsanitize=address,undefined -fno-sanitize-recover=all: any access beyond the x rows, the parameters, the outputs
// or the staging areas that stand for the kernel's LDS aborts it.  Exits 0 when every run returned what it must.
#include <cstdio>

#include "lqr_hostsim.cpp"

namespace {

int run(int N, int topt, int batch, int M, int K, int fault) {
  int32_t eo[MAXM], eb[MAXK];
  for (int m = 0; m < M; ++m) eo[m] = 3 + (m % 5);
  for (int k = 0; k < K; ++k) eb[k] = 4;
  Dims D;
  make_dims(D, N, M, K, topt, eo, eb);
  const double dT = 0.1;
  // one double of padding in front: the rows start 8 bytes off a 16-byte boundary
  std::vector<double> xbuf((size_t)batch * D.n + 2, __builtin_nan("")), par((size_t)batch * NPARAM, 0.0);
  double* x = xbuf.data() + ((((uintptr_t)xbuf.data() >> 3) & 1u) ? 0 : 1);
  if ((((uintptr_t)x >> 3) & 1u) != 1u) return 1;
  for (int p = 0; p < batch; ++p) {
    double* r = x + (size_t)p * D.n;
    for (int i = 0; i < N; ++i) {      // a gentle left arc at 0.8 m/s (reverse for odd problems)
      const double t = dT * i, v = (p & 1) ? -0.8 : 0.8, w = 0.1;
      r[5 * i] = v / w * std::sin(w * t); r[5 * i + 1] = v / w * (1.0 - std::cos(w * t)); r[5 * i + 2] = v;
      r[5 * i + 3] = w * t; r[5 * i + 4] = std::atan(1.9 * w / v);
    }
    for (int i = 0; i < N - 1; ++i) { r[D.oU + 2 * i] = 0.01 * ((i % 5) - 2); r[D.oU + 2 * i + 1] = 0.005 * ((i % 3) - 1); }
    if (topt) for (int i = 0; i < N - 1; ++i) r[D.oTAU + i] = 0.6 + 0.4 * ((i * 7 + p) % 10) / 10.0;
    double* P = par.data() + (size_t)p * NPARAM;
    P[P_DT] = dT; P[P_WHEELBASE] = 1.9; P[P_MAXSTEER] = 0.6; P[P_MAXV] = 2.0; P[P_MAXACC] = 1.0; P[P_MAXSR] = 0.8;
  }
  if (fault && batch >= 3) {
    x[(size_t)1 * D.n + 5 * (N / 2) + 1] = __builtin_nan("");
    if (topt) x[(size_t)2 * D.n + D.oTAU] = 0.0; else par[(size_t)2 * NPARAM + P_DT] = -dT;
  }
  htp_obca_batch in{};
  in.batch = batch; in.N = N; in.M = M; in.K = K; in.time_opt = topt;
  in.obs_edges = eo; in.body_edges = eb; in.params = par.data();
  const size_t B = (size_t)batch, n = (size_t)N;
  std::vector<double> gains(B * (n - 1) * lqr::NGAIN), tube(B * n * lqr::NTUBE), met(B * lqr::NMET);
  std::vector<double> ctg(B * n * lqr::NCTG), lin(B * (n - 1) * lqr::NLIN);
  std::vector<int32_t> worst(B * 2, -7), flags(B, -1);
  htp_obca_lqr_opts o{25.0, 100.0, 25.0, 100.0, 25.0, 10.0, 1.0, 1.0, 0.05, 0.05, 0.0, 0.02, 0.0,
                      1e-4, 1e-4, 0.0, 1e-4, 0.0, 2.0};
  htp_obca_lqr_result out{gains.data(), tube.data(), met.data(), worst.data(), flags.data(), ctg.data(), lin.data()};
  char err[128];
  if (htp_hostsim_obca_lqr(&in, x, &o, &out, err, 128) != 0) { std::printf("error: %s\n", err); return 1; }
  for (int p = 0; p < batch; ++p) {
    const int f = flags[p];
    if (f < 0) return 1;
    const bool rejected = fault && batch >= 3 && (p == 1 || p == 2);
    if (rejected != ((f & (HTP_LQR_NONFINITE | HTP_LQR_BAD_TIME)) != 0)) return 1;
    if (!rejected && ((f & HTP_LQR_SINGULAR) || worst[2 * p] < 0 || worst[2 * p] >= N || worst[2 * p + 1] < 0 ||
                      worst[2 * p + 1] >= N - 1 || !(met[(size_t)p * lqr::NMET + HTP_LQR_TRACE_P0] > 0.0)))
      return 1;
  }
  // the nullable outputs absent
  out.cost_to_go = nullptr; out.linearisation = nullptr;
  if (htp_hostsim_obca_lqr(&in, x, &o, &out, err, 128) != 0) { std::printf("error: %s\n", err); return 1; }
  std::printf("N %d topt %d batch %d M %d K %d: ok\n", N, topt, batch, M, K);
  return 0;
}

}  // namespace

int main() {
  int rc = 0;
  rc |= run(2, 1, 3, 1, 1, 0);                       // one stage
  rc |= run(7, 0, 3, 2, 1, 1);                       // Euler, a NaN problem and a negative dT
  rc |= run(65, 1, 5, 1, 1, 1);                      // exactly one chunk of stages, one node beyond it
  rc |= run(66, 1, 2, 6, 2, 0);                      // one stage beyond the chunk
  rc |= run(HTP_LQR_MAX_N, 1, 2, 1, 1, 0);
  rc |= run(HTP_LQR_MAX_N, 0, 2, 1, 1, 0);
  return rc;
}
