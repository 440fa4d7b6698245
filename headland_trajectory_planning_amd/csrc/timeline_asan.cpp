// TEST-ONLY stand-alone program: the host build of the trajectory timeline (timeline_hostsim.cpp) over the
// shapes of the tests, with exactly-sized heap buffers, meant to be built with
// -fsanitize=address,undefined -fno-sanitize-recover=all: any access beyond the x rows, the outputs or the
// staging areas that stand for the kernel's LDS aborts it.  Exits 0 when every run returned what it must.
#include <cstdio>

#include "timeline_hostsim.cpp"

namespace {

int run(int N, int topt, int batch, double dt_over_dT, int cap_short, int fault) {
  const int32_t eo[2] = {4, 3}, eb[1] = {4};
  Dims D;
  make_dims(D, N, 2, 1, topt, eo, eb);
  const double dT = 0.25;
  std::vector<double> x((size_t)batch * D.n, __builtin_nan("")), par((size_t)batch * NPARAM, 0.0);
  for (int p = 0; p < batch; ++p) {
    double* r = x.data() + (size_t)p * D.n;
    for (int i = 0; i < N; ++i) {
      const double s = (double)i / N;
      r[5 * i] = 8.0 * s; r[5 * i + 1] = 3.0 * s * s; r[5 * i + 2] = (i & 1) ? -0.7 : 0.9;
      r[5 * i + 3] = 4.0 * s - 0.3 * p; r[5 * i + 4] = 0.3 - 0.5 * s;
    }
    for (int i = 0; i < N - 1; ++i) { r[D.oU + 2 * i] = 0.1 * ((i % 5) - 2); r[D.oU + 2 * i + 1] = 0.05 * ((i % 3) - 1); }
    if (topt) for (int i = 0; i < N - 1; ++i) r[D.oTAU + i] = 0.5 + 0.5 * ((i * 7 + p) % 10) / 10.0;
    par[(size_t)p * NPARAM + P_DT] = dT;
    par[(size_t)p * NPARAM + P_WHEELBASE] = 1.9;
  }
  if (fault && batch >= 3) {
    x[(size_t)1 * D.n + 5 * (N / 2) + 1] = __builtin_nan("");
    if (topt) x[(size_t)2 * D.n + D.oTAU] = 0.0; else par[(size_t)2 * NPARAM + P_DT] = -dT;
  }
  htp_obca_batch in{};
  in.batch = batch; in.N = N; in.M = 2; in.K = 1; in.time_opt = topt;
  in.obs_edges = eo; in.body_edges = eb; in.params = par.data();
  // rows a full-length problem needs, generously; cap_short asks for fewer than that
  const int full = (int)((N - 1) / dt_over_dT) + 3;
  const int cap = cap_short ? (full / 2 > 2 ? full / 2 : 2) : full;
  std::vector<double> rows((size_t)batch * cap * timeline::NCOL), duration((size_t)batch);
  std::vector<int32_t> stage((size_t)batch * cap), count((size_t)batch, -1), flags((size_t)batch, -1);
  htp_obca_timeline_opts o{dT * dt_over_dT, cap};
  htp_obca_timeline_result out{rows.data(), stage.data(), count.data(), flags.data(), duration.data()};
  char err[128];
  if (htp_hostsim_obca_timeline(&in, x.data(), &o, &out, err, 128) != 0) { std::printf("error: %s\n", err); return 1; }
  int truncated = 0;
  for (int p = 0; p < batch; ++p) {
    if (flags[p] & (HTP_TIMELINE_NONFINITE | HTP_TIMELINE_BAD_TIME)) { if (count[p] != 0) return 1; continue; }
    if (count[p] < 2) return 1;
    truncated += (flags[p] & HTP_TIMELINE_TRUNCATED) != 0;
    if (((flags[p] & HTP_TIMELINE_TRUNCATED) != 0) != (count[p] > cap)) return 1;
  }
  if (cap_short && N > 2 && !truncated) return 1;
  if (fault && batch >= 3 && (flags[1] != HTP_TIMELINE_NONFINITE || flags[2] != HTP_TIMELINE_BAD_TIME)) return 1;
  std::printf("N %d topt %d batch %d dt/dT %g cap %d: ok (%d truncated)\n", N, topt, batch, dt_over_dT, cap, truncated);
  return 0;
}

}  // namespace

int main() {
  int rc = 0;
  rc |= run(2, 1, 3, 3.0, 0, 0);            // dt > T: two rows
  rc |= run(7, 0, 7, 0.37, 0, 1);           // Euler, a row count that is no multiple of 64
  rc |= run(80, 1, 9, 0.25, 0, 1);          // several chunks
  rc |= run(80, 1, 9, 0.25, 1, 1);          // truncated
  rc |= run(HTP_TIMELINE_MAX_N, 1, 2, 0.25, 0, 0);
  rc |= run(HTP_TIMELINE_MAX_N, 0, 2, 1.0, 1, 0);   // T an exact multiple of dt, truncated
  return rc;
}
