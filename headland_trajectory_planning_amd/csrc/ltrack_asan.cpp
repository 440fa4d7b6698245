// TEST-ONLY stand-alone program: the host build of the rollout under the LQR gains (ltrack_hostsim.cpp) over the
// shapes of the tests, with exactly-sized heap buffers, meant to be built with -fsanitize=address,undefined
// -fno-sanitize-recover=all: any access beyond the x rows, the polygon rows, the scenario table, the gains, the
// outputs or the staging areas that stand for the kernel's LDS aborts it.  Exits 0 when every run returned what it
// must.
#include <cstdio>

#include "ltrack_hostsim.cpp"

namespace {

// a square of half side r around (cx, cy) as four halfspace rows
void square(double* A, double* b, double cx, double cy, double r) {
  const double n[4][2] = {{1, 0}, {0, 1}, {-1, 0}, {0, -1}};
  for (int e = 0; e < 4; ++e) { A[2 * e] = n[e][0]; A[2 * e + 1] = n[e][1]; b[e] = n[e][0] * cx + n[e][1] * cy + r; }
}

int run(int N, int topt, int R, int batch, int M, int K, double dt_over_dT, int ticks_short, int fault) {
  int32_t eo[MAXM], eb[MAXK];
  for (int m = 0; m < M; ++m) eo[m] = 4;
  for (int k = 0; k < K; ++k) eb[k] = 4;
  Dims D;
  make_dims(D, N, M, K, topt, eo, eb);
  const double dT = 0.1;
  const int TEo = 4 * M, TEb = 4 * K;
  std::vector<double> x((size_t)batch * D.n, __builtin_nan("")), par((size_t)batch * NPARAM, 0.0);
  std::vector<double> oA((size_t)batch * TEo * 2), ob((size_t)batch * TEo), bG((size_t)batch * TEb * 2), bg((size_t)batch * TEb);
  std::vector<double> gains((size_t)batch * (N - 1) * ltrack::NGAIN);
  for (int p = 0; p < batch; ++p) {
    double* r = x.data() + (size_t)p * D.n;
    for (int i = 0; i < N; ++i) {      // a gentle left arc at 0.8 m/s (reverse for odd problems), roughly consistent
      const double t = dT * i, v = (p & 1) ? -0.8 : 0.8, w = 0.1;
      r[5 * i] = v / w * std::sin(w * t); r[5 * i + 1] = v / w * (1.0 - std::cos(w * t)); r[5 * i + 2] = v;
      r[5 * i + 3] = w * t; r[5 * i + 4] = std::atan(1.9 * w / v);
    }
    for (int i = 0; i < N - 1; ++i) { r[D.oU + 2 * i] = 0.01 * ((i % 5) - 2); r[D.oU + 2 * i + 1] = 0.005 * ((i % 3) - 1); }
    if (topt) for (int i = 0; i < N - 1; ++i) r[D.oTAU + i] = 0.6 + 0.4 * ((i * 7 + p) % 10) / 10.0;
    double* P = par.data() + (size_t)p * NPARAM;
    P[P_DT] = dT; P[P_WHEELBASE] = 1.9; P[P_MAXSTEER] = 0.6; P[P_MAXV] = 2.0; P[P_MAXACC] = 1.0; P[P_MAXSR] = 0.8;
    P[P_DMIN] = 0.1;
    for (int m = 0; m < M; ++m)
      square(oA.data() + ((size_t)p * TEo + 4 * m) * 2, ob.data() + (size_t)p * TEo + 4 * m, 3.0 * m, 4.0 + m, 0.5);
    for (int k = 0; k < K; ++k)
      square(bG.data() + ((size_t)p * TEb + 4 * k) * 2, bg.data() + (size_t)p * TEb + 4 * k, 0.8 * k, 0.0, 0.7);
    // gains of a plausible size and sign in the world frame of a heading near 0: a acts on x and v, w on y, theta, delta
    const double g = (p & 1) ? -1.0 : 1.0;
    for (int i = 0; i < N - 1; ++i) {
      double* Kp = gains.data() + ((size_t)p * (N - 1) + i) * ltrack::NGAIN;
      const double s = 1.0 + 0.1 * (i % 4);
      const double row_a[5] = {1.0 * s, 0.05, 1.5 * s, 0.0, 0.0}, row_w[5] = {-0.02, g * 0.8 * s, 0.0, 1.6 * s, 2.0 * s};
      for (int q = 0; q < 5; ++q) { Kp[q] = row_a[q]; Kp[5 + q] = row_w[q]; }
    }
  }
  if (fault && batch >= 3) {
    x[(size_t)1 * D.n + 5 * (N / 2) + 1] = __builtin_nan("");
    if (topt) x[(size_t)2 * D.n + D.oTAU] = 0.0; else par[(size_t)2 * NPARAM + P_DT] = -dT;
  }
  if (fault && batch >= 4) gains[((size_t)3 * (N - 1) + (N - 2)) * ltrack::NGAIN + 9] = __builtin_nan("");
  std::vector<double> scen((size_t)R * ltrack::NDIST);
  for (int s = 0; s < R; ++s) {
    double* d = scen.data() + (size_t)s * ltrack::NDIST;
    d[0] = 0.01 * ((s % 7) - 3); d[1] = 0.01 * ((s % 5) - 2); d[2] = 0.005 * ((s % 9) - 4); d[3] = 0.002 * ((s % 3) - 1);
    d[4] = 0.01 * (s % 4); d[5] = 1.0 + 0.01 * ((s % 5) - 2);
  }
  if (fault && R >= 3) { scen[1 * ltrack::NDIST + 3] = __builtin_nan(""); scen[2 * ltrack::NDIST] = 25.0; }
  htp_obca_batch in{};
  in.batch = batch; in.N = N; in.M = M; in.K = K; in.time_opt = topt;
  in.obs_edges = eo; in.body_edges = eb; in.params = par.data();
  in.obs_A = oA.data(); in.obs_b = ob.data(); in.body_G = bG.data(); in.body_g = bg.data();
  // poses a full-length problem needs, generously; ticks_short asks for fewer than that
  const int full = (int)((N - 1) / dt_over_dT) + 3;
  const int mt = ticks_short ? (full / 2 > 2 ? full / 2 : 2) : full;
  const size_t BR = (size_t)batch * R;
  std::vector<double> met(BR * ltrack::NMET), tick((size_t)batch * mt), ref((size_t)batch * mt * ltrack::NREF);
  std::vector<double> terr((size_t)batch * mt * ltrack::NERR, -1.0);
  std::vector<int32_t> worst(BR * 3), flags(BR, -1), tally((size_t)batch * ltrack::NFLAG, -1), ws((size_t)batch, -7);
  htp_obca_ltrack_opts o{dT * dt_over_dT, mt, 2, 2.0, 1e-4, R, scen.data(), gains.data()};
  htp_obca_ltrack_result out{met.data(), worst.data(), flags.data(), tally.data(), ws.data(), tick.data(), ref.data(),
                             terr.data()};
  char err[128];
  if (htp_hostsim_obca_ltrack(&in, x.data(), &o, &out, err, 128) != 0) { std::printf("error: %s\n", err); return 1; }
  int truncated = 0, diverged = 0;
  for (int p = 0; p < batch; ++p) {
    int sum = 0;
    for (int s = 0; s < R; ++s) {
      const int f = flags[(size_t)p * R + s];
      if (f < 0) return 1;
      truncated += (f & HTP_TRACK_TRUNCATED) != 0;
      diverged += (f & HTP_TRACK_DIVERGED) != 0;
      sum += __builtin_popcount((unsigned)f);
    }
    int tsum = 0;
    for (int q = 0; q < ltrack::NFLAG; ++q) tsum += tally[(size_t)p * ltrack::NFLAG + q];
    if (tsum != sum) return 1;
    if (ws[p] < -1 || ws[p] >= R) return 1;
    if (!(terr[(size_t)p * mt * ltrack::NERR] >= 0.0) && flags[(size_t)p * R] != HTP_TRACK_NONFINITE &&
        flags[(size_t)p * R] != HTP_TRACK_BAD_TIME)
      return 1;                        // pose 0 of every accepted problem has its error maxima
  }
  if (ticks_short && N > 2 && !truncated) return 1;
  if (fault && R >= 3 && !diverged) return 1;
  if (fault && batch >= 3 && (flags[(size_t)1 * R] != HTP_TRACK_NONFINITE || flags[(size_t)2 * R] != HTP_TRACK_BAD_TIME)) return 1;
  if (fault && batch >= 4 && flags[(size_t)3 * R] != HTP_TRACK_NONFINITE) return 1;
  // the nullable outputs absent
  out.tick_clearance = nullptr; out.reference = nullptr; out.tick_error = nullptr;
  if (htp_hostsim_obca_ltrack(&in, x.data(), &o, &out, err, 128) != 0) { std::printf("error: %s\n", err); return 1; }
  std::printf("N %d topt %d R %d batch %d M %d K %d dt/dT %g max_ticks %d: ok (%d truncated, %d diverged)\n", N, topt, R,
              batch, M, K, dt_over_dT, mt, truncated, diverged);
  return 0;
}

}  // namespace

int main() {
  int rc = 0;
  rc |= run(2, 1, 1, 3, 1, 1, 3.0, 0, 0);            // dt > T: two poses, one scenario
  rc |= run(7, 0, 65, 5, 2, 1, 0.37, 0, 1);          // Euler, a second pass of scenarios, a partial tick chunk
  rc |= run(80, 1, 64, 8, 6, 2, 0.25, 0, 1);         // several tick chunks
  rc |= run(80, 1, 64, 8, 6, 2, 0.25, 1, 1);         // truncated
  rc |= run(HTP_TRACK_MAX_N, 1, 3, 2, 1, 1, 0.25, 0, 1);
  rc |= run(HTP_TRACK_MAX_N, 0, 3, 2, 1, 1, 1.0, 1, 0);   // T an exact multiple of dt, truncated
  return rc;
}
