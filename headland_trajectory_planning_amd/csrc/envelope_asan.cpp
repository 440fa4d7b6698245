// TEST-ONLY stand-alone program: the host build of the swept-footprint envelope (envelope_hostsim.cpp) over the
// shapes of the tests, with exactly-sized heap buffers, meant to be built with
// -fsanitize=address,undefined -fno-sanitize-recover=all: any access beyond the x rows, the outputs or the
// staging areas that stand for the kernel's LDS aborts it.  Exits 0 when every run returned what it must.
#include <cmath>
#include <cstdio>

#include "envelope_hostsim.cpp"

namespace {

// K rectangles (the second one a hexagon's worth of rows with two redundant ones), a quarter turn of N nodes
int run(int N, int topt, int batch, int K, int S, int W, int H, double res, double phi, int fault, int want_bitmap) {
  const int32_t eo[1] = {3}, eb[2] = {4, 6};
  Dims D;
  make_dims(D, N, 1, K, topt, eo, eb);
  const int TEb = K == 1 ? 4 : 10;
  std::vector<double> x((size_t)batch * D.n, __builtin_nan("")), par((size_t)batch * NPARAM, 0.0);
  std::vector<double> G((size_t)batch * TEb * 2), g((size_t)batch * TEb), frame((size_t)batch * 3);
  for (int p = 0; p < batch; ++p) {
    double* r = x.data() + (size_t)p * D.n;
    for (int i = 0; i < N; ++i) {
      const double s = (double)i / N;
      r[5 * i] = 8.0 * s; r[5 * i + 1] = 3.0 * s * s; r[5 * i + 2] = (i & 1) ? -0.7 : 0.9;
      r[5 * i + 3] = 4.0 * s - 0.3 * p; r[5 * i + 4] = 0.3 - 0.5 * s;
    }
    for (int i = 0; i < N - 1; ++i) { r[D.oU + 2 * i] = 0.1 * ((i % 5) - 2); r[D.oU + 2 * i + 1] = 0.05 * ((i % 3) - 1); }
    if (topt) for (int i = 0; i < N - 1; ++i) r[D.oTAU + i] = 0.5 + 0.5 * ((i * 7 + p) % 10) / 10.0;
    par[(size_t)p * NPARAM + P_DT] = 0.25;
    par[(size_t)p * NPARAM + P_WHEELBASE] = 1.9;
    double* Gp = G.data() + (size_t)p * TEb * 2;
    double* gp = g.data() + (size_t)p * TEb;
    const double rows[10][3] = {{1, 0, 1.5}, {0, 1, 0.8}, {-1, 0, 0.5}, {0, -1, 0.8},
                                {1, 0, -0.5}, {0, 1, 1.2}, {-1, 0, 2.0}, {0, -1, 1.2}, {1, 1, 9.0}, {0, 1, 3.0}};
    for (int q = 0; q < TEb; ++q) { Gp[2 * q] = rows[q][0]; Gp[2 * q + 1] = rows[q][1]; gp[q] = rows[q][2]; }
    frame[3 * p] = -1.0 + 0.01 * p; frame[3 * p + 1] = -0.4; frame[3 * p + 2] = phi;
  }
  if (fault && batch >= 3) {
    x[(size_t)1 * D.n + 5 * (N / 2) + 1] = __builtin_nan("");
    g[(size_t)2 * TEb + 2] = -3.0;   // body 0 of problem 2 is empty
  }
  htp_obca_batch in{};
  in.batch = batch; in.N = N; in.M = 1; in.K = K; in.time_opt = topt;
  in.obs_edges = eo; in.body_edges = eb; in.params = par.data(); in.body_G = G.data(); in.body_g = g.data();
  const size_t nw = (size_t)H * (size_t)(W / 32);
  std::vector<double> extent((size_t)batch * 4), ebody((size_t)batch * K * 4);
  std::vector<int32_t> where((size_t)batch * 12), cells(W ? (size_t)batch * (K + 1) : 0), flags((size_t)batch, -1);
  std::vector<uint32_t> bm(want_bitmap ? (size_t)batch * nw : 0);
  htp_obca_envelope_opts o{S, res, W, H};
  htp_obca_envelope_result out{extent.data(), where.data(), ebody.data(), W ? cells.data() : nullptr,
                               (want_bitmap && W) ? bm.data() : nullptr, flags.data()};
  char err[128];
  if (htp_hostsim_obca_envelope(&in, x.data(), frame.data(), &o, &out, err, 128) != 0) { std::printf("error: %s\n", err); return 1; }
  long total = 0;
  for (int p = 0; p < batch; ++p) {
    if (flags[p] & (HTP_ENVELOPE_NONFINITE | HTP_ENVELOPE_BAD_POLYTOPE)) {
      if (!std::isnan(extent[4 * p]) || where[12 * p] != -1 || (W && cells[(size_t)p * (K + 1) + K] != 0)) return 1;
      continue;
    }
    if (!(extent[4 * p] < extent[4 * p + 1]) || !(extent[4 * p + 2] < extent[4 * p + 3])) return 1;
    if (W) {
      long bits = 0;
      if (want_bitmap) for (size_t q = 0; q < nw; ++q) bits += __builtin_popcount(bm[p * nw + q]);
      if (want_bitmap && bits != cells[(size_t)p * (K + 1) + K]) return 1;
      for (int k = 0; k < K; ++k) if (cells[(size_t)p * (K + 1) + k] > cells[(size_t)p * (K + 1) + K]) return 1;
      total += cells[(size_t)p * (K + 1) + K];
    }
  }
  if (fault && batch >= 3 && (flags[1] != HTP_ENVELOPE_NONFINITE || flags[2] != HTP_ENVELOPE_BAD_POLYTOPE)) return 1;
  std::printf("N %d topt %d batch %d K %d S %d grid %d x %d phi %g: ok (%ld cells)\n", N, topt, batch, K, S, W, H, phi, total);
  return 0;
}

}  // namespace

int main() {
  int rc = 0;
  rc |= run(2, 1, 1, 1, 1, 32, 1, 0.1, 0.0, 0, 1);              // two poses, one bitmap word
  rc |= run(7, 0, 3, 2, 3, 64, 48, 0.2, 0.4, 1, 1);             // Euler, a rotated frame, a partial pose chunk
  rc |= run(80, 1, 3, 2, 4, 256, 256, 0.05, -0.3, 1, 1);        // several chunks, a full bitmap
  rc |= run(80, 1, 2, 2, 4, 65536, 1, 0.001, 0.0, 0, 1);        // the widest grid
  rc |= run(80, 1, 2, 2, 4, 32, 2048, 0.01, -1.2, 0, 1);        // the tallest one with 32 columns
  rc |= run(HTP_ENVELOPE_MAX_N, 1, 2, 2, 16, 256, 256, 0.06, 0.0, 0, 0);   // the LDS limit, no bitmap
  rc |= run(HTP_ENVELOPE_MAX_N, 0, 2, 1, 4, 0, 0, 0.0, 2.0, 0, 0);         // extent only
  return rc;
}
