// TEST-ONLY probe of the small dense factorizations in obca_core.h, one block per call: the unpivoted LDL^T of
// the local blocks, every form of the Bunch-Kaufman factorization / solve the solver substitutes for one another,
// and the 3 x 3 / 5 x 5 Cholesky helpers.  One body, three builds: the device (htp_bkprobe.hip, one block per
// lane), the serial host build (htp_hostsim.cpp) and the contracting host build (htp_emusim.cpp).  It defines no
// solver object; the solver's static members are named through its type.  tests/test_bk_cpu.py, test_gpu_bk.py.
#pragma once
#include <type_traits>

#include "obca_core.h"

namespace htp {
namespace bkp {

// variant ids (include/htp.h, htp_bk_probe)
constexpr int V_UNPIV = 0;       // LocalBlock<4,4> (n 10) / PtBlock<4> / PtBlock<8>: factor, solve (+ forward, n 10)
constexpr int V_PACKED = 1;      // bk_factor_packed / bk_solve_packed on a private array
constexpr int V_PACKED_LDS = 2;  // the same on the lane-contiguous LDS slice of ObcaSolver::local_pivoted
constexpr int V_SIMD = 3;        // bk_factor_simd / bk_solve_simd
constexpr int V_BATCH = 4;       // bk_factor_batch / bk_solve_batch (+ bk_solve_batch_multi<.., 4> when nrhs == 4)
constexpr int V_BATCH_P = 5;     // bk_factor_batch_p / bk_solve_batch_l (packed pivots, right-hand side at stride 64)
constexpr int V_CHOL3 = 6;       // ObcaSolver::chol3 / chol3_solve, n = nv
constexpr int V_CHOL5 = 7;       // ObcaSolver::chol5 / chol5_fwd / chol5_bwd
constexpr int MAXRHS = 4;

// doubles per block of the input matrix and of the returned factor
inline int in_doubles(int v, int n) { return v == V_CHOL3 ? 9 : v == V_CHOL5 ? 25 : n * (n + 1) / 2; }
inline int out_doubles(int v, int n) { return v == V_CHOL3 ? 9 : v == V_CHOL5 ? 15 : n * (n + 1) / 2; }

struct Io {
  const double* K0;   // packed lower [n (n + 1) / 2]; chol3: 3 x 3 stride 3; chol5: 5 x 5 row-major
  const double* rhs;  // [nrhs][n]
  int nrhs;           // <= MAXRHS
  double* K;          // the factor as the form leaves it (chol3: Lc[9]; chol5: packed Lc[15])
  int* ip;            // [n] pivot vector (bk_factor_packed's convention); the unpivoted forms write j
  int* flags;         // neg, zero, piv, ok (-1 where the form has none)
  double* x;          // [nrhs][n] solutions
  double* x2;         // [nrhs][n]: V_UNPIV n 10 forward(); V_BATCH nrhs 4 bk_solve_batch_multi; V_CHOL5 chol5_fwd
};

// Block `idx` of the batch arrays (htp_bk_probe's layout)
HTP_HD HTP_FI inline Io view(int v_in, int v_out, int n, int nrhs, long long idx, const double* K0, const double* rhs,
                             double* K, int* ip, int* flags, double* x, double* x2) {
  return Io{K0 + idx * v_in, rhs + idx * nrhs * n, nrhs, K + idx * v_out, ip + idx * n, flags + idx * 4,
            x + idx * nrhs * n, x2 + idx * nrhs * n};
}

// lds: the wave's LDS as the solver sizes it (LDS_WAVE_DOUBLES); lane: this block's lane in it.  S = 64: the block
// interleaved with the other lanes' at lds[RING_OFF + 64 e + lane] (local_pivoted_v); S = 1: a private array.
template <class Ctx, int V, int N, int S>
HTP_HD HTP_FI inline void probe_block(const Io& io, typename Ctx::ld* lds, int lane) {
  using ld = typename Ctx::ld;
  static_assert(S == 1 || S == 64, "the solver's two layouts");
  int neg = -1, zero = -1, piv = -1, ok = -1;
  if constexpr (V == V_UNPIV) {
    static_assert(S == 1 && (N == 10 || N == 4 || N == 8), "LocalBlock<4,4>, PtBlock<4>, PtBlock<8>");
    using Blk = std::conditional_t<N == 10, LocalBlock<4, 4>, PtBlock<N == 10 ? 4 : N>>;
    static_assert(Blk::NL == N, "block size");
    Blk B;
    for (int q = 0; q < Blk::NPK; ++q) B.K[q] = io.K0[q];
    B.factor();
    for (int q = 0; q < Blk::NPK; ++q) io.K[q] = B.K[q];
    for (int j = 0; j < N; ++j) io.ip[j] = j;
    neg = B.neg;
    zero = B.zero;
    piv = B.piv ? 1 : 0;
    for (int k = 0; k < io.nrhs; ++k) {
      double v[N];
      for (int j = 0; j < N; ++j) v[j] = io.rhs[k * N + j];
      B.solve(v);
      for (int j = 0; j < N; ++j) io.x[k * N + j] = v[j];
      if constexpr (N == 10) {
        for (int j = 0; j < N; ++j) v[j] = io.rhs[k * N + j];
        B.forward(v);
        for (int j = 0; j < N; ++j) io.x2[k * N + j] = v[j];
      }
    }
  } else if constexpr (V == V_PACKED || V == V_PACKED_LDS) {
    static_assert(S == 1, "serial form");
    constexpr int NPK = N * (N + 1) / 2;
    int ip[N];
    double v[N];
    if constexpr (V == V_PACKED_LDS) {
      static_assert(NPK <= PIV_LDS_PER_LANE, "the lane's LDS slice");
      ld* K = lds + RING_OFF + lane * NPK;
      for (int q = 0; q < NPK; ++q) K[q] = io.K0[q];
      bk_factor_packed(K, ip, N, neg, zero);
      for (int k = 0; k < io.nrhs; ++k) {
        for (int j = 0; j < N; ++j) v[j] = io.rhs[k * N + j];
        bk_solve_packed(K, ip, N, v);
        for (int j = 0; j < N; ++j) io.x[k * N + j] = v[j];
      }
      for (int q = 0; q < NPK; ++q) io.K[q] = K[q];
    } else {
      double K[NPK];
      for (int q = 0; q < NPK; ++q) K[q] = io.K0[q];
      bk_factor_packed(K, ip, N, neg, zero);
      for (int k = 0; k < io.nrhs; ++k) {
        for (int j = 0; j < N; ++j) v[j] = io.rhs[k * N + j];
        bk_solve_packed(K, ip, N, v);
        for (int j = 0; j < N; ++j) io.x[k * N + j] = v[j];
      }
      for (int q = 0; q < NPK; ++q) io.K[q] = K[q];
    }
    for (int j = 0; j < N; ++j) io.ip[j] = ip[j];
  } else if constexpr (V == V_SIMD || V == V_BATCH || V == V_BATCH_P) {
    constexpr int NPK = N * (N + 1) / 2;
    static_assert(S == 1 || NPK <= PIV_LDS_PER_LANE, "the lane's LDS slice");
    using KT = std::conditional_t<S == 64, ld, double>;
    double Kp[S == 64 ? 1 : NPK];
    KT* K;
    if constexpr (S == 64) K = lds + RING_OFF + lane;
    else K = Kp;
#pragma unroll
    for (int q = 0; q < NPK; ++q) K[S * q] = io.K0[q];
    int ip[N];
    if constexpr (V == V_BATCH_P) {
      // the right-hand side in this lane's slice of the stage-LDL scratch [0, 64 N), as local_pivoted_v lays it out
      static_assert(64 * N <= 4 * NBMAX * NBMAX, "pivoted right-hand sides exceed the stage-LDL scratch");
      unsigned long long ipw;
      bk_factor_batch_p<N, S>(K, ipw, neg, zero);
      ld* vl = lds + lane;
      for (int k = 0; k < io.nrhs; ++k) {
#pragma unroll
        for (int j = 0; j < N; ++j) vl[64 * j] = io.rhs[k * N + j];
        bk_solve_batch_l<N, S>(K, ipw, vl);
#pragma unroll
        for (int j = 0; j < N; ++j) io.x[k * N + j] = vl[64 * j];
      }
#pragma unroll
      for (int j = 0; j < N; ++j) ip[j] = piv_get(ipw, j);
    } else {
      if constexpr (V == V_SIMD) bk_factor_simd<N, S>(K, ip, neg, zero);
      else bk_factor_batch<N, S>(K, ip, neg, zero);
      for (int k = 0; k < io.nrhs; ++k) {
        double v[N];
#pragma unroll
        for (int j = 0; j < N; ++j) v[j] = io.rhs[k * N + j];
        if constexpr (V == V_SIMD) bk_solve_simd<N, S>(K, ip, v);
        else bk_solve_batch<N, S>(K, ip, v);
#pragma unroll
        for (int j = 0; j < N; ++j) io.x[k * N + j] = v[j];
      }
      if constexpr (V == V_BATCH) {
        if (io.nrhs == MAXRHS) {
          double vm[MAXRHS][N];
#pragma unroll
          for (int k = 0; k < MAXRHS; ++k)
#pragma unroll
            for (int j = 0; j < N; ++j) vm[k][j] = io.rhs[k * N + j];
          bk_solve_batch_multi<N, S, MAXRHS>(K, ip, vm);
#pragma unroll
          for (int k = 0; k < MAXRHS; ++k)
#pragma unroll
            for (int j = 0; j < N; ++j) io.x2[k * N + j] = vm[k][j];
        }
      }
    }
#pragma unroll
    for (int q = 0; q < NPK; ++q) io.K[q] = K[S * q];
#pragma unroll
    for (int j = 0; j < N; ++j) io.ip[j] = ip[j];
  } else if constexpr (V == V_CHOL3) {
    static_assert(S == 1 && N >= 1 && N <= 3, "nv");
    using Sv = ObcaSolver<Ctx, 4, 4, 0>;
    double R[9], Lc[9];
    for (int q = 0; q < 9; ++q) R[q] = io.K0[q];
    ok = Sv::chol3(R, N, Lc) ? 1 : 0;
    for (int q = 0; q < 9; ++q) io.K[q] = Lc[q];
    for (int j = 0; j < N; ++j) io.ip[j] = j;
    for (int k = 0; k < io.nrhs; ++k) {
      double b[3] = {0.0, 0.0, 0.0};
      for (int j = 0; j < N; ++j) b[j] = io.rhs[k * N + j];
      Sv::chol3_solve(Lc, N, b);
      for (int j = 0; j < N; ++j) io.x[k * N + j] = b[j];
    }
  } else {
    static_assert(V == V_CHOL5 && S == 1 && N == NS, "chol5 factors an NS x NS matrix");
    using Sv = ObcaSolver<Ctx, 4, 4, 0>;
    double Am[NS * NS], Lc[15];
    for (int q = 0; q < NS * NS; ++q) Am[q] = io.K0[q];
    ok = Sv::chol5(Am, Lc) ? 1 : 0;
    for (int q = 0; q < 15; ++q) io.K[q] = Lc[q];
    for (int j = 0; j < N; ++j) io.ip[j] = j;
    for (int k = 0; k < io.nrhs; ++k) {
      double b[NS];
      for (int j = 0; j < N; ++j) b[j] = io.rhs[k * N + j];
      Sv::chol5_fwd(Lc, b);
      for (int j = 0; j < N; ++j) io.x2[k * N + j] = b[j];
      Sv::chol5_bwd(Lc, b);
      for (int j = 0; j < N; ++j) io.x[k * N + j] = b[j];
    }
  }
  io.flags[0] = neg;
  io.flags[1] = zero;
  io.flags[2] = piv;
  io.flags[3] = ok;
}

// piv_put / piv_get round trip: word w with slot j set to v -> the word and all n slots read back
HTP_HD HTP_FI inline unsigned long long piv_roundtrip(unsigned long long w, int j, int v, int n, int* slots) {
  const unsigned long long r = piv_put(w, j, v);
  for (int q = 0; q < n; ++q) slots[q] = piv_get(r, q);
  return r;
}

template <int V_, int N_, int S_>
struct Tag {
  static constexpr int V = V_, N = N_, S = S_;
};

// The (variant, n, S) instantiations: the sizes the shipped kernels run (n 10 = LocalBlock<4,4>, n 18 =
// LocalBlock<MAXE,MAXE>, n 4 / 8 = PtBlock<4> / PtBlock<MAXE>), S = 64 only where the block fits the LDS slice.
template <class F>
inline bool dispatch(int v, int n, int s, F&& f) {
#define HTP_BKP_CASE(V_, N_, S_) \
  if (v == V_ && n == N_ && s == S_) { f(Tag<V_, N_, S_>{}); return true; }
  HTP_BKP_CASE(V_UNPIV, 10, 1) HTP_BKP_CASE(V_UNPIV, 4, 1) HTP_BKP_CASE(V_UNPIV, 8, 1)
  HTP_BKP_CASE(V_PACKED, 4, 1) HTP_BKP_CASE(V_PACKED, 8, 1) HTP_BKP_CASE(V_PACKED, 10, 1) HTP_BKP_CASE(V_PACKED, 18, 1)
  HTP_BKP_CASE(V_PACKED_LDS, 10, 1)
  HTP_BKP_CASE(V_SIMD, 10, 64) HTP_BKP_CASE(V_SIMD, 10, 1) HTP_BKP_CASE(V_SIMD, 18, 1)
  HTP_BKP_CASE(V_BATCH, 10, 64) HTP_BKP_CASE(V_BATCH, 10, 1) HTP_BKP_CASE(V_BATCH, 18, 1)
  HTP_BKP_CASE(V_BATCH_P, 10, 64) HTP_BKP_CASE(V_BATCH_P, 10, 1)
  HTP_BKP_CASE(V_CHOL3, 1, 1) HTP_BKP_CASE(V_CHOL3, 2, 1) HTP_BKP_CASE(V_CHOL3, 3, 1)
  HTP_BKP_CASE(V_CHOL5, 5, 1)
#undef HTP_BKP_CASE
  return false;
}

// Serial host driver (both host builds): block idx runs as lane idx % 64 of a wave's LDS image
template <class Ctx>
inline int run_host(int variant, int n, int s, long long count, int nrhs, const double* K0, const double* rhs,
                    double* K, int* ip, int* flags, double* x, double* x2, double* lds) {
  if (count < 0 || nrhs < 0 || nrhs > MAXRHS) return -1;
  const int vi = in_doubles(variant, n), vo = out_doubles(variant, n);
  const bool known = dispatch(variant, n, s, [&](auto tag) {
    using T = decltype(tag);
    for (long long idx = 0; idx < count; ++idx)
      probe_block<Ctx, T::V, T::N, T::S>(view(vi, vo, n, nrhs, idx, K0, rhs, K, ip, flags, x, x2), lds,
                                         (int)(idx % 64));
  });
  return known ? 0 : -2;
}

}  // namespace bkp
}  // namespace htp
