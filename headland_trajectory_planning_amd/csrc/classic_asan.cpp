// TEST-ONLY stand-alone program: the host build of the classic-turn planner (classic_batch.h run_problem, the
// serial HostLane) over one packed batch read from a file, with exactly-sized heap buffers, meant to be built with
// -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all: a double converted to int out of its
// range, or any access beyond the parameter rows, the polygon pools, the planner scratch (SCR_PER_POINT * cap_samples
// doubles) or the outputs (batch * cap_path * 5 doubles) aborts it.
//
//   classic_asan IN OUT
//   IN : int32 batch, npoly, nvert, cap_path, cap_samples; double params[batch][HTP_CT_NPARAM]; int32 desc[batch][3];
//        int32 poly_off[npoly + 1]; double vertices[nvert][2]
//   OUT: int32 status[batch]; int32 n_path[batch]; double path[batch][cap_path][5]
// The outputs start as -77 / -7.25 (the tests' sentinels), so what the planner leaves unwritten is recognisable.
#include <cstdint>
#include <cstdio>
#include <vector>

#define HTP_HD
#include "wave_ctx.h"
#include "classic_batch.h"

namespace {

template <class T>
bool get(std::FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

template <class T>
bool put(std::FILE* f, const std::vector<T>& v) {
  return v.empty() || std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: classic_asan IN OUT\n"); return 2; }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::fprintf(stderr, "classic_asan: cannot read %s\n", argv[1]); return 2; }
  std::vector<int32_t> hdr, desc, poly_off;
  std::vector<double> params, vertices;
  bool ok = get(f, hdr, 5);
  ok = ok && hdr[0] >= 0 && hdr[1] >= 0 && hdr[2] >= 0 && hdr[3] >= 1 && hdr[4] >= 16;
  const size_t B = ok ? hdr[0] : 0;
  ok = ok && get(f, params, B * HTP_CT_NPARAM) && get(f, desc, 3 * B) && get(f, poly_off, (size_t)hdr[1] + 1) &&
       get(f, vertices, 2 * (size_t)hdr[2]);
  std::fclose(f);
  if (!ok) { std::fprintf(stderr, "classic_asan: bad input file\n"); return 2; }
  for (size_t b = 0; b < B; ++b) {   // polygon ids in range, as htp_classic_turn_batch checks them
    const int32_t* d = desc.data() + 3 * b;
    if (d[0] < 0 || d[0] >= hdr[1] || d[1] < 0 || d[2] < d[1] || d[2] > hdr[1]) return 2;
  }
  if (poly_off[0] != 0 || poly_off[hdr[1]] != hdr[2]) return 2;
  const htp_classic_batch in{hdr[0], hdr[1], hdr[2], params.data(), desc.data(), poly_off.data(), vertices.data(),
                             hdr[3], hdr[4]};
  std::vector<int32_t> status(B, -77), n_path(B, -77);
  std::vector<double> path(B * (size_t)in.cap_path * 5, -7.25);
  const htp_classic_result out{status.data(), n_path.data(), path.data()};
  std::vector<double> scr((size_t)htp::ct::SCR_PER_POINT * (size_t)in.cap_samples);
  std::vector<htp::rs::Path> paths(htp::rs::MAXP);
  std::vector<int> flags(htp::rs::MAXP);
  for (size_t b = 0; b < B; ++b) {
    htp::HostLane c;
    htp::ct::run_problem(c, in, out, (int64_t)b, scr.data(), paths.data(), flags.data());
  }
  f = std::fopen(argv[2], "wb");
  if (!f) { std::fprintf(stderr, "classic_asan: cannot write %s\n", argv[2]); return 2; }
  ok = put(f, status) && put(f, n_path) && put(f, path);
  ok = std::fclose(f) == 0 && ok;
  return ok ? 0 : 2;
}
