// TEST-ONLY host build of the sampled pose search (sample_core.h, serial single-lane context), same structs and
// argument checks as htp_classic_sample_batch.  The product never loads it.
#include <cstdint>
#include <cstdio>
#include <vector>

#define HTP_HD
#include "wave_ctx.h"
#include "sample_batch.h"

extern "C" int htp_hostsim_classic_sample(const htp_classic_sample_in* in, htp_classic_sample_result* out, char* msg,
                                          int32_t msg_len) {
  using namespace htp;
  const char* e = nullptr;
  if (smp::check_args(in, out, &e) || (in->batch > 0 && smp::check_polygons(in, &e))) {
    if (msg && msg_len > 0) std::snprintf(msg, (size_t)msg_len, "%s", e);
    return -1;
  }
  const int64_t total = (int64_t)in->batch * in->cap_cand;
  std::vector<double> ws((size_t)smp::WS_PER_POINT * (size_t)in->cap_samples);
  std::vector<rs::Path> paths(rs::MAXP);
  std::vector<double> tab_s;
  std::vector<int32_t> tab_c;
  double* cs = out->cand_score;
  int32_t* ct = out->cand_status;
  if (!cs) {
    tab_s.resize((size_t)total);
    tab_c.resize((size_t)total);
    cs = tab_s.data();
    ct = tab_c.data();
  }
  std::vector<smp::Scene> scene(1);   // on the heap, exactly sized: the sanitizer build sees an overrun
  HostLane c;
  smp::TurnInfo t;
  int64_t cur = -1;
  for (int64_t it = 0; it < total; ++it) {
    const int64_t b = it / in->cap_cand;
    const int k = (int)(it - b * in->cap_cand);
    if (b != cur) {
      smp::turn_info(*in, b, t);
      if (t.status == smp::ST_OK) smp::load_scene(c, *in, b, t, scene[0]);
      cur = b;
    }
    smp::run_item<smp::M_ALL>(c, *in, cs, ct, b, k, t, scene[0], ws.data(), paths.data());
  }
  for (int64_t b = 0; b < in->batch; ++b) smp::run_winner(c, *in, *out, cs, ct, b);
  return 0;
}

// ring_signed_distance on n points (the hand-computable cases of the tests)
extern "C" void htp_hostsim_ring_distance(const double* ring, int32_t m, const double* pts, int32_t n, double* out) {
  for (int32_t i = 0; i < n; ++i) out[i] = htp::smp::ring_signed_distance(ring, m, pts[2 * i], pts[2 * i + 1]);
}
