// TEST-ONLY host build of the speed profile (speed_core.h, serial single-lane context), same structs and argument
// checks as htp_speed_profile_batch.  The product never loads it.
#include <cstdint>
#include <cstdio>
#include <vector>

#define HTP_HD
#include "wave_ctx.h"
#include "speed_batch.h"

extern "C" int htp_hostsim_speed_profile(const htp_speed_in* in, htp_speed_result* out, char* msg, int32_t msg_len) {
  using namespace htp;
  const char* e = nullptr;
  if (spd::check_args(in, out, &e)) {
    if (msg && msg_len > 0) std::snprintf(msg, (size_t)msg_len, "%s", e);
    return -1;
  }
  // on the heap, exactly sized: the sanitizer build sees an overrun
  std::vector<double> ws((size_t)spd::WS_PER_NODE * (size_t)in->cap_path), tile(spd::TILE);
  HostLane c;
  for (int64_t b = 0; b < in->batch; ++b) spd::run_path(c, *in, *out, b, ws.data(), tile.data());
  return 0;
}
