// TEST-ONLY host build of the repair steps (repair_core.h): serial pack and merge with the argument checks,
// structs and outputs of htp_obca_repair_pack_batch / htp_obca_repair_merge_batch.  Lets CPU tests pin the
// logic against a numpy restatement without a GPU, and the GPU tests compare bit for bit.
#include <cstdint>
#include <cstring>

#define HTP_HD
#include "repair_batch.h"

using namespace htp;

namespace {
int report(const char* e, char* err, int32_t err_len) {
  if (err && err_len > 0) {
    std::strncpy(err, e, (size_t)err_len - 1);
    err[err_len - 1] = 0;
  }
  return -1;
}
}  // namespace

extern "C" int htp_hostsim_repair_pack(const htp_obca_batch* in, const htp_obca_result* out,
                                       const htp_obca_audit_result* audit, const htp_obca_repair_opts* opts,
                                       htp_obca_repair_state* state, htp_obca_repair_slots* slots, char* err,
                                       int32_t err_len) {
  const char* e = nullptr;
  if (repair::check_pack(in, out, audit, opts, state, slots, &e)) return report(e, err, err_len);
  if (in->batch == 0) return 0;
  repair::Shape sh;
  repair::make_shape(sh, *in, slots->cap, opts->pad, opts->max_raise);
  repair::pack_serial(sh, repair::pack_view(*in, *out, *audit, *state, *slots));
  return 0;
}

extern "C" int htp_hostsim_repair_merge(const htp_obca_batch* in, const htp_obca_repair_slots* slots,
                                        const htp_obca_result* re, const htp_obca_audit_result* re_audit,
                                        htp_obca_result* out, htp_obca_audit_result* audit,
                                        htp_obca_repair_state* state, int32_t* tally, char* err, int32_t err_len) {
  const char* e = nullptr;
  if (repair::check_merge(in, slots, re, re_audit, out, audit, state, &e)) return report(e, err, err_len);
  if (in->batch == 0) return 0;
  repair::Shape sh;
  repair::make_shape(sh, *in, slots->cap, 0.0, 0.0);
  repair::merge_serial(sh, repair::merge_view(*slots, *re, *re_audit, *out, *audit, *state, tally));
  return 0;
}

// the argument checks of the loop (htp_obca_repair_batch), which the host build does not run itself
extern "C" int htp_hostsim_repair_check_loop(const htp_obca_batch* in, const htp_obca_result* out,
                                             const htp_obca_repair_opts* opts, const htp_obca_audit_result* audit,
                                             const htp_obca_repair_report* rep, char* err, int32_t err_len) {
  const char* e = nullptr;
  if (repair::check_loop(in, out, opts, audit, rep, &e)) return report(e, err, err_len);
  return 0;
}
