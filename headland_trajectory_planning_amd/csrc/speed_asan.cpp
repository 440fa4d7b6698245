// TEST-ONLY stand-alone program: the host build of the speed profile (speed_hostsim.cpp) over line, arc, cusp, dwell,
// hop and bad-input paths, with exactly-sized heap buffers, meant to be built with -fsanitize=address,undefined
// -fno-sanitize-recover=all: any access beyond the path rows, the limits, the per-node outputs, the fixed-period rows,
// the scratch or the tile that stands for the kernel's LDS aborts it.  Exits 0 when every run returned what it must.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "speed_hostsim.cpp"

namespace {

int failures = 0;

void expect(bool ok, const char* what) {
  if (!ok) {
    std::printf("FAIL: %s\n", what);
    ++failures;
  }
}

struct Batch {
  int cap;
  std::vector<double> path, limits;
  std::vector<int32_t> n_path, pstat;
  explicit Batch(int c) : cap(c) {}

  // rows of one path appended by the caller through row(); close() pads the block to cap rows
  std::vector<double> cur;
  void row(double x, double y, double yaw, double k, double dir) {
    const double r[5] = {x, y, yaw, k, dir};
    cur.insert(cur.end(), r, r + 5);
  }
  void close(int n_override = -1, int status = 0, double acc = 1.0) {
    const int n = (int)cur.size() / 5;
    cur.resize((size_t)cap * 5, 0.0);
    path.insert(path.end(), cur.begin(), cur.end());
    cur.clear();
    n_path.push_back(n_override >= 0 ? n_override : n);
    pstat.push_back(status);
    const double l[HTP_SPD_NLIM] = {1.9, 2.0, 1.0, acc, 1.0, 1.0, 0.7, 0.55, 0.0, 0.0};
    limits.insert(limits.end(), l, l + HTP_SPD_NLIM);
  }
  int batch() const { return (int)n_path.size(); }
};

struct Out {
  std::vector<int32_t> status, flags, active, count, stage;
  std::vector<double> summary, node, rows;
  Out(int B, int cap, int capr)
      : status(B, -7), flags(B, -7), active((size_t)B * cap, -7), count(B, -7), stage((size_t)B * capr, -7),
        summary((size_t)B * HTP_SPD_NSUM, -7.0), node((size_t)B * cap * HTP_SPD_NNODE, -7.0),
        rows((size_t)B * capr * HTP_TIMELINE_NCOL, -7.0) {}
  htp_speed_result res() {
    return htp_speed_result{status.data(), flags.data(), summary.data(), node.data(), active.data(), count.data(),
                            rows.empty() ? nullptr : rows.data(), stage.empty() ? nullptr : stage.data()};
  }
};

}  // namespace

int main() {
  const int cap = 130;
  Batch b(cap);
  // 0: a 10 m line, 101 rows
  for (int i = 0; i <= 100; ++i) b.row(0.1 * i, 0.0, 0.0, 0.0, 1.0);
  b.close();
  // 1: exactly cap rows: an arc of radius 3, then reversing along it (a cusp in the middle)
  for (int i = 0; i < cap; ++i) {
    const int j = i < 65 ? i : 129 - i;
    const double a = 0.1 * j / 3.0;
    b.row(3.0 * std::sin(a), 3.0 * (1.0 - std::cos(a)), a, 1.0 / 3.0, i <= 65 ? 1.0 : -1.0);
  }
  b.close();
  // 2: a two-row path: a hop
  b.row(0.0, 0.0, 0.0, 0.0, 1.0);
  b.row(0.05, 0.0, 0.0, 0.0, 1.0);
  b.close();
  // 3: a dwell: a repeated row across which the curvature jumps from lock to lock
  for (int i = 0; i <= 20; ++i) b.row(0.1 * i, 0.0, 0.0, 0.3, 1.0);
  for (int i = 20; i <= 40; ++i) b.row(0.1 * i, 0.0, 0.0, -0.3, 1.0);
  b.close();
  // 4: n_path beyond cap, 5: n_path 1, 6: a NaN row, 7: skipped, 8: a bad direction, 9: acc = 0
  b.row(0.0, 0.0, 0.0, 0.0, 1.0); b.row(1.0, 0.0, 0.0, 0.0, 1.0); b.close(cap + 1);
  b.row(0.0, 0.0, 0.0, 0.0, 1.0); b.close();
  b.row(0.0, 0.0, 0.0, 0.0, 1.0); b.row(std::nan(""), 0.0, 0.0, 0.0, 1.0); b.close();
  b.row(0.0, 0.0, 0.0, 0.0, 1.0); b.row(1.0, 0.0, 0.0, 0.0, 1.0); b.close(-1, 3);
  b.row(0.0, 0.0, 0.0, 0.0, 1.0); b.row(1.0, 0.0, 0.0, 0.0, 0.5); b.close();
  b.row(0.0, 0.0, 0.0, 0.0, 1.0); b.row(1.0, 0.0, 0.0, 0.0, 1.0); b.close(-1, 0, 0.0);
  const int B = b.batch();

  char msg[128];
  for (int pass = 0; pass < 3; ++pass) {   // rows with room, rows truncated, no rows
    const double dt = pass == 2 ? 0.0 : 0.25;
    const int capr = pass == 0 ? 64 : (pass == 1 ? 5 : 0);
    Out o(B, cap, capr);
    htp_speed_in in{B, cap, b.path.data(), b.n_path.data(), b.pstat.data(), b.limits.data(), dt, capr, 0};
    htp_speed_result r = o.res();
    expect(htp_hostsim_speed_profile(&in, &r, msg, sizeof msg) == 0, "the call succeeds");
    expect(o.status[0] == HTP_SPD_OK && std::fabs(o.summary[HTP_SPD_S_T] - 7.0) < 1e-12, "10 m line: T = 7");
    expect(o.status[1] == HTP_SPD_OK && o.summary[HTP_SPD_NSUM + HTP_SPD_S_STOPS] == 1.0, "arc and back: one stop");
    expect(o.status[2] == HTP_SPD_OK && (o.flags[2] & HTP_SPD_F_HOP), "two rows: a hop");
    expect(o.status[3] == HTP_SPD_OK && o.summary[3 * HTP_SPD_NSUM + HTP_SPD_S_DWELL] > 0.0, "lock to lock: a dwell");
    for (int k = 4; k < B; ++k) {
      const int want = k == 7 ? HTP_SPD_SKIPPED : HTP_SPD_BAD_INPUT;
      expect(o.status[k] == want && o.count[k] == 0 && o.flags[k] == 0, "rejected path: its status");
      expect(o.summary[(size_t)k * HTP_SPD_NSUM] == -7.0 && o.node[(size_t)k * cap * HTP_SPD_NNODE] == -7.0 &&
                 o.active[(size_t)k * cap] == -7, "rejected path: nothing else written");
    }
    if (pass == 0) expect(o.count[0] == 29 && !(o.flags[0] & HTP_SPD_F_TRUNCATED), "28 regular rows and the final one");
    if (pass == 1) {
      expect(o.count[0] == 29 && (o.flags[0] & HTP_SPD_F_TRUNCATED), "truncated, count intact");
      expect(o.rows[(size_t)4 * HTP_TIMELINE_NCOL] == 1.0, "row 4 of the line at t = 1");
    }
    if (pass == 2) expect(o.count[0] == 0, "dt = 0: no rows");
    expect(o.node[((size_t)0 * cap + 101) * HTP_SPD_NNODE] == -7.0, "rows from n_path on are left as they were");
  }
  // API errors
  Out o(B, cap, 8);
  htp_speed_result r = o.res();
  htp_speed_in in{B, cap, b.path.data(), b.n_path.data(), nullptr, b.limits.data(), 0.25, 1, 0};
  expect(htp_hostsim_speed_profile(&in, &r, msg, sizeof msg) == -1 && std::strstr(msg, "[speed]"), "cap_rows < 2");
  in.cap_rows = 8;
  in.cap_path = 1;
  expect(htp_hostsim_speed_profile(&in, &r, msg, sizeof msg) == -1, "cap_path < 2");
  expect(htp_hostsim_speed_profile(nullptr, &r, msg, sizeof msg) == -1, "null input");
  std::printf(failures ? "speed_asan: %d failure(s)\n" : "speed_asan: OK\n", failures);
  return failures ? 1 : 0;
}
