// TEST-ONLY stand-alone program: the host build of the pose clearance and the turn selection (clear_hostsim.cpp) over
// paths of 1, 2, a chunk and two chunks plus one poses, both layouts, shared scenes, rejected paths and a gather at, below
// and above its row storage, with exactly-sized heap buffers, meant to be built with -fsanitize=address,undefined
// -fno-sanitize-recover=all: any access beyond the pose rows, the scenes, the outputs or the array that stands for the
// kernel's LDS aborts it.  Exits 0 when every run returned what it must.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "clear_hostsim.cpp"

namespace {

int failures = 0;

void expect(bool ok, const char* what) {
  if (!ok) {
    std::printf("FAIL: %s\n", what);
    ++failures;
  }
}

// axis-parallel rectangle [x0, x1] x [y0, y1] as four halfspace rows
void rect(std::vector<double>& A, std::vector<double>& b, double x0, double x1, double y0, double y1) {
  const double a[8] = {1, 0, -1, 0, 0, 1, 0, -1}, r[4] = {x1, -x0, y1, -y0};
  A.insert(A.end(), a, a + 8);
  b.insert(b.end(), r, r + 4);
}

}  // namespace

int main() {
  char msg[160];
  // two scenes: M = 2 obstacles (a wall above the path, a block ahead of it), K = 1 body, a 2 x 1 rectangle
  const int32_t oe[2] = {4, 4}, be[1] = {4};
  std::vector<double> A, b, G, g, margin = {0.1, 0.1};
  for (int s = 0; s < 2; ++s) {
    rect(A, b, -5.0, 40.0, 1.5 + s, 2.5 + s);
    rect(A, b, 30.0, 31.0, -0.5, 0.5);
    rect(G, g, -1.0, 1.0, -0.5, 0.5);
  }
  for (int pass = 0; pass < 4; ++pass) {
    const int S = pass == 0 ? 1 : pass == 1 ? 2 : 16, CP = 128 / S;
    const int stride = pass == 3 ? 10 : 5, cx = pass == 3 ? 1 : 0, cy = pass == 3 ? 2 : 1, cw = pass == 3 ? 4 : 2;
    const int lens[8] = {1, 2, CP - 1, CP, CP + 1, 2 * CP + 1, 3, 3};
    const int cap = 2 * CP + 1, B = 8;
    std::vector<double> poses((size_t)B * cap * stride, 0.0);
    std::vector<int32_t> n(B), pstat(B, 0), scene = {0, 1, 0, 0, 1, 0, 0, 5};
    for (int p = 0; p < B; ++p) {
      n[p] = lens[p];
      for (int i = 0; i < lens[p]; ++i) {
        double* r = &poses[((size_t)p * cap + i) * stride];
        r[cx] = 0.1 * i; r[cy] = 0.0; r[cw] = 0.0001 * i;
      }
    }
    n[5] = cap + 3;      // more poses than storage: truncated
    pstat[6] = 4;        // skipped; path 7 names a scene that does not exist
    std::vector<int32_t> status(B, -7), flags(B, -7), worst((size_t)B * 4, -7);
    std::vector<double> metrics((size_t)B * HTP_CLR_NMETRIC, -7.0), pc((size_t)B * cap, -7.0);
    htp_clear_in in{B, cap, stride, cx, cy, cw, poses.data(), n.data(), pstat.data(), scene.data(), 2, 2, 1, oe, be,
                    A.data(), b.data(), G.data(), g.data(), margin.data(), S, 1e-9, 0};
    htp_clear_result out{status.data(), flags.data(), metrics.data(), worst.data(), pc.data()};
    expect(htp_hostsim_pose_clearance(&in, &out, msg, sizeof msg) == 0, "the call succeeds");
    for (int p = 0; p < 6; ++p) {
      expect(status[p] == HTP_CLR_OK, "a good path is OK");
      // the body's top edge is at y = 0.5 (nearly: the yaw is small), the wall's bottom at 1.5 + scene
      expect(std::fabs(metrics[(size_t)p * HTP_CLR_NMETRIC] - (1.0 + scene[p])) < 0.2, "clearance to the wall");
      expect(lens[p] >= cap || pc[(size_t)p * cap + lens[p]] == -7.0, "entries from n on untouched");
    }
    expect(flags[5] == HTP_CLR_F_TRUNCATED && flags[0] == 0, "truncation is flagged");
    expect(status[6] == HTP_CLR_SKIPPED && status[7] == HTP_CLR_BAD_INPUT && flags[6] == 0 && flags[7] == 0,
           "rejected paths: their status");
    expect(metrics[6 * HTP_CLR_NMETRIC] == -7.0 && worst[7 * 4] == -7 && pc[(size_t)6 * cap] == -7.0,
           "rejected paths: nothing else written");
    // scene = null needs n_scenes == batch
    in.scene = nullptr;
    expect(htp_hostsim_pose_clearance(&in, &out, msg, sizeof msg) == -1 && std::strstr(msg, "[clearance]"), "null scene");
  }
  expect(htp_hostsim_pose_clearance(nullptr, nullptr, msg, sizeof msg) == -1, "null input");

  // selection: B = 2 problems, C = 3 candidates, rows of 4 with count below, at and above the storage
  {
    const int B = 2, C = 3, capr = 4, N = B * C;
    std::vector<int32_t> ss(N, 0), sf(N, 0), cs(N, 0), cf(N, 0), count = {2, 9, 4, 1, 5, 3};
    std::vector<double> sm((size_t)N * HTP_SPD_NSUM, 0.0), cm((size_t)N * HTP_CLR_NMETRIC, 0.5);
    std::vector<double> rows((size_t)N * capr * HTP_TIMELINE_NCOL);
    for (size_t q = 0; q < rows.size(); ++q) rows[q] = (double)q;
    const double T[6] = {9.0, 3.0, 7.0, 8.0, 7.0, 2.0};   // index c B + b
    for (int j = 0; j < N; ++j) sm[(size_t)j * HTP_SPD_NSUM + HTP_SPD_S_T] = T[j];
    cf[5] = HTP_CLR_F_COLLISION;    // problem 1's fastest candidate collides
    std::vector<int32_t> verdict(N, -7), winner(B, -7), ocount(B, -7);
    std::vector<double> score(B, -7.0), clear(B, -7.0), orows((size_t)B * capr * HTP_TIMELINE_NCOL, -7.0);
    htp_select_in in{B, C, ss.data(), sf.data(), sm.data(), rows.data(), count.data(), capr, cs.data(), cf.data(),
                     cm.data(), 0, HTP_CLR_F_COLLISION, 0.0};
    htp_select_result out{verdict.data(), winner.data(), score.data(), clear.data(), orows.data(), ocount.data()};
    expect(htp_hostsim_turn_select(&in, &out, msg, sizeof msg) == 0, "the selection succeeds");
    expect(winner[0] == 1 && score[0] == 7.0 && ocount[0] == 4, "problem 0: candidate 1, T = 7 (a tie goes to the lower c)");
    expect(winner[1] == 0 && score[1] == 3.0 && ocount[1] == 9, "problem 1: the colliding candidate is rejected");
    expect(verdict[1 * C + 2] == HTP_SEL_CLEAR_FLAG && verdict[0] == 0, "the verdicts");
    expect(orows[0] == rows[((size_t)1 * B + 0) * capr * HTP_TIMELINE_NCOL], "the winner's rows are copied");
    in.C = 9;
    expect(htp_hostsim_turn_select(&in, &out, msg, sizeof msg) == -1 && std::strstr(msg, "[select]"), "C out of range");
  }
  std::printf(failures ? "clear_asan: %d failure(s)\n" : "clear_asan: OK\n", failures);
  return failures ? 1 : 0;
}
