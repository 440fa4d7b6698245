// TEST-ONLY stand-alone program: the host build of the sampled pose search (sample_hostsim.cpp) over one small batch
// of each type and the bad-input cases, with exactly-sized heap buffers, meant to be built with
// -fsanitize=address,undefined -fno-sanitize-recover=all: any access beyond the parameter rows, the polygon pools, the
// x lists, the candidate tables, the outputs, the planner scratch or the Scene that stands for the kernel's LDS aborts
// it.  Exits 0 when every run returned what it must.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "sample_hostsim.cpp"

namespace {

struct Batch {
  std::vector<double> params, vertices, start_x, end_x;
  std::vector<int32_t> desc, poly_off{0}, n_start, n_end;
  int cap_s, cap_e, cap_cand, cap_samples;
  int batch = 0;

  Batch(int cs, int ce, int cc, int cap) : cap_s(cs), cap_e(ce), cap_cand(cc), cap_samples(cap) {}

  int rect(double x0, double x1, double y0, double y1) {   // counter-clockwise
    const double v[8] = {x0, y0, x1, y0, x1, y1, x0, y1};
    vertices.insert(vertices.end(), v, v + 8);
    poly_off.push_back((int32_t)(vertices.size() / 2));
    return (int)poly_off.size() - 2;
  }

  // four tree rows along x at y = 0, 3, 6, 9, a rectangular field around them, the tractor and one implement
  void turn(int type, int side, double sy, double ey, int ns, int ne, double x0, double dx, bool implement,
            bool blocked) {
    const int body = rect(-0.55, 2.85, -0.74, 0.74);
    const int aux = implement ? rect(-1.84, -0.74, -0.6, 0.5) : -1;
    const int b0 = (int)poly_off.size() - 1;
    for (int r = 0; r < 4; ++r) rect(0.0, 20.0, 3.0 * r - 0.15, 3.0 * r + 0.15);
    if (blocked) rect(-30.0, 0.0, ey - 1.0, ey + 1.0);   // laid over the whole entry side
    const int b1 = (int)poly_off.size() - 1;
    const int field = rect(-9.0, 29.0, -4.0, 13.0);
    const double near = 3.141592653589793;
    const double p[HTP_CT_NPARAM] = {(double)type, (double)side, x0, sy, side == 1 ? near : 0.0, x0, ey,
                                     side == 1 ? 0.0 : near, 1.9, 0.55, 1.9 / std::tan(0.55), 0.1};
    params.insert(params.end(), p, p + HTP_CT_NPARAM);
    const int32_t d[HTP_SMP_NDESC] = {body, aux, -1, b0, b1, field};
    desc.insert(desc.end(), d, d + HTP_SMP_NDESC);
    for (int i = 0; i < cap_s; ++i) start_x.push_back(x0 + dx * i);
    for (int j = 0; j < cap_e; ++j) end_x.push_back(x0 + dx * j);
    n_start.push_back(ns);
    n_end.push_back(ne);
    ++batch;
  }

  htp_classic_sample_in in() const {
    return htp_classic_sample_in{batch, (int32_t)poly_off.size() - 1, (int32_t)(vertices.size() / 2), params.data(),
                                 desc.data(), poly_off.data(), vertices.data(), start_x.data(), end_x.data(),
                                 n_start.data(), n_end.data(), cap_s, cap_e, cap_cand, cap_samples, 0};
  }
};

struct Out {
  std::vector<int32_t> status, winner, n_feasible, cand_status;
  std::vector<double> poses, score, cand_score;
  Out(int B, int cc)
      : status(B, -9), winner(2 * B, -9), n_feasible(B, -9), cand_status((size_t)B * cc, -9),
        poses((size_t)B * HTP_SMP_NPOSE), score(B), cand_score((size_t)B * cc) {}
  htp_classic_sample_result res(bool tables = true) {
    return htp_classic_sample_result{status.data(), winner.data(), poses.data(), score.data(), n_feasible.data(),
                                     tables ? cand_score.data() : nullptr, tables ? cand_status.data() : nullptr};
  }
};

int fails = 0;
void expect(bool ok, const char* what) {
  if (!ok) { std::printf("FAILED: %s\n", what); ++fails; }
}

}  // namespace

int main() {
  char msg[128];
  {   // one batch of each type, near side; the last Dubins turn has every candidate blocked
    Batch B(3, 3, 9, 1024);
    B.turn(HTP_SMP_DUBINS, 1, 1.5, 7.5, 3, 3, -1.0, -1.5, true, false);
    B.turn(HTP_SMP_REEDS_SHEPP, 1, 1.5, 4.5, 2, 3, -1.0, -1.5, true, false);
    B.turn(HTP_SMP_CIRCLE_BACK, 1, 1.5, 4.5, 3, 1, -1.0, -1.5, false, false);
    B.turn(HTP_SMP_DUBINS, 1, 1.5, 7.5, 3, 3, -1.0, -1.5, false, true);
    B.turn(HTP_SMP_DUBINS, 2, 1.5, 7.5, 2, 2, 21.0, 1.5, true, false);   // far side
    htp_classic_sample_in in = B.in();
    Out O(B.batch, B.cap_cand);
    htp_classic_sample_result r = O.res();
    expect(htp_hostsim_classic_sample(&in, &r, msg, sizeof msg) == 0, "the batch of each type runs");
    for (int b = 0; b < B.batch; ++b)
      std::printf("turn %d: status %d winner (%d, %d) score %.6f feasible %d\n", b, O.status[b], O.winner[2 * b],
                  O.winner[2 * b + 1], O.score[b], O.n_feasible[b]);
    expect(O.status[0] == HTP_SMP_OK && O.n_feasible[0] > 0, "the Dubins turn has a winner");
    expect(O.status[1] == HTP_SMP_OK && O.n_feasible[1] > 0, "the Reeds-Shepp turn has a winner");
    expect(O.status[2] == HTP_SMP_OK && O.winner[5] == 0, "the circle-back turn has a winner");
    expect(O.status[3] == HTP_SMP_NONE_FEASIBLE && O.winner[6] == -1 && O.n_feasible[3] == 0, "a blocked entry: none feasible");
    expect(O.status[4] == HTP_SMP_OK, "the far-side Dubins turn has a winner");
    expect(O.cand_status[1 * 9 + 6] == HTP_SMP_C_UNUSED, "slots past n_start * n_end are unused");
    // the same without the tables: the same winners
    Out Q(B.batch, B.cap_cand);
    htp_classic_sample_result q = Q.res(false);
    expect(htp_hostsim_classic_sample(&in, &q, msg, sizeof msg) == 0, "the batch runs without the tables");
    expect(Q.winner == O.winner && Q.status == O.status, "the tables do not change the winners");
  }
  {   // bad input, turn by turn; the healthy turn between them is left intact
    Batch B(3, 3, 6, 1024);
    B.turn(HTP_SMP_DUBINS, 1, 1.5, 7.5, 2, 2, -1.0, -1.5, false, false);   // 0 healthy
    B.turn(HTP_SMP_DUBINS, 1, 1.5, 7.5, 0, 2, -1.0, -1.5, false, false);   // 1 empty
    B.turn(HTP_SMP_DUBINS, 1, 1.5, 7.5, 3, 3, -1.0, -1.5, false, false);   // 2 nine candidates, six slots
    B.turn(HTP_SMP_DUBINS, 1, 1.5, 7.5, 2, 2, -1.0, -1.5, false, false);   // 3 NaN pose
    B.params[3 * HTP_CT_NPARAM + HTP_CT_P_SYAW] = std::nan("");
    B.turn(HTP_SMP_DUBINS, 1, 1.5, 7.5, 2, 2, -1.0, -1.5, false, false);   // 4 NaN sample
    B.start_x[4 * 3 + 1] = std::nan("");
    B.turn(HTP_SMP_CIRCLE_BACK, 1, 1.5, 4.5, 2, 2, -1.0, -1.5, false, false);   // 5 circle-back with n_end 2
    B.turn(HTP_SMP_DUBINS, 1, 1.5, 7.5, 4, 2, -1.0, -1.5, false, false);   // 6 n_start over cap_s
    B.turn(HTP_SMP_DUBINS, 1, 1.5, 7.5, 2, 2, -1.0, -1.5, false, false);   // 7 healthy
    htp_classic_sample_in in = B.in();
    Out O(B.batch, B.cap_cand);
    htp_classic_sample_result r = O.res();
    expect(htp_hostsim_classic_sample(&in, &r, msg, sizeof msg) == 0, "the bad-input batch runs");
    const int want[8] = {HTP_SMP_OK, HTP_SMP_BAD_INPUT, HTP_SMP_OVERFLOW, HTP_SMP_BAD_INPUT, HTP_SMP_OK,
                         HTP_SMP_BAD_INPUT, HTP_SMP_BAD_INPUT, HTP_SMP_OK};
    for (int b = 0; b < 8; ++b) {
      std::printf("bad-input turn %d: status %d\n", b, O.status[b]);
      expect(O.status[b] == want[b], "bad-input status");
    }
    expect(O.cand_status[4 * 6 + 2] == HTP_SMP_C_BAD_INPUT && O.cand_status[4 * 6 + 0] != HTP_SMP_C_BAD_INPUT,
           "a NaN sample spoils its own candidates only");
    expect(O.winner[0] == O.winner[14] && O.winner[1] == O.winner[15] && O.score[0] == O.score[7],
           "the healthy turns agree");
    // a path longer than cap_samples: a status, not a loop
    in.cap_samples = 16;
    expect(htp_hostsim_classic_sample(&in, &r, msg, sizeof msg) == 0, "the short-scratch batch runs");
    expect(O.status[0] == HTP_SMP_OVERFLOW && O.cand_status[0] == HTP_SMP_C_OVERFLOW, "cap_samples too small: overflow");
    // argument errors
    in.cap_samples = 8;
    expect(htp_hostsim_classic_sample(&in, &r, msg, sizeof msg) == -1, "cap_samples below 16 is refused");
    in = B.in();
    in.cap_cand = 0;
    expect(htp_hostsim_classic_sample(&in, &r, msg, sizeof msg) == -1, "cap_cand 0 is refused");
    in = B.in();
    in.start_x = nullptr;
    expect(htp_hostsim_classic_sample(&in, &r, msg, sizeof msg) == -1, "a null input is refused");
    in = B.in();
    r.status = nullptr;
    expect(htp_hostsim_classic_sample(&in, &r, msg, sizeof msg) == -1, "a null output is refused");
    r = O.res();
    r.cand_score = nullptr;
    expect(htp_hostsim_classic_sample(&in, &r, msg, sizeof msg) == -1, "half a pair of tables is refused");
    expect(htp_hostsim_classic_sample(nullptr, &r, msg, sizeof msg) == -1, "a null batch is refused");
    r = O.res();
    B.desc[HTP_SMP_D_FIELD] = 1000;
    in = B.in();
    expect(htp_hostsim_classic_sample(&in, &r, msg, sizeof msg) == -1, "a polygon id out of range is refused");
  }
  {   // a circle-back turn whose step makes an arc of 6e9 samples: judged as a double, an overflow, never converted
    Batch B(3, 1, 3, 64);
    B.turn(HTP_SMP_CIRCLE_BACK, 1, 1.5, 4.5, 3, 1, -1.0, -1.5, false, false);
    B.turn(HTP_SMP_CIRCLE_BACK, 1, 1.5, 4.5, 3, 1, -1.0, -1.5, false, false);
    B.params[1 * HTP_CT_NPARAM + HTP_CT_P_STEP] = 1e-9;
    htp_classic_sample_in in = B.in();
    Out O(B.batch, B.cap_cand);
    htp_classic_sample_result r = O.res();
    expect(htp_hostsim_classic_sample(&in, &r, msg, sizeof msg) == 0, "the tiny-step batch runs");
    std::printf("tiny step: status %d, candidates %d %d %d\n", O.status[1], O.cand_status[3], O.cand_status[4],
                O.cand_status[5]);
    expect(O.status[1] == HTP_SMP_OVERFLOW, "a step of 1e-9: overflow");
    for (int k = 0; k < 3; ++k) expect(O.cand_status[3 + k] == HTP_SMP_C_OVERFLOW, "a step of 1e-9: candidate overflow");
  }
  std::printf(fails ? "%d check(s) failed\n" : "all checks passed\n", fails);
  return fails ? 1 : 0;
}
