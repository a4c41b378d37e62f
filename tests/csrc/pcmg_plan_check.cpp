// Host check of the multigrid planner (macroc_amd/csrc/pcmg_plan.h): the functions pcmg.cpp plans the
// distributed hierarchy with (option pc_mg_dist), run stand-alone (no GPU, no library), so it can be
// built with -fsanitize=address,undefined (the Makefile's pcmg-plan-check; tests/test_pcmg_dist_cpu.py).
//   usage: pcmg_plan_check                      the built-in cases
//          pcmg_plan_check NX NY NZ m n p [levels]   one case, its boxes printed
// Checks, for every case and level:
//   1. the ranks' boxes tile the level exactly (per axis: contiguous, in rank order, no gap, no overlap);
//   2. a rank's coarse range is the set of coarse nodes sitting on its fine nodes (f(I) = min(2 I, N - 1));
//   3. every coarse node P needs for an owned fine node, and every fine node P^T gathers for an owned
//      coarse node, lies in the owned range or one node beside it (one ghost layer suffices);
//   4. every rank plans the same number of levels with the same global sizes, and refuses alike.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../macroc_amd/csrc/pcmg_plan.h"

using namespace mcx;

static int fails = 0;
#define CHECK(c, ...)                          \
  do {                                         \
    if (!(c)) {                                \
      if (fails++ < 20) {                      \
        std::fprintf(stderr, "FAIL %s: ", #c); \
        std::fprintf(stderr, __VA_ARGS__);     \
        std::fprintf(stderr, "\n");            \
      }                                        \
    }                                          \
  } while (0)

// fine node of coarse node I on an axis of N nodes
static int fine_of(int N, int I) { return N <= 2 ? I : (2 * I < N - 1 ? 2 * I : N - 1); }

// returns the plan's code (0 / 2) after checking it on every rank
static int check_case(const int N0[3], const int mnp[3], int levels, bool print, std::string* msg) {
  const int nr = mnp[0] * mnp[1] * mnp[2];
  std::vector<PcmgPlan> P(nr);
  int code = -1;
  for (int r = 0; r < nr; r++) {
    std::string err;
    const int rc = pcmg_plan_checked(N0, mnp, r, levels, &P[r], &err);
    if (r == 0) {
      code = rc;
      if (msg) *msg = err;
    }
    CHECK(rc == code, "rank %d returns %d, rank 0 %d", r, rc, code);
    if (msg) CHECK(err == *msg, "rank %d: another message: %s", r, err.c_str());
  }
  if (code) return code;
  const int nl = P[0].nlev;
  for (int r = 0; r < nr; r++) {
    CHECK(P[r].nlev == nl, "rank %d plans %d levels, rank 0 %d", r, P[r].nlev, nl);
    for (int l = 0; l < nl; l++)
      for (int a = 0; a < 3; a++) CHECK(P[r].N[l][a] == P[0].N[l][a], "rank %d level %d axis %d: global size", r, l, a);
  }
  const int stride[3] = {1, mnp[0], mnp[0] * mnp[1]};
  for (int l = 0; l < nl; l++)
    for (int a = 0; a < 3; a++) {
      const int N = P[0].N[l][a];
      int next = 0;
      for (int q = 0; q < mnp[a]; q++) {  // the column's box, from any rank in it
        const PcmgPlan& R = P[q * stride[a]];
        CHECK(R.s[l][a] == next && R.n[l][a] >= 1, "level %d axis %d column %d: start %d count %d, expected start %d", l, a,
              q, R.s[l][a], R.n[l][a], next);
        next = R.s[l][a] + R.n[l][a];
        for (int r = 0; r < nr; r++) {  // every rank of the column agrees
          const int col = a == 0 ? r % mnp[0] : a == 1 ? (r / mnp[0]) % mnp[1] : r / (mnp[0] * mnp[1]);
          if (col == q) CHECK(P[r].s[l][a] == R.s[l][a] && P[r].n[l][a] == R.n[l][a], "rank %d level %d axis %d", r, l, a);
        }
        if (l + 1 == nl) continue;
        const PcmgPlan& C = R;
        const int Nc = P[0].N[l + 1][a], cs = C.s[l + 1][a], cn = C.n[l + 1][a], s = R.s[l][a], n = R.n[l][a];
        CHECK(Nc == pcmg_coarse_count(N), "level %d axis %d: %d coarse nodes of %d", l, a, Nc, N);
        for (int I = 0; I < Nc; I++) {  // 2. ownership follows the fine node
          const int f = fine_of(N, I);
          const bool mine = f >= s && f < s + n, planned = I >= cs && I < cs + cn;
          CHECK(mine == planned, "level %d axis %d column %d: coarse %d on fine %d", l, a, q, I, f);
        }
        if (N <= 2) continue;
        std::vector<int> pos(N, -1);
        for (int I = 0; I < Nc; I++) pos[fine_of(N, I)] = I;
        for (int f = 0; f < N; f++) {  // 3. one ghost layer
          const int p0 = pos[f] >= 0 ? pos[f] : pos[f - 1], p1 = pos[f] >= 0 ? pos[f] : pos[f + 1];
          if (f >= s && f < s + n) CHECK(p0 >= cs - 1 && p1 <= cs + cn, "P: level %d axis %d column %d fine %d", l, a, q, f);
          for (int I : {p0, p1})
            if (I >= cs && I < cs + cn) CHECK(f >= s - 1 && f <= s + n, "P^T: level %d axis %d column %d coarse %d fine %d", l, a, q, I, f);
        }
      }
      CHECK(next == N, "level %d axis %d: the boxes end at %d of %d", l, a, next, N);
    }
  if (print) {
    std::printf("%d levels\n", nl);
    for (int l = 0; l < nl; l++) {
      std::printf("level %d: %d x %d x %d\n", l, P[0].N[l][0], P[0].N[l][1], P[0].N[l][2]);
      for (int r = 0; r < nr; r++)
        std::printf("  rank %d: start %d %d %d count %d %d %d\n", r, P[r].s[l][0], P[r].s[l][1], P[r].s[l][2], P[r].n[l][0],
                    P[r].n[l][1], P[r].n[l][2]);
    }
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 7) {
    const int N0[3] = {std::atoi(argv[1]), std::atoi(argv[2]), std::atoi(argv[3])};
    const int mnp[3] = {std::atoi(argv[4]), std::atoi(argv[5]), std::atoi(argv[6])};
    std::string msg;
    const int rc = check_case(N0, mnp, argc > 7 ? std::atoi(argv[7]) : 0, true, &msg);
    if (rc) std::printf("refused (%d): %s\n", rc, msg.c_str());
    std::printf("%d failures\n", fails);
    return fails ? 1 : rc;
  }
  // x split of the issue's axis cases (y = z = 9 on one rank each), 2 x 2 x 2 on 16^3, the early stop,
  // the headline's 512^3 over 2 x 2 x 2, thin ranks
  static const int cases[][6] = {{17, 9, 9, 2, 1, 1},  {16, 9, 9, 2, 1, 1},  {24, 9, 9, 3, 1, 1},   {33, 9, 9, 4, 1, 1},
                                 {13, 9, 9, 2, 1, 1},  {20, 9, 9, 3, 1, 1},  {9, 9, 9, 2, 1, 1},    {40, 9, 9, 2, 1, 1},
                                 {10, 9, 9, 2, 1, 1},  {8, 9, 9, 2, 1, 1},   {16, 16, 16, 2, 2, 2}, {24, 9, 40, 3, 1, 1},
                                 {24, 9, 13, 3, 1, 2}, {12, 10, 12, 2, 1, 2}, {512, 512, 512, 2, 2, 2}, {5, 9, 9, 3, 1, 1},
                                 {12, 9, 9, 4, 1, 1},  {40, 3, 40, 4, 1, 2}};
  for (const auto& k : cases) {
    const int rc = check_case(k, k + 3, 0, false, nullptr);
    CHECK(rc == 0, "%d x %d x %d over %d x %d x %d: automatic levels refused (%d)", k[0], k[1], k[2], k[3], k[4], k[5], rc);
  }
  {  // automatic early stop: 4 levels ending at (4, 2, 6); one rank: 5
    const int N0[3] = {24, 9, 40}, m3[3] = {3, 1, 1}, m1[3] = {1, 1, 1};
    PcmgPlan P;
    CHECK(pcmg_plan_checked(N0, m3, 1, 0, &P, nullptr) == 0 && P.nlev == 4 && P.N[3][0] == 4 && P.N[3][1] == 2 &&
              P.N[3][2] == 6, "24 x 9 x 40 over 3: %d levels", P.nlev);
    CHECK(pcmg_plan_checked(N0, m1, 0, 0, &P, nullptr) == 0 && P.nlev == 5, "24 x 9 x 40 on one rank: %d levels", P.nlev);
  }
  {  // a fixed count that reaches a level with an empty rank: code 2 on every rank, naming axis and rank
    const int N0[3] = {12, 9, 9}, mnp[3] = {4, 1, 1};
    std::string msg;
    CHECK(check_case(N0, mnp, 4, false, &msg) == 2, "12 x 9 x 9 over 4 with 4 levels: accepted");
    CHECK(msg.find("axis x") != std::string::npos && msg.find("rank 1") != std::string::npos &&
              msg.find("level 3") != std::string::npos, "message: %s", msg.c_str());
    CHECK(check_case(N0, mnp, 3, false, nullptr) == 0, "12 x 9 x 9 over 4 with 3 levels: refused");
  }
  {  // the coarsest level too large, and a grid that cannot coarsen
    const int N0[3] = {33, 33, 33}, m1[3] = {1, 1, 1}, N2[3] = {2, 2, 2};
    std::string msg;
    CHECK(check_case(N0, m1, 2, false, &msg) == 2 && msg.find("3 levels fit") != std::string::npos, "message: %s", msg.c_str());
    CHECK(check_case(N2, m1, 0, false, nullptr) == 2, "2 x 2 x 2: accepted");
    PcmgPlan P;
    const int bad[3] = {3, 1, 1};
    CHECK(pcmg_plan(N2, bad, 0, 0, &P, &msg) == 2, "more ranks than nodes: accepted");
    CHECK(pcmg_plan(N0, m1, 5, 0, &P, &msg) == 2, "rank outside the grid: accepted");
  }
  std::printf("%d failures\n", fails);
  return fails ? 1 : 0;
}
