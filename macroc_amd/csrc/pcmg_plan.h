// pcmg_plan.h — -pc_type mg: the level sizes and, on a decomposed grid, every rank's owned box per
// level.  Host-only integers, no HIP: pcmg.cpp plans with these functions, and
// tests/csrc/pcmg_plan_check.cpp runs them stand-alone under AddressSanitizer + UBSan.
//
// The rule.  An axis of N > 2 nodes keeps its even nodes and, when N - 1 is odd, its last node:
// coarse node I sits on fine node f(I) = min(2 I, N - 1).  The owner of a coarse node is the owner of
// the fine node it sits on; the fine ranges are the DMDA's (width N / P + (N % P > r)).  Every rank's
// coarse range is contiguous, and P and P^T reach at most one node beyond the owned ranges, so one
// ghost layer per level is enough.  A rank can run out of nodes on an axis at a deep level: automatic
// levels stop before such a level, a fixed level count that reaches one is refused.  Every rank
// decides all of this from the grid and the rank grid alone: no communication.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

namespace mcx {

constexpr int PCMG_MAXLEV = 16;
constexpr int PCMG_COARSE_MAX = 3072;  // dofs of the coarsest level (its inverse is dense)

struct PcmgPlan {
  int nlev = 0;
  int N[PCMG_MAXLEV][3];  // global node counts
  int s[PCMG_MAXLEV][3];  // the rank's owned box: global start ...
  int n[PCMG_MAXLEV][3];  // ... and count
};

// coarse node count of an axis with N nodes: the even indices, plus the last node when N - 1 is odd
inline int pcmg_coarse_count(int N) { return N <= 2 ? N : (N - 1) / 2 + 1 + ((N - 1) & 1); }

// coarse nodes of an axis of N nodes that sit on a fine node below t (0 <= t <= N)
inline int pcmg_coarse_below(int N, int t) {
  if (N <= 2) return t;
  if (t >= N) return pcmg_coarse_count(N);
  return (t + 1) / 2;  // the even nodes below t; the last node N - 1 is not below t <= N - 1
}

// levels 0: automatic (stop once every axis has <= 5 nodes, or before a level that leaves a rank
// column without a node); otherwise that many levels, or fewer when nothing coarsens any more.
// mnp: the rank grid; rank = pi + m (pj + n pk).  Returns 0, or 2 with the reason in *err.
inline int pcmg_plan(const int N0[3], const int mnp[3], int rank, int levels, PcmgPlan* P, std::string* err) {
  static const char* const axis = "xyz";
  for (int a = 0; a < 3; a++)
    if (N0[a] < 1 || mnp[a] < 1 || mnp[a] > N0[a]) {
      if (err) *err = std::string("pc_type mg: bad grid or rank grid on axis ") + axis[a];
      return 2;
    }
  if (rank < 0 || rank >= mnp[0] * mnp[1] * mnp[2]) {
    if (err) *err = "pc_type mg: rank " + std::to_string(rank) + " outside the rank grid";
    return 2;
  }
  const int col[3] = {rank % mnp[0], (rank / mnp[0]) % mnp[1], rank / (mnp[0] * mnp[1])};
  const int stride[3] = {1, mnp[0], mnp[0] * mnp[1]};
  // every rank column's range per axis (all of them: an empty column anywhere stops every rank alike)
  std::vector<int> s[3], n[3];
  int cur[3];
  for (int a = 0; a < 3; a++) {
    cur[a] = N0[a];
    s[a].resize(mnp[a]);
    n[a].resize(mnp[a]);
    int acc = 0;
    for (int q = 0; q < mnp[a]; q++) {
      n[a][q] = N0[a] / mnp[a] + ((N0[a] % mnp[a]) > q);
      s[a][q] = acc;
      acc += n[a][q];
    }
  }
  const int want = levels > 0 ? levels : PCMG_MAXLEV;
  int L = 0;
  while (true) {
    for (int a = 0; a < 3; a++) {
      P->N[L][a] = cur[a];
      P->s[L][a] = s[a][col[a]];
      P->n[L][a] = n[a][col[a]];
    }
    L++;
    if (L >= want || L >= PCMG_MAXLEV) break;
    if (levels <= 0 && L >= 2 && cur[0] <= 5 && cur[1] <= 5 && cur[2] <= 5) break;
    int nxt[3];
    for (int a = 0; a < 3; a++) nxt[a] = pcmg_coarse_count(cur[a]);
    if (nxt[0] == cur[0] && nxt[1] == cur[1] && nxt[2] == cur[2]) break;
    std::vector<int> cs[3], cn[3];
    int empty_axis = -1, empty_col = -1;
    for (int a = 0; a < 3; a++) {
      cs[a].resize(mnp[a]);
      cn[a].resize(mnp[a]);
      for (int q = 0; q < mnp[a]; q++) {
        const int lo = pcmg_coarse_below(cur[a], s[a][q]), hi = pcmg_coarse_below(cur[a], s[a][q] + n[a][q]);
        cs[a][q] = lo;
        cn[a][q] = hi - lo;
        if (hi <= lo && empty_axis < 0) {
          empty_axis = a;
          empty_col = q;
        }
      }
    }
    if (empty_axis >= 0) {
      if (levels <= 0) break;  // automatic: this level is the coarsest
      if (err)
        *err = "pc_mg_levels " + std::to_string(levels) + ": level " + std::to_string(L) + " (" +
               std::to_string(nxt[0]) + " x " + std::to_string(nxt[1]) + " x " + std::to_string(nxt[2]) +
               ") leaves rank " + std::to_string(empty_col * stride[empty_axis]) + " without a node on axis " +
               axis[empty_axis] + " (" + std::to_string(L) + " levels fit this decomposition; 0: automatic)";
      return 2;
    }
    for (int a = 0; a < 3; a++) {
      cur[a] = nxt[a];
      s[a].swap(cs[a]);
      n[a].swap(cn[a]);
    }
  }
  P->nlev = L;
  return 0;
}

// the plan with the option's checks: a coarser level exists, the coarsest one fits its dense inverse
inline int pcmg_plan_checked(const int N0[3], const int mnp[3], int rank, int levels, PcmgPlan* P, std::string* err) {
  int rc = pcmg_plan(N0, mnp, rank, levels, P, err);
  if (rc) return rc;
  const int nl = P->nlev;
  const int64_t nc = 3 * (int64_t)P->N[nl - 1][0] * P->N[nl - 1][1] * P->N[nl - 1][2];
  if (nl < 2) {
    if (err)
      *err = "pc_type mg: the grid " + std::to_string(N0[0]) + " x " + std::to_string(N0[1]) + " x " +
             std::to_string(N0[2]) + " has no coarser level";
    return 2;
  }
  if (nc > PCMG_COARSE_MAX) {
    int fit = 0;
    for (int q = nl + 1; q <= PCMG_MAXLEV && !fit; q++) {
      PcmgPlan Q;
      if (pcmg_plan(N0, mnp, rank, q, &Q, nullptr)) break;
      if (3 * (int64_t)Q.N[Q.nlev - 1][0] * Q.N[Q.nlev - 1][1] * Q.N[Q.nlev - 1][2] <= PCMG_COARSE_MAX) fit = Q.nlev;
    }
    if (err)
      *err = "pc_mg_levels " + std::to_string(levels) + ": the coarsest level " + std::to_string(P->N[nl - 1][0]) +
             " x " + std::to_string(P->N[nl - 1][1]) + " x " + std::to_string(P->N[nl - 1][2]) + " has " +
             std::to_string(nc) + " dofs, above the " + std::to_string(PCMG_COARSE_MAX) +
             " its dense inverse takes; " + (fit ? std::to_string(fit) + " levels fit" : std::string("no level count fits")) +
             " (0: automatic)";
    return 2;
  }
  return 0;
}

}  // namespace mcx
