// pcmg.cpp — -pc_type mg: the geometric multigrid preconditioner of the macro CG.
// Host side only: the level sizes, the Galerkin operators by probing, the eigenvalue estimates, the
// coarsest level's dense inverse, the V-cycle and the PCG loop around it.  Every kernel is in
// kernels.hip (launch_pcmg_*).
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "mcx_internal.h"

namespace mcx {

bool pcmg_dist(const Ctx& c) { return c.pc_mg_dist && (c.nranks > 1 || c.comm || c.lg); }

// the context's plan: one rank (or pc_mg_dist off) the whole grid, else the rank's box per level
int pcmg_plan_ctx(const Ctx& c, int levels, PcmgPlan* P) {
  const int N0[3] = {c.g.NX, c.g.NY, c.g.NZ};
  const bool d = pcmg_dist(c);
  const int mnp[3] = {d ? c.m : 1, d ? c.n : 1, d ? c.p : 1};
  std::string err;
  const int rc = pcmg_plan_checked(N0, mnp, d ? c.rank : 0, levels, P, &err);
  if (rc) set_error(err);
  return rc;
}

// the global level sizes.  levels 0: stop once every axis has <= 5 nodes (pc_mg_dist: or before a level
// that leaves a rank without a node); otherwise that many levels, or fewer when nothing coarsens any
// more.  Returns the dofs of the coarsest level.
int pcmg_dims(const Ctx& c, int levels, int* nlev, int n[][3]) {
  const int N0[3] = {c.g.NX, c.g.NY, c.g.NZ};
  const bool d = pcmg_dist(c);
  const int mnp[3] = {d ? c.m : 1, d ? c.n : 1, d ? c.p : 1};
  PcmgPlan P;
  if (pcmg_plan(N0, mnp, d ? c.rank : 0, levels, &P, nullptr)) {  // refused level count: the fine level alone
    P.nlev = 1;
    for (int a = 0; a < 3; a++) P.N[0][a] = N0[a];
  }
  for (int l = 0; l < P.nlev; l++)
    for (int a = 0; a < 3; a++) n[l][a] = P.N[l][a];
  *nlev = P.nlev;
  return 3 * n[P.nlev - 1][0] * n[P.nlev - 1][1] * n[P.nlev - 1][2];
}

// option check (pc_type 1 with the current pc_mg_levels): 0, or 2 with the reason
int pcmg_check(Ctx& c, int levels) {
  if ((c.nranks > 1 || c.comm || c.lg) && !c.pc_mg_dist) {
    set_error("pc_type mg: one rank only (this context is rank " + std::to_string(c.rank) + " of " +
              std::to_string(c.nranks) + "); use -pc_type jacobi, or set pc_mg_dist 1 first (-pc_mg_dist 1: the "
              "distributed hierarchy)");
    return 2;
  }
  PcmgPlan P;
  return pcmg_plan_ctx(c, levels, &P);
}

void pcmg_free(Ctx& c) {
  Pcmg& M = c.mg;
  // in-process transport: a neighbour's stream may still copy from this rank's send buffers or sum its arin
  if (M.dist && c.lg) (void)hipDeviceSynchronize();
  if (c.stream) (void)hipStreamSynchronize(c.stream);
  if (c.comm_stream) (void)hipStreamSynchronize(c.comm_stream);
  for (int l = 0; l < PCMG_MAXLEV; l++) {
    PcmgLevel& v = M.L[l];
    if (v.x_base) (void)hipFree(v.x_base);
    else if (v.x) (void)hipFree(v.x.p);
    if (v.rp_base) (void)hipFree(v.rp_base);
    else if (v.rp) (void)hipFree(v.rp.p);
    void* own[] = {v.A.p, v.mask};
    for (void* p : own)
      if (p) (void)hipFree(p);
    if (l > 0)
      for (void* p : {v.b.p, v.r.p, v.d.p, v.dinv.p})
        if (p) (void)hipFree(p);
    free_halo_plan(v.halo);
    v = PcmgLevel();
  }
  for (void* p : {(void*)M.ainv, (void*)M.arin, (void*)M.arout, (void*)M.xfull, (void*)M.d_ar_ptrs})
    if (p) (void)hipFree(p);
  c.device_bytes -= M.bytes;
  M = Pcmg();
}

template <class T>
static int mg_alloc(Ctx& c, T** p, int64_t n) {
  MCX_HIP(hipMalloc((void**)p, sizeof(T) * (size_t)n));
  MCX_HIP(hipMemsetAsync(*p, 0, sizeof(T) * (size_t)n, c.stream));
  c.mg.bytes += (int64_t)sizeof(T) * n;  // counted at once: pcmg_free subtracts what a failed allocation got
  c.device_bytes += (int64_t)sizeof(T) * n;
  return 0;
}

// a vector or an operator of a level: n values of the storage type, which the vector carries from here on
static int mg_alloc_v(Ctx& c, PcmgVec* v, int64_t n, bool f32) {
  float* p4 = nullptr;
  double* p8 = nullptr;
  const int rc = f32 ? mg_alloc(c, &p4, n) : mg_alloc(c, &p8, n);
  *v = f32 ? PcmgVec(p4) : PcmgVec(p8);
  return rc;
}
static size_t esz(const PcmgLevel& v) { return v.f32 ? sizeof(float) : sizeof(double); }

static int pcmg_alloc(Ctx& c) {
  Pcmg& M = c.mg;
  if (M.alloc) return 0;
  PcmgPlan P;
  int rc = pcmg_check(c, c.pc_mg_levels);
  if (rc || (rc = pcmg_plan_ctx(c, c.pc_mg_levels, &P))) return rc;
  M.nlev = P.nlev;
  M.dist = pcmg_dist(c);
  M.bytes = 0;
  M.alloc = true;  // pcmg_free releases whatever a failed allocation leaves
  for (int l = 0; l < M.nlev; l++) {
    PcmgLevel& v = M.L[l];
    for (int a = 0; a < 3; a++) {
      v.n[a] = P.n[l][a];
      v.s[a] = P.s[l][a];
      v.N[a] = P.N[l][a];
    }
    v.nn = (int64_t)v.n[0] * v.n[1] * v.n[2];
    v.f32 = c.pc_mg_precision == 1 && l > 0;
    if ((rc = mg_alloc(c, &v.mask, v.nn))) return rc;
    if (l == 0) {  // the iterate in the padded box (the SpMV's input), aligned as u and p are
      const int64_t npad = (int64_t)c.g.PX * c.g.PY * c.g.PZ * 3;
      char* base = nullptr;
      if ((rc = mg_alloc(c, &base, (int64_t)sizeof(double) * npad + 256))) return rc;
      v.x_base = base;
      v.x = reinterpret_cast<double*>(base + c.pad_off);
      if (M.dist) {
        if ((rc = mg_alloc(c, &base, (int64_t)sizeof(double) * npad + 256))) return rc;
        v.rp_base = base;
        v.rp = reinterpret_cast<double*>(base + c.pad_off);
      }
      v.r = c.w;
      v.d = c.z;
      v.dinv = c.dinv;
      launch_pcmg_mask0(c, v.mask);
    } else {
      const int64_t nbox = M.dist ? (int64_t)(v.n[0] + 2) * (v.n[1] + 2) * (v.n[2] + 2) : v.nn;
      if ((rc = mg_alloc_v(c, &v.A, 243 * v.nn, v.f32)) || (rc = mg_alloc_v(c, &v.x, 3 * nbox, v.f32)) ||
          (rc = mg_alloc_v(c, &v.b, 3 * v.nn, v.f32)) || (rc = mg_alloc_v(c, &v.r, 3 * v.nn, v.f32)) ||
          (rc = mg_alloc_v(c, &v.d, 3 * v.nn, v.f32)) || (rc = mg_alloc_v(c, &v.dinv, 3 * v.nn, v.f32)))
        return rc;
      if (M.dist) {
        if ((rc = mg_alloc_v(c, &v.rp, 3 * nbox, v.f32))) return rc;
        v.halo.level = l;
        v.halo.esz = (int)esz(v);
        int64_t hb = 0;
        rc = build_halo_plan(c, v.halo, v.n, v.n[0] + 2, (v.n[0] + 2) * (v.n[1] + 2), &hb);
        M.bytes += hb;
        c.device_bytes += hb;
        if (rc) return rc;
      }
    }
  }
  const PcmgLevel& last = M.L[M.nlev - 1];
  const int64_t NN = (int64_t)last.N[0] * last.N[1] * last.N[2];
  M.nc = (int)(3 * NN);
  if ((rc = mg_alloc(c, &M.ainv, (int64_t)M.nc * M.nc))) return rc;
  if (M.dist) {
    M.ar_cap = 243 * NN;
    if ((rc = mg_alloc(c, &M.arin, M.ar_cap)) || (rc = mg_alloc(c, &M.arout, M.ar_cap)) ||
        (rc = mg_alloc(c, &M.xfull, (int64_t)M.nc)))
      return rc;
    if (c.lg && (rc = mg_alloc(c, &M.d_ar_ptrs, (int64_t)c.lg->nranks))) return rc;
  }
  return 0;
}

static PcmgXfer xfer(const Pcmg& M, int l) {
  PcmgXfer t;
  for (int a = 0; a < 3; a++) {
    t.fn[a] = M.L[l].n[a];
    t.cn[a] = M.L[l + 1].n[a];
    t.fs[a] = M.L[l].s[a];
    t.cs[a] = M.L[l + 1].s[a];
    t.FN[a] = M.L[l].N[a];
    t.CN[a] = M.L[l + 1].N[a];
  }
  return t;
}
// the layout of level l's iterate (and, pc_mg_dist, of its masked residual): padded wherever ghosts are read
static PcmgLay lay_of(const Ctx& c, int l) {
  if (l == 0) return pcmg_lay_pad(c);
  return c.mg.dist ? pcmg_lay_box(c.mg.L[l]) : pcmg_lay_nat(c.mg.L[l].n);
}
// owned order of level l's box
static PcmgLay lay_own(const Ctx& c, int l) {
  const PcmgLevel& v = c.mg.L[l];
  PcmgLay y = pcmg_lay_nat(v.n);
  for (int a = 0; a < 3; a++) {
    y.gs[a] = v.s[a];
    y.gn[a] = v.N[a];
  }
  return y;
}

// c.red[0 .. n) on the host, after a bounded wait (the stream may hold collectives)
static int read_red(Ctx& c, int n, double* out) {
  double* h = reinterpret_cast<double*>(c.h_cg);
  MCX_HIP(hipMemcpyAsync(h, c.red, sizeof(double) * n, hipMemcpyDeviceToHost, c.stream));
  MCX_HIP(hipEventRecord(c.ev_chunk[0], c.stream));
  int rc = comm_wait(c, c.ev_chunk[0], "multigrid scalar readback");
  if (rc) return rc;
  for (int q = 0; q < n; q++) out[q] = h[q];
  return 0;
}

// pc_mg_dist: fill the ghosts of a padded vector of level l
static int ghosts(Ctx& c, int l, PcmgVec xpad) {
  if (!c.mg.dist) return 0;
  if (l == 0) return halo_exchange(c, c.halo, xpad.as<double>());
  HaloPlan& h = c.mg.L[l].halo;  // its buffers have the level's storage type
  return halo_exchange(c, h, h.esz == 4 ? (void*)xpad.as<float>() : (void*)xpad.as<double>());
}

// level l's operator on its iterate: r = b - A x (b null: A x) in v.r
static int apply_level(Ctx& c, int l, PcmgVec b) {
  PcmgLevel& v = c.mg.L[l];
  if (int rc = ghosts(c, l, v.x)) return rc;
  if (l == 0)  // v.r = A x; the callers subtract
    launch_spmv(c, v.x.as<double>(), v.r.as<double>(), false, false);
  else launch_pcmg_spmv(c, v, lay_of(c, l), v.x, b, v.r);
  return 0;
}

// L[l + 1].b = P^T (b - w) with level l's Dirichlet dofs masked (w null: P^T b).  pc_mg_dist: the owner
// masks the residual into the padded box, one exchange fills its ghosts, P^T reads them
static int restrict_level(Ctx& c, int l, PcmgVec b, PcmgVec w) {
  Pcmg& M = c.mg;
  PcmgLevel& v = M.L[l];
  const PcmgXfer t = xfer(M, l);
  if (!M.dist) {
    launch_pcmg_restrict(c, t, lay_own(c, l), b, w, v.mask, M.L[l + 1].b);
    return 0;
  }
  const PcmgLay lp = lay_of(c, l);
  launch_pcmg_resid(c, lp, v.nn, b, w, v.mask, v.rp);
  if (int rc = ghosts(c, l, v.rp)) return rc;
  launch_pcmg_restrict(c, t, lp, v.rp, nullptr, nullptr, M.L[l + 1].b);
  return 0;
}

// pc_mg_dist: something that can fail on one rank alone, agreed before the next collective: every
// rank learns whether any rank failed (one all-reduced maximum)
static int agree(Ctx& c, int rc, const char* what) {
  const std::string e = rc ? std::string(mcx_last_error()) : std::string();
  int r2 = allreduce_prepare(c);
  if (r2) return r2;
  const double flag = rc ? 1. : 0.;
  MCX_HIP(hipMemcpyAsync(c.red_loc, &flag, sizeof(double), hipMemcpyHostToDevice, c.stream));
  MCX_HIP(hipStreamSynchronize(c.stream));  // flag is a stack variable
  if ((r2 = allreduce_max(c, c.red_loc, c.red, 1))) return r2;
  double any = 0.;
  if ((r2 = read_red(c, 1, &any))) return r2;
  if (rc) {
    set_error(e);
    return rc;
  }
  if (any != 0.) {
    set_error(std::string("pc_type mg: ") + what + " failed on another rank");
    return 27;
  }
  return 0;
}

// dense inverse of the coarsest operator: Cholesky A = L L^T on the host, then A^-1 = L^-T L^-1.
// pc_mg_dist: every rank contributes its owned blocks, one all-reduce gives every rank the whole
// operator, and every rank factors it alike
static int coarse_inverse(Ctx& c) {
  Pcmg& M = c.mg;
  const PcmgLevel& v = M.L[M.nlev - 1];
  const int n = M.nc;
  const int64_t nn = (int64_t)v.N[0] * v.N[1] * v.N[2];
  std::vector<double> blk((size_t)243 * nn), A((size_t)n * n, 0.);
  if (M.dist) {
    int rc = allreduce_prepare(c);
    if (rc) return rc;
    MCX_HIP(hipMemsetAsync(M.arin, 0, sizeof(double) * 243 * nn, c.stream));
    launch_pcmg_blocks_to_full(c, v, lay_own(c, M.nlev - 1), nn, M.arin);
    if ((rc = allreduce_sum_mg(c, M.arout, (int)(243 * nn)))) return rc;
    MCX_HIP(hipMemcpyAsync(blk.data(), M.arout, sizeof(double) * blk.size(), hipMemcpyDeviceToHost, c.stream));
    MCX_HIP(hipEventRecord(c.ev_chunk[0], c.stream));
    if ((rc = comm_wait(c, c.ev_chunk[0], "multigrid coarsest operator (all-reduced blocks)"))) return rc;
    MCX_HIP(hipStreamSynchronize(c.stream));
  } else if (v.f32) {  // the float blocks, widened on the host
    std::vector<float> blk32(blk.size());
    MCX_HIP(hipMemcpyAsync(blk32.data(), v.A.as<float>(), sizeof(float) * blk32.size(), hipMemcpyDeviceToHost, c.stream));
    MCX_HIP(hipStreamSynchronize(c.stream));
    for (size_t q = 0; q < blk.size(); q++) blk[q] = blk32[q];
  } else {
    MCX_HIP(hipMemcpyAsync(blk.data(), v.A.as<double>(), sizeof(double) * blk.size(), hipMemcpyDeviceToHost, c.stream));
    MCX_HIP(hipStreamSynchronize(c.stream));
  }
  for (int64_t p = 0; p < nn; p++) {
    const int i = (int)(p % v.N[0]), j = (int)((p / v.N[0]) % v.N[1]), k = (int)(p / ((int64_t)v.N[0] * v.N[1]));
    for (int nb = 0; nb < 27; nb++) {
      const int ii = i + nb % 3 - 1, jj = j + (nb / 3) % 3 - 1, kk = k + nb / 9 - 1;
      if (ii < 0 || jj < 0 || kk < 0 || ii >= v.N[0] || jj >= v.N[1] || kk >= v.N[2]) continue;
      const int64_t q = ii + (int64_t)v.N[0] * (jj + (int64_t)v.N[1] * kk);
      for (int r = 0; r < 3; r++)
        for (int cc = 0; cc < 3; cc++) A[(size_t)(3 * p + r) * n + 3 * q + cc] = blk[(size_t)(nb * 9 + r * 3 + cc) * nn + p];
    }
  }
  // the probed operator is symmetric up to rounding: factor its symmetric part
  for (int r = 0; r < n; r++)
    for (int cc = 0; cc < r; cc++) A[(size_t)r * n + cc] = A[(size_t)cc * n + r] = .5 * (A[(size_t)r * n + cc] + A[(size_t)cc * n + r]);
  for (int j = 0; j < n; j++) {  // A's lower triangle <- L, row by row
    for (int k = 0; k <= j; k++) {
      double s = A[(size_t)j * n + k];
      const double *rj = &A[(size_t)j * n], *rk = &A[(size_t)k * n];
      for (int q = 0; q < k; q++) s -= rj[q] * rk[q];
      if (k < j) {
        A[(size_t)j * n + k] = s / rk[k];
      } else {
        if (!(s > 0.)) {
          set_error("pc_type mg: the coarsest operator is not positive definite (pivot " + std::to_string(j) + ")");
          return 31;
        }
        A[(size_t)j * n + j] = std::sqrt(s);
      }
    }
  }
  // W = L^-1 (lower), stored by rows; then Ainv = W^T W
  std::vector<double> W((size_t)n * n, 0.);
  for (int i = 0; i < n; i++) {  // row i of W: W[i][j] = (delta_ij - sum_{k<i} L[i][k] W[k][j]) / L[i][i]
    double* wi = &W[(size_t)i * n];
    const double* li = &A[(size_t)i * n];
    for (int k = 0; k < i; k++) {
      const double lik = li[k];
      if (lik == 0.) continue;
      const double* wk = &W[(size_t)k * n];
      for (int j = 0; j <= k; j++) wi[j] -= lik * wk[j];
    }
    wi[i] += 1.;
    const double inv = 1. / li[i];
    for (int j = 0; j <= i; j++) wi[j] *= inv;
  }
  std::vector<double> Ai((size_t)n * n, 0.);
  for (int k = 0; k < n; k++) {  // Ainv += W[k]^T W[k] (row k has entries 0 .. k)
    const double* wk = &W[(size_t)k * n];
    for (int i = 0; i <= k; i++) {
      const double a = wk[i];
      if (a == 0.) continue;
      double* ai = &Ai[(size_t)i * n];
      for (int j = 0; j <= i; j++) ai[j] += a * wk[j];
    }
  }
  for (int i = 0; i < n; i++)
    for (int j = 0; j < i; j++) Ai[(size_t)j * n + i] = Ai[(size_t)i * n + j];
  MCX_HIP(hipMemcpyAsync(M.ainv, Ai.data(), sizeof(double) * Ai.size(), hipMemcpyHostToDevice, c.stream));
  MCX_HIP(hipStreamSynchronize(c.stream));
  return 0;
}

int pcmg_ensure(Ctx& c) {
  Pcmg& M = c.mg;
  const bool fresh = !M.alloc;
  int rc = pcmg_alloc(c);
  if (fresh && pcmg_dist(c) && (!rc || M.alloc)) {
    // every member has allocated its hierarchy (or failed to) before anyone exchanges with it, and
    // every rank learns of a failure before the first collective of the set-up
    if (c.lg) {
      const std::string e = rc ? std::string(mcx_last_error()) : std::string();
      if (int r2 = group_barrier(c.lg, c.rank, BAR_MG_ALLOC, c.comm_timeout)) return r2;
      if (rc) set_error(e);
    }
    rc = agree(c, rc, "the allocation of the hierarchy");
    if (!rc && c.lg) {
      std::vector<double*> ptrs(c.lg->nranks);
      for (int q = 0; q < c.lg->nranks; q++) ptrs[q] = c.lg->members[q]->mg.arin;
      MCX_HIP(hipMemcpy(M.d_ar_ptrs, ptrs.data(), sizeof(double*) * ptrs.size(), hipMemcpyHostToDevice));
    }
  }
  if (rc) {
    const std::string e = mcx_last_error();
    if (M.alloc) pcmg_free(c);
    set_error(e);
    return rc;
  }
  if (M.built) return 0;
  launch_jacobi(c);  // the fine level's D^-1
  // Galerkin operators A_{l+1} = P^T A_l P by probing: 27 colours x 3 components
  for (int l = 0; l + 1 < M.nlev; l++) {
    PcmgLevel &f = M.L[l], &k = M.L[l + 1];
    const PcmgXfer t = xfer(M, l);
    const PcmgLay lx = lay_of(c, l), lc = lay_of(c, l + 1);
    MCX_HIP(hipMemsetAsync(k.A.p, 0, esz(k) * 243 * k.nn, c.stream));
    for (int colour = 0; colour < 27; colour++) {
      if (colour % 3 >= k.N[0] || (colour / 3) % 3 >= k.N[1] || colour / 9 >= k.N[2]) continue;  // no node has it
      for (int d = 0; d < 3; d++) {
        launch_pcmg_prolong(c, t, lx, lc, nullptr, colour * 3 + d, f.mask, f.x, false);
        if ((rc = apply_level(c, l, nullptr)) || (rc = restrict_level(c, l, f.r, nullptr))) return rc;
        launch_pcmg_scatter(c, k, lay_own(c, l + 1), k.b, colour, d);
      }
    }
    launch_pcmg_diag(c, k);
  }
  // largest eigenvalue of D^-1 A on every smoothed level: 10 power iterations from a fixed start
  for (int l = 0; l + 1 < M.nlev; l++) {
    PcmgLevel& v = M.L[l];
    const PcmgLay lx = lay_of(c, l);
    launch_pcmg_seed(c, lx, v.nn, v.x);
    double nrm = 0.;
    for (int it = 0; it < 10; it++) {
      if ((rc = apply_level(c, l, nullptr)) || (rc = launch_pcmg_scale_dot(c, v.nn, v.dinv, v.r, v.d)))
        return rc;
      double s = 0.;
      if ((rc = read_red(c, 1, &s))) return rc;
      nrm = std::sqrt(s);
      if (!(nrm > 0.) || !std::isfinite(nrm)) {
        set_error("pc_type mg: the eigenvalue estimate of level " + std::to_string(l) + " failed (|D^-1 A v| = " +
                  std::to_string(nrm) + ")");
        return 32;
      }
      launch_pcmg_scaleto(c, lx, v.nn, v.d, 1. / nrm, v.x);
    }
    v.lmax = nrm;  // |D^-1 A v| with |v| = 1
  }
  M.L[M.nlev - 1].lmax = 0.;
  if ((rc = coarse_inverse(c))) return rc;
  MCX_HIP(hipGetLastError());
  M.built = true;
  return 0;
}

// Chebyshev of degree k on D^-1 A over [0.1, 1.1] lmax (the recurrence of PETSc's KSPCHEBYSHEV,
// written for the increment d = x_new - x)
static int smooth(Ctx& c, int l, PcmgVec b, bool xzero) {
  PcmgLevel& v = c.mg.L[l];
  const PcmgLay lx = lay_of(c, l);
  const double emin = .1 * v.lmax, emax = 1.1 * v.lmax;
  const double scale = 2. / (emax + emin), alpha = 1. - scale * emin, mu = 1. / alpha, omegaprod = 2. / alpha;
  double ckm1 = 1., ck = mu;
  for (int s = 0; s < c.pc_mg_smooth; s++) {
    const bool skip = xzero && s == 0;  // x = 0: the residual is b
    if (!skip)
      if (int rc = apply_level(c, l, b)) return rc;
    // level 0: v.r = A x, the kernel subtracts; coarser levels: v.r = b - A x already
    const PcmgVec rb = skip || l == 0 ? b : v.r;
    const PcmgVec rw = !skip && l == 0 ? v.r : PcmgVec();
    if (s == 0) {
      launch_pcmg_cheb(c, lx, v.nn, rb, rw, v.dinv, v.d, v.x, 0., scale, true, xzero);
    } else {
      const double ckp1 = 2. * mu * ck - ckm1, omega = omegaprod * ck / ckp1;
      launch_pcmg_cheb(c, lx, v.nn, rb, rw, v.dinv, v.d, v.x, omega - 1., omega * scale, false, false);
      ckm1 = ck;
      ck = ckp1;
    }
  }
  return 0;
}

// One V-cycle.  pc_mg_dist adds, per smoothed level, one ghost fill before every operator
// application, one of the masked residual before P^T and one of the coarse correction before P; the
// coarsest level is one all-reduce of its right-hand side, the dense product on every rank, and each
// rank's box of the result, ghosts included
static int cycle(Ctx& c, int l, PcmgVec b) {
  Pcmg& M = c.mg;
  PcmgLevel& v = M.L[l];
  int rc = 0;
  if (l == M.nlev - 1) {
    if (!M.dist) {
      launch_pcmg_gemv(c, M.nc, M.ainv, b, v.x);
      return 0;
    }
    if ((rc = allreduce_prepare(c))) return rc;  // every rank has summed the previous arin
    MCX_HIP(hipMemsetAsync(M.arin, 0, sizeof(double) * M.nc, c.stream));
    launch_pcmg_to_full(c, lay_own(c, l), v.nn, b, M.arin);
    if ((rc = allreduce_sum_mg(c, M.arout, M.nc))) return rc;
    launch_pcmg_gemv(c, M.nc, M.ainv, M.arout, M.xfull);
    launch_pcmg_from_full(c, lay_of(c, l), M.xfull, v.x);
    return 0;
  }
  if ((rc = smooth(c, l, b, true)) || (rc = apply_level(c, l, b))) return rc;
  const PcmgXfer t = xfer(M, l);
  if ((rc = l == 0 ? restrict_level(c, l, b, v.r) : restrict_level(c, l, v.r, nullptr))) return rc;
  if ((rc = cycle(c, l + 1, M.L[l + 1].b))) return rc;
  if (l + 1 < M.nlev - 1 && (rc = ghosts(c, l + 1, M.L[l + 1].x))) return rc;  // the coarsest level left its ghosts
  launch_pcmg_prolong(c, t, lay_of(c, l), lay_of(c, l + 1), M.L[l + 1].x, -1, v.mask, v.x, true);
  return smooth(c, l, b, false);
}

int pcmg_apply(Ctx& c, const double* r_owned) {
  int rc = pcmg_ensure(c);
  if (rc) return rc;
  return cycle(c, 0, r_owned);
}

// PCG around the V-cycle: KSPSolve_CG's steps and reasons with the norm sqrt(r . z), the two
// scalars of an iteration read back by the host (two waits per iteration)
int pcmg_solve(Ctx& c, int* its_out, double* rnorm, int* reason_out) {
  int rc = pcmg_ensure(c);
  if (rc) return rc;
  c.fusep_used = c.pdb_used = c.pqb_used = c.xs_used = false;
  c.t.spmv_launches = 0;
  c.t.spmv_ms_total = 0.;
  const Geo& g = c.g;
  const int64_t nown3 = 3 * (int64_t)g.nown, npad3 = (int64_t)g.PX * g.PY * g.PZ * 3;
  const PcmgLay lp = pcmg_lay_pad(c);
  double* z = c.mg.L[0].x.as<double>();
  const double rtol = c.o.ksp_rtol, abstol = c.o.ksp_abstol, dtol = c.o.ksp_dtol;
  const int maxits = c.o.ksp_max_it;
  std::vector<double> hist;
  auto converged = [&](double rn, double ttol, double rnorm0) -> int {
    if (std::isnan(rn) || std::isinf(rn)) return MCX_KSP_DIVERGED_NANORINF;
    if (rn <= ttol) return rn < abstol ? MCX_KSP_CONVERGED_ATOL : MCX_KSP_CONVERGED_RTOL;
    if (rn >= dtol * rnorm0) return MCX_KSP_DIVERGED_DTOL;
    return 0;
  };
  MCX_HIP(hipMemsetAsync(c.du, 0, sizeof(double) * nown3, c.stream));
  MCX_HIP(hipMemcpyAsync(c.r, c.b, sizeof(double) * nown3, hipMemcpyDeviceToDevice, c.stream));
  if ((rc = cycle(c, 0, c.r)) || (rc = launch_pcmg_dot(c, lp, g.nown, z, c.r))) return rc;
  double beta = 0., betaold = 0., dpi = 0., dpiold = 0.;
  if ((rc = read_red(c, 1, &beta))) return rc;
  double dp = std::sqrt(beta);
  hist.push_back(dp);
  const double rnorm0 = dp, ttol = std::fmax(rtol * dp, abstol);
  int i = 0, its = 0;
  int reason = beta < 0. ? MCX_KSP_DIVERGED_INDEFINITE_PC : converged(dp, ttol, rnorm0);
  while (!reason) {
    its = i + 1;
    if (beta == 0.) {
      reason = MCX_KSP_CONVERGED_ATOL;
      break;
    }
    if (i > 0 && beta * betaold < 0.) {
      reason = MCX_KSP_DIVERGED_INDEFINITE_PC;
      break;
    }
    launch_pcmg_aypx(c, npad3, z, i > 0 ? beta / betaold : 0., c.p_pad, i == 0);
    if (c.mg.dist && (rc = halo_exchange(c, c.p_pad))) return rc;  // z's ghosts are stale: p's are filled here
    launch_spmv(c, c.p_pad, c.w, false, false);
    if ((rc = launch_pcmg_dot(c, lp, g.nown, c.p_pad, c.w))) return rc;
    dpiold = dpi;
    if ((rc = read_red(c, 1, &dpi))) return rc;
    betaold = beta;
    if (dpi == 0. || (i > 0 && dpi * dpiold <= 0.) || std::isnan(dpi)) {
      reason = std::isnan(dpi) ? MCX_KSP_DIVERGED_NANORINF : MCX_KSP_DIVERGED_INDEFINITE_MAT;
      break;
    }
    const double a = beta / dpi;
    launch_pcmg_xr(c, lp, g.nown, a, c.p_pad, c.w, c.du, c.r);
    if ((rc = cycle(c, 0, c.r)) || (rc = launch_pcmg_dot(c, lp, g.nown, z, c.r))) return rc;
    if ((rc = read_red(c, 1, &beta))) return rc;
    if (beta < 0.) {
      reason = MCX_KSP_DIVERGED_INDEFINITE_PC;
      break;
    }
    dp = std::sqrt(beta);
    hist.push_back(dp);
    if ((reason = converged(dp, ttol, rnorm0))) break;
    i++;
    if (i >= maxits) {
      reason = MCX_KSP_DIVERGED_ITS;
      break;
    }
  }
  MCX_HIP(hipGetLastError());
  *its_out = its;
  *rnorm = dp;
  *reason_out = reason;
  c.last_its = its;
  if (c.o.ksp_monitor) c.last_hist = hist;
  return 0;
}

}  // namespace mcx
