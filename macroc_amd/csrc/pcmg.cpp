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

// coarse node count of an axis with N nodes: the even indices, plus the last node when N - 1 is odd
static int coarse_count(int N) { return N <= 2 ? N : (N - 1) / 2 + 1 + ((N - 1) & 1); }

// level sizes.  levels 0: stop once every axis has <= 5 nodes; otherwise that many levels, or fewer
// when nothing coarsens any more.  Returns the dofs of the coarsest level.
int pcmg_dims(const Ctx& c, int levels, int* nlev, int n[][3]) {
  int cur[3] = {c.g.NX, c.g.NY, c.g.NZ}, L = 0;
  const int want = levels > 0 ? levels : PCMG_MAXLEV;
  while (true) {
    for (int a = 0; a < 3; a++) n[L][a] = cur[a];
    L++;
    if (L >= want) break;
    if (levels <= 0 && L >= 2 && cur[0] <= 5 && cur[1] <= 5 && cur[2] <= 5) break;
    int nxt[3];
    for (int a = 0; a < 3; a++) nxt[a] = coarse_count(cur[a]);
    if (nxt[0] == cur[0] && nxt[1] == cur[1] && nxt[2] == cur[2]) break;
    for (int a = 0; a < 3; a++) cur[a] = nxt[a];
  }
  *nlev = L;
  return 3 * n[L - 1][0] * n[L - 1][1] * n[L - 1][2];
}

// option check (pc_type 1 with the current pc_mg_levels): 0, or 2 with the reason
int pcmg_check(Ctx& c, int levels) {
  if (c.nranks > 1 || c.comm || c.lg) {
    set_error("pc_type mg: one rank only (this context is rank " + std::to_string(c.rank) + " of " +
              std::to_string(c.nranks) + "); use -pc_type jacobi");
    return 2;
  }
  int n[PCMG_MAXLEV][3], nl = 0;
  pcmg_dims(c, levels, &nl, n);
  const int64_t nc = 3 * (int64_t)n[nl - 1][0] * n[nl - 1][1] * n[nl - 1][2];
  if (nl < 2) {
    set_error("pc_type mg: the grid " + std::to_string(c.g.NX) + " x " + std::to_string(c.g.NY) + " x " +
              std::to_string(c.g.NZ) + " has no coarser level");
    return 2;
  }
  if (nc > PCMG_COARSE_MAX) {
    int fit = 0;
    for (int q = nl + 1; q <= PCMG_MAXLEV && !fit; q++) {
      int m[PCMG_MAXLEV][3], ml = 0;
      if (pcmg_dims(c, q, &ml, m) <= PCMG_COARSE_MAX) fit = ml;
    }
    set_error("pc_mg_levels " + std::to_string(levels) + ": the coarsest level " + std::to_string(n[nl - 1][0]) + " x " +
              std::to_string(n[nl - 1][1]) + " x " + std::to_string(n[nl - 1][2]) + " has " + std::to_string(nc) +
              " dofs, above the " + std::to_string(PCMG_COARSE_MAX) + " its dense inverse takes; " +
              (fit ? std::to_string(fit) + " levels fit" : std::string("no level count fits")) + " (0: automatic)");
    return 2;
  }
  return 0;
}

void pcmg_free(Ctx& c) {
  Pcmg& M = c.mg;
  if (c.stream) (void)hipStreamSynchronize(c.stream);
  for (int l = 0; l < PCMG_MAXLEV; l++) {
    PcmgLevel& v = M.L[l];
    if (v.x_base) (void)hipFree(v.x_base);
    else if (v.x) (void)hipFree(v.x);
    void* own[] = {v.A, v.mask};
    for (void* p : own)
      if (p) (void)hipFree(p);
    if (l > 0)
      for (void* p : {(void*)v.b, (void*)v.r, (void*)v.d, (void*)v.dinv})
        if (p) (void)hipFree(p);
    v = PcmgLevel();
  }
  if (M.ainv) (void)hipFree(M.ainv);
  c.device_bytes -= M.bytes;
  M = Pcmg();
}

template <class T>
static int mg_alloc(Ctx& c, T** p, int64_t n) {
  MCX_HIP(hipMalloc((void**)p, sizeof(T) * (size_t)n));
  MCX_HIP(hipMemsetAsync(*p, 0, sizeof(T) * (size_t)n, c.stream));
  c.mg.bytes += (int64_t)sizeof(T) * n;
  return 0;
}

static int pcmg_alloc(Ctx& c) {
  Pcmg& M = c.mg;
  if (M.alloc) return 0;
  int rc = pcmg_check(c, c.pc_mg_levels);
  if (rc) return rc;
  int n[PCMG_MAXLEV][3];
  pcmg_dims(c, c.pc_mg_levels, &M.nlev, n);
  M.bytes = 0;
  M.alloc = true;  // pcmg_free releases whatever a failed allocation leaves
  for (int l = 0; l < M.nlev; l++) {
    PcmgLevel& v = M.L[l];
    for (int a = 0; a < 3; a++) v.n[a] = n[l][a];
    v.nn = (int64_t)n[l][0] * n[l][1] * n[l][2];
    if ((rc = mg_alloc(c, &v.mask, v.nn))) return rc;
    if (l == 0) {  // the iterate in the padded box (the SpMV's input), aligned as u and p are
      const int64_t npad = (int64_t)c.g.PX * c.g.PY * c.g.PZ * 3;
      char* base = nullptr;
      if ((rc = mg_alloc(c, &base, (int64_t)sizeof(double) * npad + 256))) return rc;
      v.x_base = base;
      v.x = reinterpret_cast<double*>(base + c.pad_off);
      v.r = c.w;
      v.d = c.z;
      v.dinv = c.dinv;
      launch_pcmg_mask0(c, v.mask);
    } else if ((rc = mg_alloc(c, &v.A, 243 * v.nn)) || (rc = mg_alloc(c, &v.x, 3 * v.nn)) ||
               (rc = mg_alloc(c, &v.b, 3 * v.nn)) || (rc = mg_alloc(c, &v.r, 3 * v.nn)) ||
               (rc = mg_alloc(c, &v.d, 3 * v.nn)) || (rc = mg_alloc(c, &v.dinv, 3 * v.nn))) {
      return rc;
    }
  }
  M.nc = (int)(3 * M.L[M.nlev - 1].nn);
  if ((rc = mg_alloc(c, &M.ainv, (int64_t)M.nc * M.nc))) return rc;
  c.device_bytes += M.bytes;
  return 0;
}

static PcmgXfer xfer(const Pcmg& M, int l) {
  PcmgXfer t;
  for (int a = 0; a < 3; a++) {
    t.fn[a] = M.L[l].n[a];
    t.cn[a] = M.L[l + 1].n[a];
  }
  return t;
}
static PcmgLay lay_of(const Ctx& c, int l) { return l == 0 ? pcmg_lay_pad(c) : pcmg_lay_nat(c.mg.L[l].n); }

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

// level l's operator on its iterate: r = b - A x (b null: A x) in v.r
static void apply_level(Ctx& c, int l, const double* b) {
  PcmgLevel& v = c.mg.L[l];
  if (l == 0) launch_spmv(c, v.x, v.r, false, false);  // v.r = A x; the callers subtract
  else launch_pcmg_spmv(c, v, v.x, b, v.r);
}

// dense inverse of the coarsest operator: Cholesky A = L L^T on the host, then A^-1 = L^-T L^-1
static int coarse_inverse(Ctx& c) {
  Pcmg& M = c.mg;
  const PcmgLevel& v = M.L[M.nlev - 1];
  const int n = M.nc;
  const int64_t nn = v.nn;
  std::vector<double> blk((size_t)243 * nn), A((size_t)n * n, 0.);
  MCX_HIP(hipMemcpyAsync(blk.data(), v.A, sizeof(double) * blk.size(), hipMemcpyDeviceToHost, c.stream));
  MCX_HIP(hipStreamSynchronize(c.stream));
  for (int64_t p = 0; p < nn; p++) {
    const int i = (int)(p % v.n[0]), j = (int)((p / v.n[0]) % v.n[1]), k = (int)(p / ((int64_t)v.n[0] * v.n[1]));
    for (int nb = 0; nb < 27; nb++) {
      const int ii = i + nb % 3 - 1, jj = j + (nb / 3) % 3 - 1, kk = k + nb / 9 - 1;
      if (ii < 0 || jj < 0 || kk < 0 || ii >= v.n[0] || jj >= v.n[1] || kk >= v.n[2]) continue;
      const int64_t q = ii + (int64_t)v.n[0] * (jj + (int64_t)v.n[1] * kk);
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
  int rc = pcmg_alloc(c);
  if (rc) {
    const std::string e = mcx_last_error();
    if (M.alloc) {
      c.device_bytes += M.bytes;  // pcmg_free subtracts what was counted: a failed allocation counted nothing yet
      pcmg_free(c);
    }
    set_error(e);
    return rc;
  }
  if (M.built) return 0;
  launch_jacobi(c);  // the fine level's D^-1
  // Galerkin operators A_{l+1} = P^T A_l P by probing: 27 colours x 3 components
  for (int l = 0; l + 1 < M.nlev; l++) {
    PcmgLevel &f = M.L[l], &k = M.L[l + 1];
    const PcmgXfer t = xfer(M, l);
    const PcmgLay lx = lay_of(c, l);
    MCX_HIP(hipMemsetAsync(k.A, 0, sizeof(double) * 243 * k.nn, c.stream));
    for (int colour = 0; colour < 27; colour++) {
      if (colour % 3 >= k.n[0] || (colour / 3) % 3 >= k.n[1] || colour / 9 >= k.n[2]) continue;  // no node has it
      for (int d = 0; d < 3; d++) {
        launch_pcmg_prolong(c, t, lx, nullptr, colour * 3 + d, f.mask, f.x, false);
        apply_level(c, l, nullptr);
        launch_pcmg_restrict(c, t, f.r, nullptr, f.mask, k.b);
        launch_pcmg_scatter(c, k, k.b, colour, d);
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
      apply_level(c, l, nullptr);
      launch_pcmg_scale_dot(c, v.nn, v.dinv, v.r, v.d);
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
static void smooth(Ctx& c, int l, const double* b, bool xzero) {
  PcmgLevel& v = c.mg.L[l];
  const PcmgLay lx = lay_of(c, l);
  const double emin = .1 * v.lmax, emax = 1.1 * v.lmax;
  const double scale = 2. / (emax + emin), alpha = 1. - scale * emin, mu = 1. / alpha, omegaprod = 2. / alpha;
  double ckm1 = 1., ck = mu;
  for (int s = 0; s < c.pc_mg_smooth; s++) {
    const bool skip = xzero && s == 0;  // x = 0: the residual is b
    if (!skip) apply_level(c, l, b);
    // level 0: v.r = A x, the kernel subtracts; coarser levels: v.r = b - A x already
    const double* rb = skip || l == 0 ? b : v.r;
    const double* rw = !skip && l == 0 ? v.r : nullptr;
    if (s == 0) {
      launch_pcmg_cheb(c, lx, v.nn, rb, rw, v.dinv, v.d, v.x, 0., scale, true, xzero);
    } else {
      const double ckp1 = 2. * mu * ck - ckm1, omega = omegaprod * ck / ckp1;
      launch_pcmg_cheb(c, lx, v.nn, rb, rw, v.dinv, v.d, v.x, omega - 1., omega * scale, false, false);
      ckm1 = ck;
      ck = ckp1;
    }
  }
}

static void cycle(Ctx& c, int l, const double* b) {
  Pcmg& M = c.mg;
  PcmgLevel& v = M.L[l];
  if (l == M.nlev - 1) {
    launch_pcmg_gemv(c, M.nc, M.ainv, b, v.x);
    return;
  }
  smooth(c, l, b, true);
  apply_level(c, l, b);
  const PcmgXfer t = xfer(M, l);
  if (l == 0) launch_pcmg_restrict(c, t, b, v.r, v.mask, M.L[1].b);
  else launch_pcmg_restrict(c, t, v.r, nullptr, v.mask, M.L[l + 1].b);
  cycle(c, l + 1, M.L[l + 1].b);
  launch_pcmg_prolong(c, t, lay_of(c, l), M.L[l + 1].x, -1, v.mask, v.x, true);
  smooth(c, l, b, false);
}

int pcmg_apply(Ctx& c, const double* r_owned) {
  int rc = pcmg_ensure(c);
  if (rc) return rc;
  cycle(c, 0, r_owned);
  return 0;
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
  double* z = c.mg.L[0].x;
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
  cycle(c, 0, c.r);
  launch_pcmg_dot(c, lp, g.nown, z, c.r);
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
    launch_spmv(c, c.p_pad, c.w, false, false);
    launch_pcmg_dot(c, lp, g.nown, c.p_pad, c.w);
    dpiold = dpi;
    if ((rc = read_red(c, 1, &dpi))) return rc;
    betaold = beta;
    if (dpi == 0. || (i > 0 && dpi * dpiold <= 0.) || std::isnan(dpi)) {
      reason = std::isnan(dpi) ? MCX_KSP_DIVERGED_NANORINF : MCX_KSP_DIVERGED_INDEFINITE_MAT;
      break;
    }
    const double a = beta / dpi;
    launch_pcmg_xr(c, lp, g.nown, a, c.p_pad, c.w, c.du, c.r);
    cycle(c, 0, c.r);
    launch_pcmg_dot(c, lp, g.nown, z, c.r);
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
