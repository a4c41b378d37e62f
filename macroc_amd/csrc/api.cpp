// api.cpp — C-ABI (include/macroc_amd.h) of the MI355X MacroC Newton inner loop.
// Host control mirrors the reference driver (src/main.c:49-109); all numerics run in the
// HIP kernels of kernels.hip on the context's stream.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "mcx_internal.h"

namespace mcx {

static thread_local std::string g_err;
void set_error(const std::string& s) { g_err = s; }

int exc_return(const char* fn, const char* what) {
  try {
    g_err = std::string(fn) + ": internal exception: " + what;
  } catch (...) {
  }
  return MCX_EXC;
}

// MCX_TEST_THROW (a comma list of entry names) is read once, when the library is loaded: no
// getenv per call (not thread-safe against a concurrent setenv), nothing to do when it is unset
static const std::string g_test_throw = [] {
  const char* e = std::getenv("MCX_TEST_THROW");
  return e ? "," + std::string(e) + "," : std::string();
}();

void test_inject(const char* fn) {
  if (!g_test_throw.empty() && g_test_throw.find("," + std::string(fn) + ",") != std::string::npos)
    throw std::bad_alloc();
}

// padded node vectors (u, p and its buffers): the allocation is shifted by pad_off bytes so that
// with a 16-node row pitch (pad_align) every interior row's first owned node starts a 128-B line
// (DESIGN §3); the base pointers are kept for hipFree
static int dalloc_pad(Ctx& c, double** p, int64_t n) {
  char* base = nullptr;
  MCX_HIP(hipMalloc((void**)&base, sizeof(double) * n + 256));
  MCX_HIP(hipMemsetAsync(base, 0, sizeof(double) * n + 256, c.stream));
  c.pad_bases.push_back(base);
  c.device_bytes += (int64_t)sizeof(double) * n + 256;
  *p = reinterpret_cast<double*>(base + c.pad_off);
  return 0;
}

template <class T>
static int dalloc(Ctx& c, T** p, int64_t n) {
  if (n <= 0) n = 1;
  MCX_HIP(hipMalloc((void**)p, sizeof(T) * n));
  MCX_HIP(hipMemsetAsync(*p, 0, sizeof(T) * n, c.stream));
  c.device_bytes += (int64_t)sizeof(T) * n;
  return 0;
}

static void elastic_C(double E, double nu, double C[36]) {
  const double lam = E * nu / ((1. + nu) * (1. - 2. * nu));
  const double mu = E / (2. * (1. + nu));
  for (int q = 0; q < 36; q++) C[q] = 0.;
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) C[a * 6 + b] = lam + (a == b ? 2. * mu : 0.);
  for (int a = 3; a < 6; a++) C[a * 6 + a] = mu;
}

// laws that hand over a tangent per Gauss point (ctan, element matrices per element); the elastic
// law and the micro law (one homogenised tangent) have one tangent in the kernel argument
static bool gp_tangent_law(int law) {
  return law == MCX_LAW_PLASTIC || law == MCX_LAW_EXTERNAL || law == MCX_LAW_MICRO_NL;
}
// laws built on the two-phase micro cell (C_hom, ensure_micro)
static bool micro_law(int law) { return law == MCX_LAW_MICRO || law == MCX_LAW_MICRO_NL; }

// phase timer: an event pair on the compute stream, recorded without any host wait (the
// timed steps are not serialised by the instrumentation); mcx_get_timing resolves the last pair
enum { PH_STRAINS, PH_HOMOG, PH_RES, PH_JAC, PH_SOLVE, PH_UPDATE };
struct PhaseTimer {
  Ctx& c;
  int k;
  PhaseTimer(Ctx& cc, int kk) : c(cc), k(kk) {
    if (c.timing && c.ev_phase[k][0]) (void)hipEventRecord(c.ev_phase[k][0], c.stream);
  }
  ~PhaseTimer() {
    if (!c.timing || !c.ev_phase[k][1]) return;
    (void)hipEventRecord(c.ev_phase[k][1], c.stream);
    c.phase_rec[k] = true;
  }
};

static int free_ctx(Ctx* c) {
  if (!c) return 0;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->comm_stream) (void)hipStreamSynchronize(c->comm_stream);
  if (c->x_stream) (void)hipStreamSynchronize(c->x_stream);
  if (c->f_stream) (void)hipStreamSynchronize(c->f_stream);
  void* ptrs[] = {c->micro_out, c->micro_ws, c->micro_grid_ws, c->mnl_ws, c->mnl_ufield, c->mnl_conc, c->mnl_slot, c->mnl_list, c->mnl_cnt, c->mnl_its, c->mnl_rn, c->mnl_pool, c->mnl_warm_store, c->hist_old, c->hist_new, c->ftrial, c->b, c->du, c->r, c->z, c->w, c->jix, c->jdd, c->V, c->U, c->D, c->d_mask, c->vi_idx, c->wd, c->vi_dict, c->vi_keys, c->vi_slot, c->vi_ctl, c->vi_bdict, c->eps, c->sig, c->ctan, c->Ke,
                  c->vib_keys, c->vib_ctl, c->vib_pos, c->ke_uni, c->xdone, c->esc_node, c->esc_res, c->esc_slot, c->elem_plain, c->cref, c->vi_xslot,
                  c->vi_xlist, c->vi_xcnt, c->vi_exc, c->st_coef, c->st_ids, c->st_slot, c->st_list, c->st_cnt, c->st_mask,
                  c->partials, c->red, c->red_loc, c->cg, c->hist, c->tmp, c->halo.d_send_idx,
                  c->halo.d_recv_idx, c->halo.d_sendbuf, c->halo.d_recvbuf, c->halo.d_bnd};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  pcmg_free(*c);
  for (void* p : c->pad_bases) (void)hipFree(p);  // u and the p buffers (dalloc_pad)
  if (c->h_cg) (void)hipHostFree(c->h_cg);
  for (void* h : {(void*)c->h_vib_keys, (void*)c->h_vib_map, (void*)c->h_vib_dict})
    if (h) (void)hipHostFree(h);
  for (hipEvent_t e : c->ev_pool) (void)hipEventDestroy(e);
  if (c->ev_a) (void)hipEventDestroy(c->ev_a);
  if (c->ev_b) (void)hipEventDestroy(c->ev_b);
  for (auto& pr : c->ev_phase)
    for (hipEvent_t e : pr)
      if (e) (void)hipEventDestroy(e);
  for (int q = 0; q < 2; q++)
    if (c->ev_chunk[q]) (void)hipEventDestroy(c->ev_chunk[q]);
  comm_destroy(*c);
  if (c->ev_pack) (void)hipEventDestroy(c->ev_pack);
  if (c->ev_comm) (void)hipEventDestroy(c->ev_comm);
  if (c->comm_stream) (void)hipStreamDestroy(c->comm_stream);
  if (c->x_stream) (void)hipStreamDestroy(c->x_stream);
  if (c->f_stream) (void)hipStreamDestroy(c->f_stream);
  for (hipEvent_t e : {c->ev_xp, c->ev_xd[0], c->ev_xd[1], c->ev_fx, c->ev_fd})
    if (e) (void)hipEventDestroy(e);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
  return 0;
}

// largest SpMV grid over the selectable kernels (mcx_set_option may switch between them)
static int64_t max_spmv_blocks(Ctx& c) {
  const int keep = c.spmv_kernel, keep_fmt = c.fmt, keep_bits = c.vi_bits;
  int64_t m = 0;
  for (int f : {FMT_V, FMT_U, FMT_SPLIT, FMT_VI})
    for (int k = 0; k <= 11; k++)
      for (int bits : {4, 8}) {
        c.fmt = f;
        c.spmv_kernel = k;
        c.vi_bits = bits;
        m = std::max(m, spmv_grid_blocks(c));
      }
  c.spmv_kernel = keep;
  c.fmt = keep_fmt;
  c.vi_bits = keep_bits;
  return m;
}

static int init_ctx(Ctx& c, const mcx_opts* o, int rank, int nranks, const void* comm_id, LocalGroup* lg) {
  c.o = *o;
  c.lg = lg;
  c.rank = rank;
  c.nranks = nranks;
  c.comm_timeout = comm_timeout_default();
  if (const char* e = std::getenv("MCX_PAD_ALIGN")) c.pad_align = std::atoi(e);  // A/B of the padded layout
  int ndev = 0;
  MCX_HIP(hipGetDeviceCount(&ndev));
  if (ndev <= 0) {
    set_error("no HIP device visible");
    return 11;
  }
  c.device = lg ? lg->device : (o->device >= 0 ? o->device : rank % ndev);
  MCX_HIP(hipSetDevice(c.device));
  int rc = setup_decomposition(c);
  if (rc) return rc;
  if (lg && (rc = group_setup(c))) return rc;
  int ncu = 0;
  MCX_HIP(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, c.device));
  // z-marching tiles (sbaij and AIJ-split): one resident round of blocks, 256x4 phased tiles
  // where the subdomain is that wide — tools/spmv_ab.py sweeps, DESIGN.md §4
  c.ncu = std::max(ncu, 1);
  c.g.ncu = c.ncu;
  c.aij_split = o->mat_type == MCX_MAT_AIJ && o->mat_aij_split;
  c.aij_vi = o->mat_type == MCX_MAT_AIJ && o->mat_aij_vi;
  c.vi_fma = o->mat_vi_fma != 0;
  if (o->mat_type == MCX_MAT_SBAIJ) {
    // phased z-march 256x4 / 128x4 / 64x4 (128^3: 0.436 vs 0.502 ms for symz 128x2; 64^3:
    // 0.0555 vs 0.0625 ms for symz 64x4; profiles/old/r02_ab_sbaij{128,64}.log)
    c.spmv_kernel = c.g.nx >= 256 ? 11 : (c.g.nx >= 128 ? 7 : 8);
    c.fmt = FMT_U;
  }
  MCX_HIP(hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking));
  MCX_HIP(hipStreamCreateWithFlags(&c.comm_stream, hipStreamNonBlocking));
  MCX_HIP(hipEventCreateWithFlags(&c.ev_pack, hipEventDisableTiming));
  MCX_HIP(hipEventCreateWithFlags(&c.ev_comm, hipEventDisableTiming));
  MCX_HIP(hipEventCreate(&c.ev_a));
  MCX_HIP(hipEventCreate(&c.ev_b));
  for (auto& pr : c.ev_phase)
    for (hipEvent_t& e : pr) MCX_HIP(hipEventCreate(&e));
  for (int q = 0; q < 2; q++) MCX_HIP(hipEventCreateWithFlags(&c.ev_chunk[q], hipEventDisableTiming));
  if ((rc = comm_init(c, comm_id))) return rc;
  {
    const int n3[3] = {c.g.nx, c.g.ny, c.g.nz};
    if ((rc = build_halo_plan(c, c.halo, n3, c.g.PX, c.g.PX * c.g.PY, &c.device_bytes))) return rc;
  }
  if ((rc = upload_constants(c))) return rc;
  const Geo& g = c.g;
  const int64_t npad = (int64_t)g.PX * g.PY * g.PZ * 3, nown3 = 3 * (int64_t)g.nown, E = g.nelem;
  // matrix storage: AIJ blocks V only for -mat_aij_split 0 (the AIJ-split path allocates it
  // lazily if a correction is not exact, mcx_assembly_jac); U for sbaij and AIJ-split; the
  // AIJ-split corrections D are sized by build_split to the active slots
  // jdd [VI_MAX][3] and the Jacobi vector dinv behind it in one buffer: the block-indexed CG
  // kernels read an exception node's (jix 255) inverse diagonal at jdd + 3 VI_MAX + 3n
  if ((rc = dalloc_pad(c, &c.u_pad, npad)) || (rc = dalloc_pad(c, &c.p_pad, npad)) || (rc = dalloc(c, &c.b, nown3)) ||
      (rc = dalloc(c, &c.du, nown3)) || (rc = dalloc(c, &c.r, nown3)) || (rc = dalloc(c, &c.z, nown3)) ||
      (rc = dalloc(c, &c.w, nown3)) || (rc = dalloc(c, &c.jdd, 3 * VI_MAX + nown3)) ||
      (rc = dalloc(c, &c.jix, (int64_t)g.nown)) || (rc = dalloc(c, &c.tmp, nown3)) ||
      (c.o.mat_type == MCX_MAT_SBAIJ && (rc = dalloc(c, &c.U, c.npgroups * UPAIR * 128))) ||
      (c.o.mat_type == MCX_MAT_AIJ && !c.aij_split && (rc = dalloc(c, &c.V, c.ngroups * NPAIR * 128))) ||
      (rc = dalloc(c, &c.eps, 6 * 8 * E)) || (rc = dalloc(c, &c.sig, 6 * 8 * E)) ||
      (rc = dalloc(c, &c.partials, c.partials_cap = 6 * std::max(max_spmv_blocks(c), node_blocks(c)) + 64)) ||
      (rc = dalloc(c, &c.red, 16)) || (rc = dalloc(c, &c.red_loc, 16)) || (rc = dalloc(c, &c.cg, 2)) ||
      (rc = dalloc(c, &c.hist, (int64_t)o->ksp_max_it + 2)) || (rc = dalloc(c, &c.ke_uni, 576)) ||
      (rc = dalloc_pad(c, &c.p_pad2, npad)) || (rc = dalloc(c, &c.xdone, 1)))  // p's second buffer (cg_pdb, cg_fusep)
    return rc;
  c.dinv = c.jdd + 3 * VI_MAX;
  // per-GP tangent: only laws that hand one over (the isotropic elastic C is a kernel argument)
  c.partials2 = c.partials + c.partials_cap / 2;
  if (gp_tangent_law(o->mat_law) &&
      ((rc = dalloc(c, &c.ctan, 36 * 8 * E)) || (rc = dalloc(c, &c.Ke, (int64_t)576 * E))))
    return rc;
  if (o->mat_law == MCX_LAW_PLASTIC &&
      ((rc = dalloc(c, &c.hist_old, 7 * 8 * E)) || (rc = dalloc(c, &c.hist_new, 7 * 8 * E)) ||
       (rc = dalloc(c, &c.ftrial, 8 * E))))
    return rc;
  if (c.aij_split) MCX_HIP(hipMalloc(&c.d_mask, 16 * sizeof(unsigned)));
  MCX_HIP(hipHostMalloc((void**)&c.h_cg, sizeof(CgState) * 2, hipHostMallocDefault));
  std::memset(c.h_cg, 0, sizeof(CgState) * 2);
  if (o->micro_n != 2 && o->mat_law != MCX_LAW_EXTERNAL && !micro_law(o->mat_law) && rank == 0)
    std::fprintf(stderr,
                 "WARNING! -micro_n %d has no effect: the device Gauss-point laws have no micro-scale FE problem "
                 "(MicroPP's FE2 solver is out of scope); it sizes an external MicroPP (-mat_law external, "
                 "micropp_C_create3, src/init.c:210-213)\n",
                 o->micro_n);
  c.mat.law = o->mat_law;
  c.mat.E = o->micro_mat_1[0];
  c.mat.nu = o->micro_mat_1[1];
  c.mat.Sy = o->micro_mat_1[2];
  c.mat.Ka = o->micro_mat_1[3];
  elastic_C(c.mat.E, c.mat.nu, c.mat.C);
  if (micro_law(o->mat_law)) {  // C_hom replaces mat.C at its first use (ensure_micro)
    if ((rc = dalloc(c, &c.micro_out, 6 * MICRO_OUT))) return rc;
    c.micro.n = o->micro_n;
    c.micro.type = o->micro_type;
    c.micro.E[0] = o->micro_mat_1[0];
    c.micro.nu[0] = o->micro_mat_1[1];
    c.micro.E[1] = o->micro_mat_2[0];
    c.micro.nu[1] = o->micro_mat_2[1];
    c.micro.rtol = 1e-12;
    c.micro_dirty = true;
  }
  if (o->mat_law == MCX_LAW_MICRO_NL) {  // the pool itself waits for the first non-linear point
    // (the unit-strain fields and the concentration tensors follow the cell's size: ensure_micro)
    const int64_t ngp = 8 * E;
    if ((rc = dalloc(c, &c.ftrial, ngp)) || (rc = dalloc(c, &c.mnl_slot, ngp)) ||
        (rc = dalloc(c, &c.mnl_list, ngp)) || (rc = dalloc(c, &c.mnl_cnt, 4)) ||
        (rc = dalloc(c, &c.mnl_its, 4 * ngp)) || (rc = dalloc(c, &c.mnl_rn, 2 * ngp)))
      return rc;
    c.mnl_col_its.assign((size_t)(6 * ngp), 0);
    MCX_HIP(hipMemsetAsync(c.mnl_slot, 0xff, sizeof(int) * (ngp > 0 ? ngp : 1), c.stream));  // -1: no slot
    c.mnl_Sy[0] = o->micro_mat_1[2];
    c.mnl_Ka[0] = o->micro_mat_1[3];
    c.mnl_Sy[1] = o->micro_mat_2[2];
    c.mnl_Ka[1] = o->micro_mat_2[3];
  }
  c.nnz_local = count_nnz_rows(c, g.xs, g.ys, g.zs, g.nx, g.ny, g.nz);
  c.nnz_global = count_nnz_rows(c, 0, 0, 0, o->NX, o->NY, o->NZ);
  c.nupper_local = count_upper_values(c);
  MCX_HIP(hipStreamSynchronize(c.stream));
  if (lg) {
    lg->members[rank] = &c;
    MCX_HIP(hipMemcpy(lg->d_red_ptrs + rank, &c.red_loc, sizeof(double*), hipMemcpyHostToDevice));
    if ((rc = group_barrier(lg, rank, BAR_INIT, c.comm_timeout))) {
      lg->members[rank] = nullptr;
      return rc;
    }
  }
  return 0;
}

// ---------------------------------------------------------------- phases
static int cg_solve(Ctx& c, int* its, double* rnorm, int* reason) {
  launch_jacobi(c);  // PCSetUp_Jacobi happens inside KSPSolve in the reference
  c.fusep_used = false;  // set by cg_iteration when the p update runs inside the SpMV
  c.pdb_used = cg_pdb(c);
  c.pqb_used = c.pdb_used && c.cg_pdb == 4;
  c.xs_used = c.pqb_used && c.cg_xs;
  if (c.pqb_used && !c.p_pad3) {  // the quad-buffered p update's third and fourth buffers
    const int64_t npad = (int64_t)c.g.PX * c.g.PY * c.g.PZ * 3;
    int rc = 0;
    if ((rc = dalloc_pad(c, &c.p_pad3, npad)) || (rc = dalloc_pad(c, &c.p_pad4, npad))) return rc;
  }
  if (c.xs_used) {  // cg_xs: buffers 5-8, the side stream and its events (each made once; a setup
                    // that failed part-way completes at the next solve instead of running without them)
    const int64_t npad = (int64_t)c.g.PX * c.g.PY * c.g.PZ * 3;
    int rc = 0;
    for (int q = 0; q < 4; q++)
      if (!c.p_pad58[q] && (rc = dalloc_pad(c, &c.p_pad58[q], npad))) return rc;
    if (!c.x_stream) MCX_HIP(hipStreamCreateWithFlags(&c.x_stream, hipStreamNonBlocking));
    for (hipEvent_t* e : {&c.ev_xp, &c.ev_xd[0], &c.ev_xd[1]})
      if (!*e) MCX_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
  }
  if (c.pdb_used) MCX_HIP(hipMemsetAsync(c.xdone, 0, sizeof(int), c.stream));
  CgState s{};
  s.rtol = c.o.ksp_rtol;
  s.abstol = c.o.ksp_abstol;
  s.dtol = c.o.ksp_dtol;
  s.maxits = c.o.ksp_max_it;
  s.hist_on = c.o.ksp_monitor ? 1 : 0;
  s.xp = -1;
  c.h_cg[0] = s;
  MCX_HIP(hipMemcpyAsync(c.cg, &c.h_cg[0], sizeof(CgState), hipMemcpyHostToDevice, c.stream));
  launch_cg_init(c);
  int rc = cg_finish_init(c);
  if (rc) return rc;
  // spmv event pairs (timing mode): every 8th iteration (spread over the solve), at most kTimed
  const int kTimed = 512;
  if (c.timing && c.ev_pool.empty()) {
    c.ev_pool.resize(2 * kTimed);
    for (auto& e : c.ev_pool) MCX_HIP(hipEventCreate(&e));
  }
  // chunks of CH iterations; the host polls the previous chunk's CgState while the next chunk
  // runs (kernels of a converged solve return at once)
  const int CH = 8;
  int issued = 0, slot = 0, pending = -1, npairs = 0;
  std::vector<int> pair_it;
  const int cap = c.o.ksp_max_it + 4 * CH;
  while (true) {
    for (int q = 0; q < CH; q++, issued++) {
      hipEvent_t e0 = nullptr, e1 = nullptr;
      if (c.timing && (issued & 7) == 4 && npairs < kTimed) {
        e0 = c.ev_pool[2 * npairs];
        e1 = c.ev_pool[2 * npairs + 1];
        pair_it.push_back(issued);
        npairs++;
      }
      c.cg_it = issued;
      if ((rc = cg_iteration(c, e0, e1, q == 0, q == CH - 1))) return rc;
    }
    MCX_HIP(hipMemcpyAsync(&c.h_cg[slot], c.cg, sizeof(CgState), hipMemcpyDeviceToHost, c.stream));
    MCX_HIP(hipEventRecord(c.ev_chunk[slot], c.stream));
    if (pending >= 0) {
      if ((rc = comm_wait(c, c.ev_chunk[pending], "CG chunk poll (all-reduced CG scalars)"))) return rc;
      if (c.h_cg[pending].reason) break;
    }
    pending = slot;
    slot ^= 1;
    if (issued > cap) break;
  }
  if ((rc = launch_cg_xfinal(c))) return rc;  // the owed VecAXPY(x, alpha, p) terms, deferred by k_cg_pupdate
  MCX_HIP(hipEventRecord(c.ev_chunk[slot], c.stream));  // after the last chunk's (gated) all-reduces
  if ((rc = comm_wait(c, c.ev_chunk[slot], "CG solve end"))) return rc;
  CgState fin;
  MCX_HIP(hipMemcpy(&fin, c.cg, sizeof(CgState), hipMemcpyDeviceToHost));
  if (!fin.reason) {
    set_error("CG loop ended without a converged reason");
    return 30;
  }
  *its = fin.its;
  *rnorm = fin.dp;
  *reason = fin.reason;
  c.last_its = fin.its;
  if (c.o.ksp_monitor) {
    // the norms this solve computed: entry 0 and one per completed iteration.  A stop before the
    // iteration's norm (INDEFINITE_MAT at the alpha step; z.r == 0 or INDEFINITE_PC at the top of the
    // next one, where its already counts it) leaves its entries, not its + 1: c.hist beyond them
    // is an earlier solve's
    const bool before_norm = fin.reason == MCX_KSP_DIVERGED_INDEFINITE_MAT ||
                             fin.reason == MCX_KSP_DIVERGED_INDEFINITE_PC ||
                             (fin.reason == MCX_KSP_CONVERGED_ATOL && fin.beta == 0.);
    const int nh = before_norm ? std::max(fin.its, 1) : fin.its + 1;
    c.last_hist.resize(nh);
    MCX_HIP(hipMemcpy(c.last_hist.data(), c.hist, sizeof(double) * nh, hipMemcpyDeviceToHost));
  }
  if (c.timing) {
    int n = 0;  // pairs around iterations that ran (later launches of the last chunk return at once)
    double tot = 0.;
    for (int q = 0; q < npairs; q++) {
      if (pair_it[q] >= fin.its) break;
      float ms = 0.f;
      MCX_HIP(hipEventElapsedTime(&ms, c.ev_pool[2 * q], c.ev_pool[2 * q + 1]));
      tot += ms;
      n++;
    }
    c.t.spmv_launches = n;
    c.t.spmv_ms_total = tot;
  }
  return 0;
}

}  // namespace mcx

using namespace mcx;

// command-line flags that are options of a context (mcx_set_option names behind a '-'), not
// mcx_opts fields: mcx_parse_args accepts them, mcx_apply_args applies them after mcx_init
static const char* const kApplyFlags[] = {"-micro_mem",     "-micro_rtol",      "-micro_max_it",  "-micro_nl_rtol",
                                          "-micro_nl_max_it", "-micro_nl_slots", "-micro_solver",
                                          "-micro_nl_solver", "-micro_nl_start",  "-micro_nl_ls",
                                          "-micro_nl_tangent", "-micro_nl_apply", "-micro_nl_warm",
                                          "-pc_type",       "-pc_mg_levels",    "-mg_levels_ksp_max_it",
                                          "-pc_mg_dist",    "-pc_mg_precision"};
static bool apply_flag(const char* k) {
  for (const char* f : kApplyFlags)
    if (!std::strcmp(k, f)) return true;
  return false;
}

// -micro_nl_ls K: the word is an integer 0 .. 16
static bool micro_nl_ls_word(const char* v) {
  if (!v || !*v) return false;
  char* end = nullptr;
  const long k = std::strtol(v, &end, 10);
  return !*end && k >= 0 && k <= 16;
}

#define CTX(p) Ctx& c = *reinterpret_cast<Ctx*>(p)
#define GUARD(p)                      \
  if (!(p)) {                         \
    set_error("null context");        \
    return 1;                         \
  }                                   \
  MCX_HIP(hipSetDevice(reinterpret_cast<Ctx*>(p)->device))

extern "C" {

const char* mcx_last_error(void) { return g_err.c_str(); }
const char* mcx_version(void) { return "macroc_amd 0.3 (gfx950, abi 3)"; }
int mcx_abi_version(void) { return MCX_ABI_VERSION; }

void mcx_default_opts(mcx_opts* o) {
  std::memset(o, 0, sizeof(*o));
  o->NX = 40;  // include/macroc.h:44-46
  o->NY = 3;
  o->NZ = 40;
  o->lx = 50.0;  // include/macroc.h:47-49
  o->ly = 1.0;
  o->lz = 50.0;
  o->dt = 0.001;
  o->final_time = 1.0;
  o->ts = 1;
  o->vtu_freq = -1;
  o->bc_type = MCX_BC_CIRCLE;  // src/init.c:64
  o->rad = 1.0;
  o->newton_max_its = 5;
  o->newton_min_tol = 1.0e-1;
  o->newton_rel_tol = 1.0e-4;
  o->ksp_rtol = 1.0e-5;  // src/init.c:147-148
  o->ksp_abstol = 1.0e-50;
  o->ksp_dtol = 1.0e4;
  o->ksp_max_it = 10000;
  o->micro_n = 2;
  o->micro_type = 1;
  const double mat[4] = {1.0e7, 0.25, 1.0e4, 1.0e7};  // src/init.c:31-32
  std::memcpy(o->micro_mat_1, mat, sizeof(mat));
  std::memcpy(o->micro_mat_2, mat, sizeof(mat));
  o->device = -1;
  o->mat_aij_split = 1;
  o->mat_aij_vi = 1;
  o->mat_vi_fma = 1;
}

int mcx_parse_args(mcx_opts* o, int argc, const char* const* argv) try {
  MCX_ENTRY();
  for (int a = 0; a < argc; a++) {
    const char* k = argv[a];
    const char* v = (a + 1 < argc) ? argv[a + 1] : nullptr;
    auto I = [&](const char* name, auto* f) {
      if (std::strcmp(k, name)) return false;
      if (!v) return false;
      *f = (std::remove_reference_t<decltype(*f)>)std::atoll(v);
      a++;
      return true;
    };
    auto D = [&](const char* name, double* f) {
      if (std::strcmp(k, name)) return false;
      if (!v) return false;
      *f = std::atof(v);
      a++;
      return true;
    };
    auto A4 = [&](const char* name, double* f) {
      if (std::strcmp(k, name)) return false;
      if (!v) return false;
      std::string s(v);
      size_t pos = 0;
      for (int q = 0; q < 4 && pos <= s.size(); q++) {
        size_t e = s.find(',', pos);
        f[q] = std::atof(s.substr(pos, e == std::string::npos ? std::string::npos : e - pos).c_str());
        if (e == std::string::npos) break;
        pos = e + 1;
      }
      a++;
      return true;
    };
    if (I("-da_grid_x", &o->NX) || I("-da_grid_y", &o->NY) || I("-da_grid_z", &o->NZ) ||
        I("-da_processors_x", &o->px) || I("-da_processors_y", &o->py) || I("-da_processors_z", &o->pz) ||
        D("-lx", &o->lx) || D("-ly", &o->ly) || D("-lz", &o->lz) || D("-dt", &o->dt) || I("-ts", &o->ts) ||
        I("-vtu_freq", &o->vtu_freq) || I("-bc_type", &o->bc_type) || I("-newton_max_its", &o->newton_max_its) ||
        D("-newton_min_tol", &o->newton_min_tol) || D("-newton_rel_tol", &o->newton_rel_tol) ||
        D("-ksp_rtol", &o->ksp_rtol) || D("-ksp_atol", &o->ksp_abstol) || D("-ksp_divtol", &o->ksp_dtol) ||
        I("-ksp_max_it", &o->ksp_max_it) || I("-micro_n", &o->micro_n) || I("-micro_type", &o->micro_type) ||
        A4("-micro_mat_1", o->micro_mat_1) || A4("-micro_mat_2", o->micro_mat_2) || I("-device", &o->device) ||
        I("-mat_aij_split", &o->mat_aij_split) || I("-mat_aij_vi", &o->mat_aij_vi) ||
        I("-mat_vi_fma", &o->mat_vi_fma))
      continue;
    if (!std::strcmp(k, "-dm_mat_type")) {
      if (!v || (std::strcmp(v, "aij") && std::strcmp(v, "sbaij"))) {
        set_error(std::string("-dm_mat_type: aij or sbaij, got ") + (v ? v : "(none)"));
        return 2;
      }
      o->mat_type = std::strcmp(v, "sbaij") ? MCX_MAT_AIJ : MCX_MAT_SBAIJ;
      a++;
      continue;
    }
    if (!std::strcmp(k, "-mat_ignore_lower_triangular")) continue;
    if (!std::strcmp(k, "-mat_law")) {
      if (!v || (std::strcmp(v, "elastic") && std::strcmp(v, "plastic") && std::strcmp(v, "external") &&
                 std::strcmp(v, "micro") && std::strcmp(v, "micro_nl"))) {
        set_error(std::string("-mat_law: micro_nl, elastic, plastic, external or micro, got ") + (v ? v : "(none)"));
        return 2;
      }
      o->mat_law = !std::strcmp(v, "plastic") ? MCX_LAW_PLASTIC
                   : !std::strcmp(v, "external") ? MCX_LAW_EXTERNAL
                   : !std::strcmp(v, "micro")    ? MCX_LAW_MICRO
                   : !std::strcmp(v, "micro_nl") ? MCX_LAW_MICRO_NL
                                                 : MCX_LAW_ELASTIC;
      a++;
      continue;
    }
    if (!std::strcmp(k, "-ksp_monitor")) {
      o->ksp_monitor = 1;
      continue;
    }
    if (apply_flag(k)) {  // options of the context: mcx_apply_args sets them after mcx_init
      if (!std::strcmp(k, "-micro_mem") && (!v || (std::strcmp(v, "lds") && std::strcmp(v, "device")))) {
        set_error(std::string("-micro_mem: lds or device, got ") + (v ? v : "(none)"));
        return 2;
      }
      if (!std::strcmp(k, "-micro_solver") && (!v || (std::strcmp(v, "cell") && std::strcmp(v, "grid")))) {
        set_error(std::string("-micro_solver: cell or grid, got ") + (v ? v : "(none)"));
        return 2;
      }
      if (!std::strcmp(k, "-micro_nl_solver") && (!v || (std::strcmp(v, "cell") && std::strcmp(v, "grid")))) {
        set_error(std::string("-micro_nl_solver: cell or grid, got ") + (v ? v : "(none)"));
        return 2;
      }
      if (!std::strcmp(k, "-micro_nl_start") && (!v || (std::strcmp(v, "zero") && std::strcmp(v, "elastic")))) {
        set_error(std::string("-micro_nl_start: zero or elastic, got ") + (v ? v : "(none)"));
        return 2;
      }
      if (!std::strcmp(k, "-micro_nl_ls") && !micro_nl_ls_word(v)) {
        set_error(std::string("-micro_nl_ls: an integer 0 .. 16, got ") + (v ? v : "(none)"));
        return 2;
      }
      if (!std::strcmp(k, "-micro_nl_tangent") && (!v || (std::strcmp(v, "seq") && std::strcmp(v, "block")))) {
        set_error(std::string("-micro_nl_tangent: seq or block, got ") + (v ? v : "(none)"));
        return 2;
      }
      if (!std::strcmp(k, "-micro_nl_apply") && (!v || (std::strcmp(v, "split") && std::strcmp(v, "fused")))) {
        set_error(std::string("-micro_nl_apply: split or fused, got ") + (v ? v : "(none)"));
        return 2;
      }
      if (!std::strcmp(k, "-micro_nl_warm") && (!v || (std::strcmp(v, "off") && std::strcmp(v, "on")))) {
        set_error(std::string("-micro_nl_warm: off or on, got ") + (v ? v : "(none)"));
        return 2;
      }
      if (!std::strcmp(k, "-pc_mg_precision") && (!v || (std::strcmp(v, "double") && std::strcmp(v, "single")))) {
        set_error(std::string("-pc_mg_precision: double or single, got ") + (v ? v : "(none)"));
        return 2;
      }
      if (!std::strcmp(k, "-pc_type") && v && std::strcmp(v, "jacobi") && std::strcmp(v, "mg")) {
        set_error(std::string("only -ksp_type cg / -pc_type jacobi / mg are implemented, got ") + v);
        return 2;
      }
      a++;
      continue;
    }
    if (!std::strcmp(k, "-ksp_type")) {
      if (v && std::strcmp(v, "cg")) {
        set_error(std::string("only -ksp_type cg / -pc_type jacobi / mg are implemented, got ") + v);
        return 2;
      }
      a++;
      continue;
    }
    if (!std::strcmp(k, "-pc_mg_galerkin")) {  // the coarse operators are Galerkin products, always
      if (v && v[0] != '-') a++;
      continue;
    }
    std::fprintf(stderr, "WARNING! There are options you set that were not used: %s\n", k);
  }
  return 0;
} MCX_CATCH

int mcx_init(const mcx_opts* o, int rank, int nranks, const void* comm_id, void** ctx) try {
  MCX_ENTRY();
  if (!o || !ctx || nranks < 1 || rank < 0 || rank >= nranks) {
    set_error("mcx_init: bad arguments");
    return 1;
  }
  Ctx* c = new Ctx();
  int rc = init_ctx(*c, o, rank, nranks, comm_id, nullptr);
  if (rc) {
    std::string e = g_err;
    free_ctx(c);
    g_err = e;
    *ctx = nullptr;
    return rc;
  }
  *ctx = c;
  return 0;
} MCX_CATCH

int mcx_init_local(const mcx_opts* o, int rank, void* group, void** ctx) try {
  MCX_ENTRY();
  auto* lg = static_cast<LocalGroup*>(group);
  if (!o || !ctx || !lg || rank < 0 || rank >= lg->nranks) {
    set_error("mcx_init_local: bad arguments");
    return 1;
  }
  Ctx* c = new Ctx();
  int rc = init_ctx(*c, o, rank, lg->nranks, nullptr, lg);
  if (rc) {
    std::string e = g_err;
    free_ctx(c);
    g_err = e;
    *ctx = nullptr;
    return rc;
  }
  *ctx = c;
  return 0;
} MCX_CATCH

int mcx_finalize(void* ctx) try {
  MCX_ENTRY();
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  int rc = 0;
  if (c && c->lg) {
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    // no member still copies from this context's buffers: every member drained its streams
    // before crossing.  If the group broke (a member stopped, or reached another collective),
    // the members' enqueued copies may still read these buffers: wait for the whole device.
    if ((rc = group_barrier(c->lg, c->rank, BAR_FINALIZE, c->comm_timeout))) (void)hipDeviceSynchronize();
    c->lg->members[c->rank] = nullptr;
  }
  const std::string e = g_err;
  free_ctx(c);
  if (rc) g_err = e;
  return rc;
} MCX_CATCH

static void fill_info(const Ctx& c, mcx_info* in) {
  const Geo& g = c.g;
  std::memset(in, 0, sizeof(*in));
  in->NX = g.NX;
  in->NY = g.NY;
  in->NZ = g.NZ;
  in->px = c.m;
  in->py = c.n;
  in->pz = c.p;
  in->rank = c.rank;
  in->nranks = c.nranks;
  in->xs = g.xs;
  in->ys = g.ys;
  in->zs = g.zs;
  in->nx = g.nx;
  in->ny = g.ny;
  in->nz = g.nz;
  in->Xs = std::max(g.xs - 1, 0);
  in->Ys = std::max(g.ys - 1, 0);
  in->Zs = std::max(g.zs - 1, 0);
  in->Nx = std::min(g.xs + g.nx + 1, g.NX) - in->Xs;
  in->Ny = std::min(g.ys + g.ny + 1, g.NY) - in->Ys;
  in->Nz = std::min(g.zs + g.nz + 1, g.NZ) - in->Zs;
  in->ndofs_global = 3 * c.rank_node_off[c.nranks];
  in->ndofs_local = 3 * (int64_t)g.nown;
  in->dof_offset = 3 * c.rank_node_off[c.rank];
  in->nnz_local = c.nnz_local;
  in->nnz_global = c.nnz_global;
  int64_t cnt[3];
  int s[3] = {g.xs, g.ys, g.zs}, w[3] = {g.nx, g.ny, g.nz};
  for (int d = 0; d < 3; d++) {
    int lo = s[d] > 0 ? s[d] - 1 : s[d];
    cnt[d] = std::max(0, s[d] + w[d] - 1 - lo);
  }
  in->nelem_local = cnt[0] * cnt[1] * cnt[2];
  in->nelem_ext = g.nelem;
  in->dx = g.dx;
  in->dy = c.dy;
  in->dz = g.dz;
  in->wg = g.wg;
  in->device_bytes = c.device_bytes;
  in->device = c.device;
  in->storage = c.fmt;
  in->split_slots = c.fmt == FMT_SPLIT ? c.dsl.L : 0;
  in->split_bits = c.fmt == FMT_SPLIT ? (c.dsl.wide ? 32 : 16) : 0;
  in->vi_values = c.fmt == FMT_VI ? c.vi_n : 0;
  in->vi_bits = c.fmt == FMT_VI ? c.vi_bits : 0;
  in->vi_blocks = c.fmt == FMT_VI && c.vi_block ? c.vi_nblocks : 0;
  in->vi_exc_nodes = c.fmt == FMT_VI && c.vi_block ? c.vi_nexc : 0;
  in->split_escapes = c.fmt == FMT_SPLIT && c.dsl.esc ? c.dsl.nesc : 0;
  in->st_listed = c.device >= 0 && st_used(c) ? c.st_n : -1;
  if (c.device >= 0) spmv_tile(c, &in->spmv_tx, &in->spmv_ty, &in->spmv_kc);
  in->ex0 = g.ex0;
  in->ey0 = g.ey0;
  in->ez0 = g.ez0;
  in->nex = g.nex;
  in->ney = g.ney;
  in->nez = g.nez;
}


int mcx_get_info(void* ctx, mcx_info* in) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  fill_info(c, in);
  return 0;
} MCX_CATCH

int mcx_get_st_dma(void* ctx, int* on) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  if (on) *on = c.st_dma_last;
  return 0;
} MCX_CATCH

int mcx_pc_mg_get_precision(void* ctx, int* single) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  if (single) *single = c.pc_mg_precision;
  return 0;
} MCX_CATCH

int mcx_micro_nl_get_tangent(void* ctx, int* block, int* col_its) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  if (block) *block = c.mnl_tangent;
  if (col_its) {  // [8 nelem][6], Gauss points in the order of mcx_micro_nl_get_info
    const int64_t E = c.g.nelem, ngp = 8 * E;
    for (int64_t e = 0; e < E; e++)
      for (int gp = 0; gp < 8; gp++)
        for (int l = 0; l < 6; l++)
          col_its[(e * 8 + gp) * 6 + l] = c.mnl_col_its.empty() ? 0 : c.mnl_col_its[(size_t)(l * ngp + gp * E + e)];
  }
  return 0;
} MCX_CATCH

int mcx_micro_nl_get_apply(void* ctx, int* fused, long long* launches) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  if (fused) *fused = c.mnl_apply;
  if (launches) *launches = c.mnl_apply_launches;
  return 0;
} MCX_CATCH

int mcx_micro_nl_get_warm(void* ctx, int* option, int* used) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  if (option) *option = c.mnl_warm;
  if (used) {  // [8 nelem], Gauss points in the order of mcx_micro_nl_get_info
    const int64_t E = c.g.nelem, ngp = 8 * E;
    for (int64_t q = 0; q < ngp; q++) used[q] = 0;
    if (c.mat.law == MCX_LAW_MICRO_NL && c.mnl_last_nsolve > 0 && c.mnl_list && c.micro.n > 2) {
      std::vector<int> list((size_t)c.mnl_last_nsolve);
      MCX_HIP(hipStreamSynchronize(c.stream));
      MCX_HIP(hipMemcpy(list.data(), c.mnl_list, sizeof(int) * list.size(), hipMemcpyDeviceToHost));
      for (int q : list)
        used[((int64_t)q % E) * 8 + q / E] = 1 + (c.mnl_warm_hit.empty() ? 0 : (int)c.mnl_warm_hit[(size_t)q]);
    }
  }
  return 0;
} MCX_CATCH

int mcx_comm_info(void* ctx, int* comm_ranks, int* comm_rank, int* device) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  int n = 1, r = 0, d = c.device;
  if (c.lg) {
    n = c.lg->nranks;
    r = c.rank;
  } else if (int rc = comm_query(c, &n, &r, &d)) {
    return rc;
  }
  if (comm_ranks) *comm_ranks = n;
  if (comm_rank) *comm_rank = r;
  if (device) *device = d;
  return 0;
} MCX_CATCH

int mcx_plan(const mcx_opts* o, int rank, int nranks, mcx_info* in) try {
  MCX_ENTRY();
  if (!o || !in || nranks < 1 || rank < 0 || rank >= nranks) {
    set_error("mcx_plan: bad arguments");
    return 1;
  }
  Ctx c;
  c.o = *o;
  c.rank = rank;
  c.nranks = nranks;
  c.device = -1;
  int rc = setup_decomposition(c);
  if (rc) return rc;
  c.nnz_local = count_nnz_rows(c, c.g.xs, c.g.ys, c.g.zs, c.g.nx, c.g.ny, c.g.nz);
  c.nnz_global = count_nnz_rows(c, 0, 0, 0, o->NX, o->NY, o->NZ);
  fill_info(c, in);
  return 0;
} MCX_CATCH

int mcx_plan_halo(const mcx_opts* o, int rank, int nranks, int* nnbr, int* nbr_rank, int64_t* send_cnt,
                  int64_t* recv_cnt, int64_t* send_nat, int64_t* recv_nat, int64_t* nsend, int64_t* nrecv) try {
  MCX_ENTRY();
  if (!o || nranks < 1 || rank < 0 || rank >= nranks) {
    set_error("mcx_plan_halo: bad arguments");
    return 1;
  }
  Ctx c;
  c.o = *o;
  c.rank = rank;
  c.nranks = nranks;
  int rc = setup_decomposition(c);
  if (rc) return rc;
  std::vector<int> sidx, ridx;
  const int n3[3] = {c.g.nx, c.g.ny, c.g.nz};
  plan_halo(c, c.halo, n3, c.g.PX, c.g.PX * c.g.PY, sidx, ridx);
  const HaloPlan& h = c.halo;
  if (nnbr) *nnbr = (int)h.nbr_rank.size();
  if (nsend) *nsend = h.nsend;
  if (nrecv) *nrecv = h.nrecv;
  for (size_t q = 0; q < h.nbr_rank.size(); q++) {
    if (nbr_rank) nbr_rank[q] = h.nbr_rank[q];
    if (send_cnt) send_cnt[q] = h.send_cnt[q];
    if (recv_cnt) recv_cnt[q] = h.recv_cnt[q];
  }
  if (send_nat)
    for (int64_t t = 0; t < h.nsend; t++) send_nat[t] = pad_to_natural(c, sidx[t]);
  if (recv_nat)
    for (int64_t t = 0; t < h.nrecv; t++) recv_nat[t] = pad_to_natural(c, ridx[t]);
  return 0;
} MCX_CATCH

int mcx_material_set(void* ctx, int id, double E, double nu, double Sy, double Ka, int type) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  (void)Sy;
  (void)Ka;
  (void)type;
  if (micro_law(c.mat.law)) {  // the micro cell's two phases; Sy, Ka: -mat_law micro_nl only
    if (id != 0 && id != 1) {
      set_error("mcx_material_set: -mat_law micro has materials 0 and 1");
      return 3;
    }
    if (id == 0) {
      c.mat.E = E;
      c.mat.nu = nu;
      c.mat.Sy = Sy;
      c.mat.Ka = Ka;
    }
    c.micro.E[id] = E;
    c.micro.nu[id] = nu;
    c.mnl_Sy[id] = Sy;
    c.mnl_Ka[id] = Ka;
    c.micro_dirty = true;
    return 0;
  }
  if (id == 0) {
    c.mat.E = E;
    c.mat.nu = nu;
    c.mat.Sy = Sy;
    c.mat.Ka = Ka;
    elastic_C(E, nu, c.mat.C);
  } else if (id == 1 && (E != c.mat.E || nu != c.mat.nu || Sy != c.mat.Sy || Ka != c.mat.Ka)) {
    set_error("two distinct materials need the MicroPP micro-structure (out of scope); use equal materials");
    return 3;
  }
  return 0;
} MCX_CATCH

double mcx_get_displacement(void* ctx, int time_s) {
  Ctx& c = *reinterpret_cast<Ctx*>(ctx);
  // src/bcs.c:52-58 with the missing `return` restored
  double time = time_s * c.o.dt;
  return -1.0 * (time / c.o.final_time);
}

int mcx_zero_u(void* ctx) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  MCX_HIP(hipMemsetAsync(c.u_pad, 0, sizeof(double) * 3 * (size_t)c.g.PX * c.g.PY * c.g.PZ, c.stream));
  return 0;
} MCX_CATCH

int mcx_apply_bc_u(void* ctx, double U) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  launch_apply_bc_u(c, U);
  MCX_HIP(hipGetLastError());
  return 0;
} MCX_CATCH

int mcx_set_strains(void* ctx) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  PhaseTimer t(c, PH_STRAINS);
  int rc = halo_exchange(c, c.u_pad);  // DMGlobalToLocal (src/assembly.c:40-41)
  if (rc) return rc;
  launch_strains(c);
  MCX_HIP(hipGetLastError());
  return 0;
} MCX_CATCH

// -mat_law micro: C_hom of the two-phase cell into mat.C when it is not current: six
// unit-strain solves in one launch (k_micro_rve), column l = block l's average stress, then
// C_hom = (C + C^T) / 2 on the host (exactly symmetric; the same bits in every context)
static MicroNlArgs mnl_args(const Ctx& c) {
  MicroNlArgs a{};
  a.m = c.micro;
  const int interior = 3 * (a.m.n - 2) * (a.m.n - 2) * (a.m.n - 2);
  a.m.max_it = c.micro_max_it > 0 ? c.micro_max_it : 10 * interior;
  for (int p = 0; p < 2; p++) {
    a.Sy[p] = c.mnl_Sy[p];
    a.Ka[p] = c.mnl_Ka[p];
  }
  a.nl_rtol = c.mnl_rtol;
  a.nl_max_it = c.mnl_max_it;
  a.nl_start = c.mnl_start;
  a.nl_ls = c.mnl_ls;
  return a;
}

// the grid-wide solver (option micro_solver 1) serves -mat_law micro only
static bool micro_grid(const Ctx& c) { return c.micro_solver == 1 && c.mat.law == MCX_LAW_MICRO; }
// the grid-wide solver of -mat_law micro_nl (option micro_nl_solver 1): C_hom and the listed points
static bool micro_nl_grid(const Ctx& c) { return c.mnl_solver == 1 && c.mat.law == MCX_LAW_MICRO_NL; }

// the largest micro_n of the solver and memory mode in use (options micro_solver, micro_mem)
static int micro_nmax(const Ctx& c) {
  return micro_grid(c) ? MICRO_NMAX_GRID : micro_nl_grid(c) ? MICRO_NMAX_NL_GRID : c.micro_mem ? MICRO_NMAX_DEV : MICRO_NMAX;
}

static int micro_n_refused(const Ctx& c) {
  const int n = c.micro.n;
  if (n >= 2 && n <= micro_nmax(c)) return 0;
  std::string e = "-mat_law micro: -micro_n " + std::to_string(n) + " outside the supported range 2 <= micro_n <= " +
                  std::to_string(micro_nmax(c));
  if (micro_grid(c))
    e += " (option micro_solver 1: one workgroup per tile of 8x8x8 nodes, the CG state in device memory)";
  else if (micro_nl_grid(c))
    e += " (option micro_nl_solver 1: one workgroup per tile of 8x8x8 nodes; a history slot is 224 B x 8 (micro_n - 1)^3)";
  else if (c.micro_mem)
    e += " (option micro_mem 1: one workgroup per cell with its CG state in device memory)";
  else
    e += " (option micro_mem 0: the cell's CG state has to fit one CU's LDS; micro_mem 1 / -micro_mem device keeps "
         "it in device memory, up to micro_n " + std::to_string(MICRO_NMAX_DEV) + ")";
  set_error(e);
  return 31;
}

// (re)allocates a device array whose size follows the cell; bytes = what it holds now
static int micro_resize(Ctx& c, double** p, int64_t* bytes, int64_t want) {
  if (*p && *bytes == want) return 0;
  if (*p) {
    MCX_HIP(hipStreamSynchronize(c.stream));
    MCX_HIP(hipFree(*p));
    *p = nullptr;
    c.device_bytes -= *bytes;
    *bytes = 0;
  }
  if (want <= 0) return 0;
  MCX_HIP(hipMalloc((void**)p, (size_t)want));
  *bytes = want;
  c.device_bytes += want;
  return 0;
}

// option micro_solver 1: the six solves as launches over the whole device.  The host
// enqueues micro_grid_poll gated iterations at a time and reads the six done flags back; the
// device stops every load case by itself (converged, !(pq > 0), max_it), so what is enqueued past
// that changes nothing and the results do not depend on micro_grid_poll.
// solves of micro_nl_solver 1 that share a launch: what keeps the vectors within 512 MiB, at most 64 and
// at most the local Gauss points (64 from n = 2 to 33, 13 at n = 64); micro_mem_blocks > 0 replaces it
// Under micro_nl_tangent 1 a solve has 26 vectors, not 6, within the same 512 MiB, and the
// five more sets of work stresses have a budget of their own, 1536 MiB (64 / 64 / 23 / 3 solves at
// n = 10 / 20 / 33 / 64)
static bool mnl_block(const Ctx& c) { return c.mnl_tangent == 1 && c.mnl_solver == 1 && c.mat.law == MCX_LAW_MICRO_NL; }
static int64_t mnl_grid_batch(const Ctx& c) {
  const int64_t n = c.micro.n, per = (int64_t)sizeof(double) * MNLG_NVEC * 3 * n * n * n + (mnl_block(c) ? mnlb_vec_bytes((int)n) : 0);
  int64_t b = std::min<int64_t>(64, ((int64_t)512 << 20) / per);
  if (mnl_block(c) && n > 1) b = std::min<int64_t>(b, ((int64_t)1536 << 20) / mnlb_sig_bytes((int)n));
  if (c.mnl_ws_blocks_opt > 0) b = c.mnl_ws_blocks_opt;
  return std::max<int64_t>(1, std::min<int64_t>(b, std::max<int64_t>(1, 8 * c.g.nelem)));
}

// the grid-wide solvers' one workspace: the six unit-strain solves' layout (mg_layout), and under
// micro_nl_solver 1 the listed points' (mnlg_layout) in the same memory at another time
static int64_t grid_ws_bytes(const Ctx& c) {
  const int64_t lin = mg_ws_bytes(c.micro.n);
  if (!micro_nl_grid(c)) return lin;
  const int64_t batch = mnl_grid_batch(c);
  return std::max(lin, mnlg_ws_bytes(c.micro.n, batch) + (mnl_block(c) ? mnlb_ws_bytes(c.micro.n, batch) : 0));
}

static int solve_micro_grid(Ctx& c, const MicroArgs& m) {
  if (int rc = micro_resize(c, &c.micro_grid_ws, &c.micro_grid_bytes, grid_ws_bytes(c))) return rc;
  const MicroGridWs w = mg_layout(c.micro_grid_ws, m.n);
  launch_mg_setup(c, m, w);
  MCX_HIP(hipGetLastError());
  for (int64_t enq = 0;;) {
    MicroGridState h[6];
    MCX_HIP(hipMemcpyAsync(h, w.st, sizeof(h), hipMemcpyDeviceToHost, c.stream));
    MCX_HIP(hipStreamSynchronize(c.stream));
    bool done = true;
    for (int l = 0; l < 6; l++) done = done && h[l].done;
    if (done || enq >= m.max_it) break;
    for (int q = 0; q < c.micro_grid_poll && enq < m.max_it; q++, enq++) launch_mg_iterate(c, m, w);
    MCX_HIP(hipGetLastError());
  }
  launch_mg_finish(c, m, w);
  return 0;
}

static int ensure_micro(Ctx& c) {
  if (!micro_law(c.mat.law) || !c.micro_dirty) return 0;
  MicroArgs m = c.micro;
  if (int rc = micro_n_refused(c)) return rc;
  if (m.type != 0 && m.type != 1) {
    set_error("-mat_law micro: -micro_type " + std::to_string(m.type) +
              " is not implemented (0: centred sphere, 1: flat layer in y)");
    return 32;
  }
  const int interior = 3 * (m.n - 2) * (m.n - 2) * (m.n - 2);
  m.max_it = c.micro_max_it > 0 ? c.micro_max_it : 10 * interior;
  const int64_t ndof = 3 * (int64_t)m.n * m.n * m.n, nmgp = 8 * (int64_t)(m.n - 1) * (m.n - 1) * (m.n - 1);
  if (c.mat.law == MCX_LAW_MICRO_NL) {  // the unit-strain fields and their concentration tensors, for this n
    int rc;
    if ((rc = micro_resize(c, &c.mnl_ufield, &c.mnl_ufield_bytes, (int64_t)sizeof(double) * 6 * ndof)) ||
        (rc = micro_resize(c, &c.mnl_conc, &c.mnl_conc_bytes, (int64_t)sizeof(double) * MNL_CONC * nmgp)))
      return rc;
  }
  if (micro_grid(c) || micro_nl_grid(c)) {  // the same six results in micro_out, by the grid-wide solver
    if (int rc = micro_resize(c, &c.micro_ws, &c.micro_ws_bytes, 0)) return rc;
    if (int rc = solve_micro_grid(c, m)) return rc;
    if (micro_nl_grid(c)) {  // the linear test superposes the six fields: x of every load case
      const MicroGridWs w = mg_layout(c.micro_grid_ws, m.n);
      MCX_HIP(hipMemcpy2DAsync(c.mnl_ufield, sizeof(double) * ndof, w.vec, sizeof(double) * 5 * ndof, sizeof(double) * ndof,
                               6, hipMemcpyDeviceToDevice, c.stream));
    }
  } else {
    const int64_t rve_ws = c.micro_mem ? (int64_t)sizeof(double) * 6 * 5 * ndof : 0;  // micro_mem 1: six workspaces
    if (int rc = micro_resize(c, &c.micro_ws, &c.micro_ws_bytes, rve_ws)) return rc;
    launch_micro_rve(c, m);
  }
  MCX_HIP(hipGetLastError());
  double h[6 * MICRO_OUT];
  MCX_HIP(hipMemcpyAsync(h, c.micro_out, sizeof(h), hipMemcpyDeviceToHost, c.stream));
  MCX_HIP(hipStreamSynchronize(c.stream));
  static const char* const kVoigt[6] = {"xx", "yy", "zz", "xy", "xz", "yz"};
  double Cc[36];
  for (int l = 0; l < 6; l++) {
    const double* o = h + MICRO_OUT * l;
    c.micro_its[l] = (int)o[6];
    c.micro_rnorm[l] = o[7];
    if (o[8] == 0.) {
      char buf[256];
      std::snprintf(buf, sizeof(buf),
                    "-mat_law micro: the micro cell's CG did not converge for load case %d (unit strain component "
                    "%s): %d iterations, relative preconditioned residual %.3e > micro_rtol %.3e",
                    l, kVoigt[l], c.micro_its[l], o[7], m.rtol);
      set_error(buf);
      return 33;
    }
    for (int k = 0; k < 6; k++) Cc[k * 6 + l] = o[k];
  }
  for (int k = 0; k < 6; k++)
    for (int l = 0; l < 6; l++) c.mat.C[k * 6 + l] = 0.5 * (Cc[k * 6 + l] + Cc[l * 6 + k]);
  if (c.mat.law == MCX_LAW_MICRO_NL) {  // the linear test's strain concentration tensors from the six fields
    launch_mnl_conc(c, mnl_args(c));
    MCX_HIP(hipGetLastError());
  }
  c.micro_dirty = false;
  return 0;
}

// -mat_law micro_nl: the linear test of the points without a slot, slots for those
// that fail it, then one non-linear cell solve per slotted point
static int64_t mnl_slot_bytes(const Ctx& c) {
  const int64_t ne = c.micro.n - 1;
  return (int64_t)sizeof(double) * MNL_WS * 8 * ne * ne * ne;
}

// option micro_nl_warm: the warm store follows the option, the solver and the pool: mnl_cap
// records, all invalid, when it is (re)allocated; a change of micro_nl_slots therefore invalidates them
static int mnl_warm_resize(Ctx& c) {
  const bool on = c.mnl_warm && micro_nl_grid(c) && c.mnl_pool && c.micro.n > 2;  // n = 2: no interior dof, nothing to keep
  const int64_t want = on ? c.mnl_cap * mnl_warm_bytes(c.micro.n) : 0;
  if (want == c.mnl_warm_store_bytes) return 0;
  if (int rc = micro_resize(c, &c.mnl_warm_store, &c.mnl_warm_store_bytes, want)) return rc;
  if (want > 0) MCX_HIP(hipMemsetAsync(c.mnl_warm_store, 0, (size_t)want, c.stream));
  return 0;
}

// option micro_nl_solver 1: the nsolve listed points, mnl_grid_batch at a time, as launches
// over the whole device.  Per batch the host enqueues one transition (a CG has ended or not begun:
// the next Newton step, the next tangent column or the end) and up to micro_grid_poll gated CG
// iterations, then reads the records back; the device steps every solve through k_mnl_solve's
// loop by itself and counts its own iterations, so what is enqueued for a solve in another stage
// changes nothing and the results do not depend on micro_grid_poll or on the batch.
// With micro_nl_start 1 or micro_nl_ls > 0 a transition may leave a solve before
// another state pass (the predictor, a rejected trial).  A round whose read-back (or start) shows a
// solve about to take a Newton state pass therefore holds a second transition, which makes that
// pass, so that the solve does not idle through the round's CG iterations; other rounds hold one.
static int solve_mnl_grid(Ctx& c, const MicroNlArgs& a, int nsolve) {
  const int64_t batch = mnl_grid_batch(c);
  if (int rc = micro_resize(c, &c.micro_grid_ws, &c.micro_grid_bytes, grid_ws_bytes(c))) return rc;
  MnlGridWs w = mnlg_layout(c.micro_grid_ws, a.m.n, batch);
  if (c.mnl_warm_store) {  // option micro_nl_warm 1: [mnl_cap][7][3 n^3] fields, then [mnl_cap] headers
    w.warm = c.mnl_warm_store;
    w.whdr = reinterpret_cast<MnlWarmHdr*>(c.mnl_warm_store + c.mnl_cap * 7 * 3 * (int64_t)a.m.n * a.m.n * a.m.n);
    c.mnl_warm_hit.assign((size_t)(8 * c.g.nelem), 0);
  }
  const bool block = mnl_block(c);  // option micro_nl_tangent 1: the six columns of a solve as one block
  const MnlBlockWs bw = block ? mnlb_layout(c.micro_grid_ws, a.m.n, batch) : MnlBlockWs{};
  std::vector<MnlBlockCol> hc(block ? (size_t)batch * 6 : 0);
  const int per = std::max(1, std::min(c.micro_grid_poll, a.m.max_it));
  // a solve has at most nl_max_it + 1 state passes and six columns, each CG at most max_it iterations
  // (and, globalised, one more pass for the predictor and up to nl_ls more per step)
  const int64_t max_rounds = (int64_t)((a.nl_max_it + 1) * (a.nl_ls + 1) + 8) * ((int64_t)(std::max(a.m.max_it, 1) + per - 1) / per + 1);
  const bool globalised = a.nl_start || a.nl_ls > 0 || w.warm;  // the warm predictor is a second state pass too
  std::vector<MnlGridState> h((size_t)batch);
  for (int base = 0; base < nsolve; base += (int)batch) {
    const int cnt = (int)std::min<int64_t>(batch, nsolve - base);
    launch_mnlg_start(c, w, base, cnt);
    bool newton_pass = true;  // a solve of the batch is at a Newton state pass (all are, at the start)
    for (int64_t round = 0;; round++) {
      if (block) {
        launch_mnlb_transition(c, a, w, bw, cnt);
        if (globalised && newton_pass) launch_mnlb_transition(c, a, w, bw, cnt);
        for (int q = 0; q < per; q++) launch_mnlb_iterate(c, a, w, bw, cnt);
      } else {
        launch_mnlg_transition(c, a, w, cnt);
        if (globalised && newton_pass) launch_mnlg_transition(c, a, w, cnt);
        for (int q = 0; q < per; q++) launch_mnlg_iterate(c, a, w, cnt);
      }
      MCX_HIP(hipGetLastError());
      MCX_HIP(hipMemcpyAsync(h.data(), w.st, sizeof(MnlGridState) * cnt, hipMemcpyDeviceToHost, c.stream));
      MCX_HIP(hipStreamSynchronize(c.stream));
      bool done = true;
      newton_pass = false;
      for (int s = 0; s < cnt; s++) {
        done = done && h[s].stage == MNLG_DONE;
        newton_pass = newton_pass || (h[s].stage == MNLG_TRANS && h[s].lc < 0);
      }
      if (done) break;
      if (round >= max_rounds) {
        set_error("-mat_law micro_nl: micro_nl_solver 1 did not end within its iteration limits (internal error)");
        return 35;
      }
    }
    if (w.warm)
      for (int s = 0; s < cnt; s++) c.mnl_warm_hit[(size_t)h[s].q] = (char)(h[s].warm != 0);
    if (block) {  // the columns' own counts, for mcx_micro_nl_get_tangent (a solve that Newton failed never started them)
      const int64_t ngp = 8 * c.g.nelem;
      MCX_HIP(hipMemcpyAsync(hc.data(), bw.col, sizeof(MnlBlockCol) * 6 * cnt, hipMemcpyDeviceToHost, c.stream));
      MCX_HIP(hipStreamSynchronize(c.stream));
      for (int s = 0; s < cnt; s++)
        for (int l = 0; l < 6 && h[s].lc == 6; l++) c.mnl_col_its[(size_t)(l * ngp + h[s].q)] = hc[(size_t)s * 6 + l].its;
    }
  }
  return 0;
}

static int micro_nl_homogenize(Ctx& c) {
  c.mnl_apply_launches = 0;
  if (int rc = ensure_micro(c)) return rc;
  const MicroNlArgs a = mnl_args(c);
  const int64_t ngp = 8 * c.g.nelem, bytes = mnl_slot_bytes(c);
  int64_t want = c.mnl_slots_opt;
  if (want <= 0) want = std::max<int64_t>(1, std::min<int64_t>(ngp, ((int64_t)2 << 30) / bytes));
  if (c.mnl_pool && want != c.mnl_cap) {  // micro_nl_slots changed with slots in use: move them
    if (want < c.mnl_used) {
      set_error("micro_nl_slots " + std::to_string(want) + " is below the " + std::to_string(c.mnl_used) +
                " slots in use");
      return 34;
    }
    double* p = nullptr;
    MCX_HIP(hipMalloc((void**)&p, (size_t)(want * bytes)));
    MCX_HIP(hipMemsetAsync(p, 0, (size_t)(want * bytes), c.stream));
    MCX_HIP(hipMemcpyAsync(p, c.mnl_pool, (size_t)(c.mnl_used * bytes), hipMemcpyDeviceToDevice, c.stream));
    MCX_HIP(hipStreamSynchronize(c.stream));
    MCX_HIP(hipFree(c.mnl_pool));
    c.device_bytes += (want - c.mnl_cap) * bytes;
    c.mnl_pool = p;
  }
  c.mnl_cap = want;
  launch_mnl_linear(c, a);
  MCX_HIP(hipGetLastError());
  int h[4];
  MCX_HIP(hipMemcpyAsync(h, c.mnl_cnt, sizeof(h), hipMemcpyDeviceToHost, c.stream));
  MCX_HIP(hipStreamSynchronize(c.stream));
  if (h[1] < 0) {
    char buf[320];
    std::snprintf(buf, sizeof(buf),
                  "-mat_law micro_nl: the history pool is too small: micro_nl_slots %lld, %lld slots in use and %d more "
                  "Gauss points left the linear range (%lld needed; %lld bytes per slot)",
                  (long long)c.mnl_cap, (long long)c.mnl_used, h[0], (long long)(c.mnl_used + h[0]), (long long)bytes);
    set_error(buf);
    return 34;
  }
  c.mnl_col_its.assign(c.mnl_col_its.size(), 0);
  c.mnl_warm_hit.clear();
  c.mnl_last_nsolve = h[1];
  if (h[1] == 0) return mnl_warm_resize(c);
  if (!c.mnl_pool) {
    MCX_HIP(hipMalloc((void**)&c.mnl_pool, (size_t)(c.mnl_cap * bytes)));
    MCX_HIP(hipMemsetAsync(c.mnl_pool, 0, (size_t)(c.mnl_cap * bytes), c.stream));
    c.device_bytes += c.mnl_cap * bytes;
  }
  if (!micro_nl_grid(c)) {  // micro_mem 1: one workspace of 6 nodal vectors per resident block (two blocks per compute unit)
    c.mnl_ws_blocks = (int)std::min<int64_t>(c.mnl_ws_blocks_opt > 0 ? c.mnl_ws_blocks_opt : 2 * (int64_t)c.ncu, ngp);
    const int64_t nn = (int64_t)a.m.n * a.m.n * a.m.n;
    if (int rc = micro_resize(c, &c.mnl_ws, &c.mnl_ws_bytes,
                              c.micro_mem ? (int64_t)sizeof(double) * c.mnl_ws_blocks * 6 * 3 * nn : 0))
      return rc;
  }
  c.mnl_used += h[0];
  if (micro_nl_grid(c)) {
    if (int rc = micro_resize(c, &c.mnl_ws, &c.mnl_ws_bytes, 0)) return rc;
    if (int rc = mnl_warm_resize(c)) return rc;
    if (int rc = solve_mnl_grid(c, a, h[1])) return rc;
  } else {
    launch_mnl_solve(c, a, h[1]);
  }
  MCX_HIP(hipGetLastError());
  MCX_HIP(hipMemcpyAsync(h, c.mnl_cnt, sizeof(h), hipMemcpyDeviceToHost, c.stream));
  MCX_HIP(hipStreamSynchronize(c.stream));
  if (h[2] > 0) {  // nothing unconverged is used: name the count and the worst point
    std::vector<int> its((size_t)4 * ngp);
    std::vector<double> rn((size_t)2 * ngp);
    MCX_HIP(hipMemcpy(its.data(), c.mnl_its, sizeof(int) * its.size(), hipMemcpyDeviceToHost));
    MCX_HIP(hipMemcpy(rn.data(), c.mnl_rn, sizeof(double) * rn.size(), hipMemcpyDeviceToHost));
    int64_t worst = -1;
    for (int64_t q = 0; q < ngp; q++)
      if (its[2 * ngp + q] && (worst < 0 || !(rn[q] <= rn[worst]))) worst = q;
    const int64_t E = c.g.nelem;
    char buf[520];
    int len = std::snprintf(buf, sizeof(buf),
                  "-mat_law micro_nl: %d of %d micro cells did not converge; worst: Gauss point %lld (%s): %d Newton "
                  "iterations (micro_nl_max_it %d), %d CG iterations (micro_max_it %d), relative residual %.3e > "
                  "micro_nl_rtol %.3e",
                  h[2], h[1], (long long)((worst % E) * 8 + worst / E),
                  its[2 * ngp + worst] == 1 ? "Newton gave up" : "the inner CG did not converge", its[worst],
                  a.nl_max_it, its[ngp + worst], a.m.max_it, rn[worst], a.nl_rtol);
    if (a.nl_start || a.nl_ls > 0)
      std::snprintf(buf + len, sizeof(buf) - (size_t)len,
                    " (micro_nl_start %d, micro_nl_ls %d: %d rejected trials, smallest accepted step %g)", a.nl_start,
                    a.nl_ls, its[3 * ngp + worst], rn[ngp + worst]);
    set_error(buf);
    return 35;
  }
  return 0;
}

// -mat_law external: the registered law fills sig and ctan from eps (see macroc_amd.h)
static int external_homogenize(Ctx& c) {
  const int64_t E = c.g.nelem, ngp = 8 * E;
  if (c.has_dlaw) {
    mcx_gp_batch b{E, ngp, c.eps, c.sig, c.ctan, (void*)c.stream};
    const int rc = c.dlaw.homogenize(c.dlaw.user, &b);
    if (rc) {
      set_error("external device law: homogenize returned " + std::to_string(rc));
      return 6;
    }
    MCX_HIP(hipGetLastError());
    return 0;
  }
  if (!c.has_mpp) return 0;  // values injected with mcx_set_gp_stress / mcx_set_gp_ctan
  // host MicroPP: strains out, per-GP calls in gpi = ie*8 + gp order, stress + tangent back
  c.h_gp.resize((size_t)ngp * 36);
  double* h = c.h_gp.data();
  MCX_HIP(hipMemcpyAsync(h, c.eps, sizeof(double) * 6 * ngp, hipMemcpyDeviceToHost, c.stream));
  MCX_HIP(hipStreamSynchronize(c.stream));
  std::vector<double> soa((size_t)ngp * 6);
  for (int64_t e = 0; e < E; e++)
    for (int gp = 0; gp < 8; gp++) {
      double eps6[6];
      for (int k = 0; k < 6; k++) eps6[k] = h[(int64_t)k * ngp + gp * E + e];
      c.mpp.set_strain3((int)(e * 8 + gp), eps6);
    }
  c.mpp.homogenize();
  for (int64_t e = 0; e < E; e++)
    for (int gp = 0; gp < 8; gp++) {
      double s6[6];
      c.mpp.get_stress3((int)(e * 8 + gp), s6);
      for (int k = 0; k < 6; k++) soa[(size_t)k * ngp + gp * E + e] = s6[k];
    }
  MCX_HIP(hipMemcpyAsync(c.sig, soa.data(), sizeof(double) * 6 * ngp, hipMemcpyHostToDevice, c.stream));
  for (int64_t e = 0; e < E; e++)
    for (int gp = 0; gp < 8; gp++) {
      double c36[36];
      c.mpp.get_ctan3((int)(e * 8 + gp), c36);
      for (int kl = 0; kl < 36; kl++) h[(size_t)kl * ngp + gp * E + e] = c36[kl];
    }
  MCX_HIP(hipMemcpyAsync(c.ctan, h, sizeof(double) * 36 * ngp, hipMemcpyHostToDevice, c.stream));
  MCX_HIP(hipStreamSynchronize(c.stream));  // the staging buffers are reused
  return 0;
}

int mcx_homogenize(void* ctx) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  PhaseTimer t(c, PH_HOMOG);
  if (c.mat.law == MCX_LAW_EXTERNAL) return external_homogenize(c);
  if (c.mat.law == MCX_LAW_MICRO_NL) return micro_nl_homogenize(c);
  if (int rc = ensure_micro(c)) return rc;
  launch_homogenize(c);
  MCX_HIP(hipGetLastError());
  return 0;
} MCX_CATCH

static int need_external(Ctx& c, const char* fn) {
  if (c.mat.law == MCX_LAW_EXTERNAL) return 0;
  set_error(std::string(fn) + ": the context was created without -mat_law external");
  return 7;
}

int mcx_set_micropp(void* ctx, const mcx_micropp_api* api) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  if (int rc = need_external(c, "mcx_set_micropp")) return rc;
  if (api && (!api->set_strain3 || !api->homogenize || !api->get_stress3 || !api->get_ctan3)) {
    set_error("mcx_set_micropp: set_strain3, homogenize, get_stress3 and get_ctan3 are required");
    return 2;
  }
  c.has_mpp = api != nullptr;
  if (api) c.mpp = *api;
  if (api) c.has_dlaw = false;
  return 0;
} MCX_CATCH

int mcx_set_device_law(void* ctx, const mcx_device_law* law) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  if (int rc = need_external(c, "mcx_set_device_law")) return rc;
  if (law && !law->homogenize) {
    set_error("mcx_set_device_law: homogenize is required");
    return 2;
  }
  c.has_dlaw = law != nullptr;
  if (law) c.dlaw = *law;
  if (law) c.has_mpp = false;
  return 0;
} MCX_CATCH

// host [ngp][ncomp] (gpi order) <-> device [ncomp][8][nelem]
static int gp_upload(Ctx& c, const double* host, double* dev, int ncomp) {
  const int64_t E = c.g.nelem, ngp = 8 * E;
  std::vector<double> soa((size_t)ngp * ncomp);
  for (int64_t e = 0; e < E; e++)
    for (int gp = 0; gp < 8; gp++)
      for (int k = 0; k < ncomp; k++) soa[(size_t)k * ngp + gp * E + e] = host[(e * 8 + gp) * ncomp + k];
  MCX_HIP(hipMemcpyAsync(dev, soa.data(), sizeof(double) * soa.size(), hipMemcpyHostToDevice, c.stream));
  MCX_HIP(hipStreamSynchronize(c.stream));
  return 0;
}

int mcx_set_gp_stress(void* ctx, const double* host) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  if (int rc = need_external(c, "mcx_set_gp_stress")) return rc;
  return gp_upload(c, host, c.sig, 6);
} MCX_CATCH

int mcx_set_gp_ctan(void* ctx, const double* host) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  if (int rc = need_external(c, "mcx_set_gp_ctan")) return rc;
  return gp_upload(c, host, c.ctan, 36);
} MCX_CATCH

int mcx_get_gp_strain(void* ctx, double* host) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  const int64_t E = c.g.nelem, ngp = 8 * E;
  std::vector<double> soa((size_t)ngp * 6);
  MCX_HIP(hipMemcpyAsync(soa.data(), c.eps, sizeof(double) * soa.size(), hipMemcpyDeviceToHost, c.stream));
  MCX_HIP(hipStreamSynchronize(c.stream));
  for (int64_t e = 0; e < E; e++)
    for (int gp = 0; gp < 8; gp++)
      for (int k = 0; k < 6; k++) host[(e * 8 + gp) * 6 + k] = soa[(size_t)k * ngp + gp * E + e];
  return 0;
} MCX_CATCH

int mcx_get_gp_ctan(void* ctx, double* host) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  if (!c.ctan) {
    set_error("mcx_get_gp_ctan: this -mat_law has no tangent per Gauss point (plastic, external, micro_nl have)");
    return 7;
  }
  const int64_t E = c.g.nelem, ngp = 8 * E;
  std::vector<double> soa((size_t)ngp * 36);
  MCX_HIP(hipMemcpyAsync(soa.data(), c.ctan, sizeof(double) * soa.size(), hipMemcpyDeviceToHost, c.stream));
  MCX_HIP(hipStreamSynchronize(c.stream));
  for (int64_t e = 0; e < E; e++)
    for (int gp = 0; gp < 8; gp++)
      for (int k = 0; k < 36; k++) host[(e * 8 + gp) * 36 + k] = soa[(size_t)k * ngp + gp * E + e];
  return 0;
} MCX_CATCH

static int need_micro_nl(Ctx& c, const char* fn) {
  if (c.mat.law == MCX_LAW_MICRO_NL) return 0;
  set_error(std::string(fn) + ": the context was created without -mat_law micro_nl");
  return 7;
}

int mcx_micro_nl_get_info(void* ctx, int* path, int* newton_its, int* cg_its, double* rnorm) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  if (int rc = need_micro_nl(c, "mcx_micro_nl_get_info")) return rc;
  const int64_t E = c.g.nelem, ngp = 8 * E;
  std::vector<int> slot((size_t)ngp), its((size_t)3 * ngp);
  std::vector<double> rn((size_t)ngp);
  MCX_HIP(hipMemcpyAsync(slot.data(), c.mnl_slot, sizeof(int) * slot.size(), hipMemcpyDeviceToHost, c.stream));
  MCX_HIP(hipMemcpyAsync(its.data(), c.mnl_its, sizeof(int) * its.size(), hipMemcpyDeviceToHost, c.stream));
  MCX_HIP(hipMemcpyAsync(rn.data(), c.mnl_rn, sizeof(double) * rn.size(), hipMemcpyDeviceToHost, c.stream));
  MCX_HIP(hipStreamSynchronize(c.stream));
  for (int64_t e = 0; e < E; e++)
    for (int gp = 0; gp < 8; gp++) {
      const int64_t q = gp * E + e, i = e * 8 + gp;
      if (path) path[i] = slot[q] >= 0;
      if (newton_its) newton_its[i] = its[q];
      if (cg_its) cg_its[i] = its[ngp + q];
      if (rnorm) rnorm[i] = rn[q];
    }
  return 0;
} MCX_CATCH

int mcx_micro_nl_get_steps(void* ctx, int* ls_rejects, double* min_step) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  if (int rc = need_micro_nl(c, "mcx_micro_nl_get_steps")) return rc;
  const int64_t E = c.g.nelem, ngp = 8 * E;
  std::vector<int> rej((size_t)ngp);
  std::vector<double> ms((size_t)ngp);
  MCX_HIP(hipMemcpyAsync(rej.data(), c.mnl_its + 3 * ngp, sizeof(int) * rej.size(), hipMemcpyDeviceToHost, c.stream));
  MCX_HIP(hipMemcpyAsync(ms.data(), c.mnl_rn + ngp, sizeof(double) * ms.size(), hipMemcpyDeviceToHost, c.stream));
  MCX_HIP(hipStreamSynchronize(c.stream));
  for (int64_t e = 0; e < E; e++)
    for (int gp = 0; gp < 8; gp++) {
      const int64_t q = gp * E + e, i = e * 8 + gp;
      if (ls_rejects) ls_rejects[i] = rej[q];
      if (min_step) min_step[i] = ms[q];
    }
  return 0;
} MCX_CATCH

int mcx_micro_nl_get_pool(void* ctx, int64_t* slots_used, int64_t* slots_allocated, int64_t* bytes_per_slot) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  if (int rc = need_micro_nl(c, "mcx_micro_nl_get_pool")) return rc;
  if (slots_used) *slots_used = c.mnl_used;
  if (slots_allocated) *slots_allocated = c.mnl_pool ? c.mnl_cap : 0;
  if (bytes_per_slot) *bytes_per_slot = c.micro.n >= 2 && c.micro.n <= micro_nmax(c) ? mnl_slot_bytes(c) : 0;
  return 0;
} MCX_CATCH

int mcx_micro_get_ctan(void* ctx, double* C, int* its, double* rnorm) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  if (!micro_law(c.mat.law)) {
    set_error("mcx_micro_get_ctan: the context was created without -mat_law micro");
    return 7;
  }
  if (int rc = ensure_micro(c)) return rc;
  for (int q = 0; q < 36 && C; q++) C[q] = c.mat.C[q];
  for (int l = 0; l < 6; l++) {
    if (its) its[l] = c.micro_its[l];
    if (rnorm) rnorm[l] = c.micro_rnorm[l];
  }
  return 0;
} MCX_CATCH

int mcx_micro_get_phase(void* ctx, unsigned char* phase, int64_t* n) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  if (!micro_law(c.mat.law)) {
    set_error("mcx_micro_get_phase: the context was created without -mat_law micro");
    return 7;
  }
  const int mn = c.micro.n, ne = mn - 1, type = c.micro.type;
  if (int rc = micro_n_refused(c)) return rc;
  if (type != 0 && type != 1) {
    set_error("-mat_law micro: -micro_type " + std::to_string(type) +
              " is not implemented (0: centred sphere, 1: flat layer in y)");
    return 32;
  }
  if (!n) {
    set_error("mcx_micro_get_phase: n is required");
    return 1;
  }
  const int64_t cnt = (int64_t)ne * ne * ne;
  if (phase) {
    if (*n < cnt) {
      set_error("mcx_micro_get_phase: capacity " + std::to_string(*n) + " < " + std::to_string(cnt) + " elements");
      return 2;
    }
    for (int k = 0; k < ne; k++)
      for (int j = 0; j < ne; j++)
        for (int i = 0; i < ne; i++) phase[i + ne * (j + ne * k)] = (unsigned char)micro_phase(type, ne, i, j, k);
  }
  *n = cnt;
  return 0;
} MCX_CATCH

int mcx_assembly_res(void* ctx, double* norm2) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  {
    PhaseTimer t(c, PH_RES);
    launch_residual(c);
    launch_reduce(c, 1, (int)node_blocks(c), c.red);
    MCX_HIP(hipGetLastError());
  }
  double nrm = 0.;
  MCX_HIP(hipMemcpyAsync(&c.h_cg[0].dp, c.red, sizeof(double), hipMemcpyDeviceToHost, c.stream));
  MCX_HIP(hipEventRecord(c.ev_chunk[0], c.stream));
  if (int rc = comm_wait(c, c.ev_chunk[0], "assembly_res (all-reduced |RES|)")) return rc;
  nrm = c.h_cg[0].dp;
  if (norm2) *norm2 = nrm;
  return 0;
} MCX_CATCH

// the AIJ stencil-block storage, allocated on first use when the context started with AIJ-split
static int ensure_V(Ctx& c) {
  if (c.V) return 0;
  return dalloc(c, &c.V, c.ngroups * NPAIR * 128);
}

// the value-indexed storage, allocated on first use
static int ensure_VI(Ctx& c) {
  if (c.vi_dict) return 0;
  const int64_t idx_bytes = 0;  // the index array is sized by build_vi to the mode it picks
  const int64_t nd = std::max(VI_MAX, NSLOT * 16), nk = 2 * VI_HASH + NSLOT * 32;
  MCX_HIP(hipMalloc(&c.vi_dict, nd * sizeof(double)));
  MCX_HIP(hipMalloc(&c.vi_bdict, VI_MAX * VIB_STRIDE * sizeof(double)));
  MCX_HIP(hipMalloc(&c.vi_keys, nk * sizeof(unsigned long long)));
  MCX_HIP(hipMalloc(&c.vi_slot, nk));
  MCX_HIP(hipMalloc(&c.vi_ctl, (5 + NSLOT) * sizeof(unsigned)));
  MCX_HIP(hipMalloc(&c.vib_keys, (NSLOT * VB_GSV + VI_HASH) * sizeof(unsigned long long)));
  MCX_HIP(hipMalloc(&c.vib_ctl, 4 * sizeof(unsigned)));
  MCX_HIP(hipHostMalloc((void**)&c.h_vib_keys, (NSLOT * VB_GSV + VI_HASH + 2) * sizeof(unsigned long long),
                        hipHostMallocDefault));
  MCX_HIP(hipHostMalloc((void**)&c.h_vib_map, VI_HASH, hipHostMallocDefault));
  MCX_HIP(hipHostMalloc((void**)&c.h_vib_dict, VI_MAX * VIB_STRIDE * sizeof(double), hipHostMallocDefault));
  c.device_bytes += idx_bytes + nd * 8 + VI_MAX * VIB_STRIDE * 8 + nk * 9 + (5 + NSLOT) * 4 +
                    (NSLOT * VB_GSV + VI_HASH) * 8 + 16;
  return 0;
}

int mcx_assembly_jac(void* ctx) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  PhaseTimer t(c, PH_JAC);
  int rc;
  c.mg.built = false;  // -pc_type mg: the hierarchy is rebuilt at the next solve or mcx_pc_apply
  if ((rc = ensure_micro(c))) return rc;
  const bool table = gp_tangent_law(c.mat.law);
  const bool try_vi = c.o.mat_type == MCX_MAT_AIJ && c.aij_vi && !c.vi_declined;
  // a per-GP-tangent law headed for the value-indexed storage with exception nodes: kref and the
  // non-plain elements' matrices only (the value-indexed build needs no other element matrix)
  c.plain_ke = false;
  if (table && try_vi && c.vi_exc_max > 0 && c.vi_block_on && c.vi_bits_max == 4 && c.vib_onepass) {
    if ((rc = launch_plain_ke(c))) return rc;
  } else if (table) {
    launch_element_ke(c);  // per-GP tangent: element matrices first
  } else {
    launch_elastic_ke(c);  // one material, one element shape: one element matrix
  }
  if (try_vi) {
    // value-indexed AIJ when the matrix has at most VI_MAX distinct values (the elastic law's
    // matrices; per-GP-tangent laws with few exception nodes); otherwise the next storage below
    bool ok = false;
    if ((rc = ensure_VI(c)) || (rc = build_vi(c, &ok))) return rc;
    if (ok) {
      c.fmt = FMT_VI;
      if ((rc = build_wdesc(c)) || (rc = build_st(c))) return rc;
      c.assembled = true;
      MCX_HIP(hipGetLastError());
      return 0;
    }
    c.vi_declined = table;  // a per-GP tangent stays varied: skip the attempt
    if (c.plain_ke) {       // the storages below sum every element's matrix
      launch_element_ke(c);
      c.plain_ke = false;
    }
  }
  if (c.o.mat_type == MCX_MAT_SBAIJ) {
    launch_gather_matrix_sym(c);
    c.fmt = FMT_U;
  } else if (c.aij_split && !c.split_declined) {
    if (!c.U && (rc = dalloc(c, &c.U, c.npgroups * UPAIR * 128))) return rc;  // first AIJ-split assembly
    launch_gather_matrix_sym(c);
    bool exact = false;
    if ((rc = build_split(c, &exact))) return rc;
    c.fmt = exact ? FMT_SPLIT : FMT_V;
    if (!exact) {  // a correction is not exact, or they are too many: plain AIJ blocks
      if ((rc = ensure_V(c))) return rc;
      launch_gather_matrix(c);
      // a per-GP-tangent law keeps its inexact (or refused dense) corrections: later assemblies
      // go straight to blocks
      c.split_declined = gp_tangent_law(c.mat.law);
    }
  } else {
    if ((rc = ensure_V(c))) return rc;
    launch_gather_matrix(c);
    c.fmt = FMT_V;
  }
  c.assembled = true;
  MCX_HIP(hipGetLastError());
  return 0;
} MCX_CATCH

int mcx_solve(void* ctx, int* its, double* rnorm, int* reason) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  if (!c.assembled) {
    set_error("mcx_solve: no matrix assembled (call mcx_assembly_jac first)");
    return 5;
  }
  int i0 = 0, r0 = 0;
  double n0 = 0.;
  int rc;
  {
    PhaseTimer t(c, PH_SOLVE);
    rc = c.pc_type == 1 ? pcmg_solve(c, &i0, &n0, &r0) : cg_solve(c, &i0, &n0, &r0);
  }
  if (rc) return rc;
  MCX_HIP(hipGetLastError());
  if (its) *its = i0;
  if (rnorm) *rnorm = n0;
  if (reason) *reason = r0;
  return 0;
} MCX_CATCH

int mcx_update_u(void* ctx) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  PhaseTimer t(c, PH_UPDATE);
  launch_update_u(c);
  MCX_HIP(hipGetLastError());
  return 0;
} MCX_CATCH

int mcx_update_vars(void* ctx) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  if (c.hist_old) std::swap(c.hist_old, c.hist_new);
  if (c.mat.law == MCX_LAW_MICRO_NL && c.mnl_pool) {
    launch_mnl_commit(c, mnl_args(c));
    MCX_HIP(hipGetLastError());
  }
  if (c.has_mpp && c.mpp.update_vars) c.mpp.update_vars();
  if (c.has_dlaw && c.dlaw.update_vars) {
    MCX_HIP(hipStreamSynchronize(c.stream));
    if (int rc = c.dlaw.update_vars(c.dlaw.user)) {
      set_error("external device law: update_vars returned " + std::to_string(rc));
      return 6;
    }
  }
  return 0;
} MCX_CATCH

int mcx_get_nonlinear_stats(void* ctx, int64_t* n_nonlinear, double* f_trial_max) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  int64_t n = 0;
  double fm = 0.;
  if (c.has_mpp) {  // the external MicroPP's own counts (over its Gauss points)
    if (c.mpp.get_non_linear_gps) n = c.mpp.get_non_linear_gps();
    if (c.mpp.get_f_trial_max) fm = c.mpp.get_f_trial_max();
  } else if (c.has_dlaw) {
    if (c.dlaw.nonlinear_stats) {
      MCX_HIP(hipStreamSynchronize(c.stream));
      if (int rc = c.dlaw.nonlinear_stats(c.dlaw.user, &n, &fm)) {
        set_error("external device law: nonlinear_stats returned " + std::to_string(rc));
        return 6;
      }
    }
  } else if (c.ftrial) {
    const Geo& g = c.g;
    std::vector<double> ft(8 * g.nelem);
    MCX_HIP(hipMemcpyAsync(ft.data(), c.ftrial, sizeof(double) * ft.size(), hipMemcpyDeviceToHost, c.stream));
    MCX_HIP(hipStreamSynchronize(c.stream));
    int lo[3], hi[3], s[3] = {g.xs, g.ys, g.zs}, w[3] = {g.nx, g.ny, g.nz};
    for (int d = 0; d < 3; d++) {
      lo[d] = s[d] > 0 ? s[d] - 1 : s[d];
      hi[d] = s[d] + w[d] - 2;
    }
    fm = -1e300;
    for (int ez = lo[2]; ez <= hi[2]; ez++)
      for (int ey = lo[1]; ey <= hi[1]; ey++)
        for (int ex = lo[0]; ex <= hi[0]; ex++) {
          int64_t le = (ex - g.ex0) + (int64_t)(ey - g.ey0) * g.nex + (int64_t)(ez - g.ez0) * g.nex * g.ney;
          for (int gp = 0; gp < 8; gp++) {
            double f = ft[gp * g.nelem + le];
            if (f > 0.) n++;
            if (f > fm) fm = f;
          }
        }
  }
  if (n_nonlinear) *n_nonlinear = n;
  if (f_trial_max) *f_trial_max = fm;
  return 0;
} MCX_CATCH

}  // extern "C"

// all-reduce of a few host doubles through red_loc / red (collective; op 0 sum, 1 max)
static int host_allreduce(Ctx& c, double* v, int n, int op) {
  if (c.nranks <= 1 && !c.comm) return 0;
  int rc;
  if ((rc = allreduce_prepare(c))) return rc;
  MCX_HIP(hipMemcpyAsync(c.red_loc, v, sizeof(double) * n, hipMemcpyHostToDevice, c.stream));
  rc = op ? allreduce_max(c, c.red_loc, c.red, n) : allreduce_sum(c, c.red_loc, c.red, n);
  if (rc) return rc;
  MCX_HIP(hipMemcpyAsync(v, c.red, sizeof(double) * n, hipMemcpyDeviceToHost, c.stream));
  MCX_HIP(hipEventRecord(c.ev_chunk[0], c.stream));
  return comm_wait(c, c.ev_chunk[0], op ? "host all-reduce (max)" : "host all-reduce (sum)");
}

extern "C" {

int mcx_reduce_nonlinear(void* ctx, int64_t* n_local, int64_t* n_total, double* f_trial_max) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  int64_t n = 0;
  double fm = 0.;
  int rc = mcx_get_nonlinear_stats(ctx, &n, &fm);
  if (rc) return rc;
  double s = (double)n;  // exact: at most 8 x elements GPs
  if ((rc = host_allreduce(c, &s, 1, 0)) || (rc = host_allreduce(c, &fm, 1, 1))) return rc;
  if (n_local) *n_local = n;
  if (n_total) *n_total = (int64_t)s;
  if (f_trial_max) *f_trial_max = fm;
  return 0;
} MCX_CATCH

int mcx_calc_force(void* ctx, double* force) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  const Geo& g = c.g;
  // the rank's own elements as PETSc lists them (DMDAGetElements): [s - (s > 0), s + w - 1)
  int lo[3], cnt[3];
  const int s[3] = {g.xs, g.ys, g.zs}, w[3] = {g.nx, g.ny, g.nz};
  for (int d = 0; d < 3; d++) {
    lo[d] = s[d] > 0 ? s[d] - 1 : s[d];
    cnt[d] = std::max(0, s[d] + w[d] - 1 - lo[d]);
  }
  double mpi_force = 0.0;
  std::vector<double> ave;
  auto layer = [&](int comp, int fa, int fixed, int a0, int na, int b0, int nb) -> int {
    ave.assign((size_t)na * nb, 0.);
    if (ave.empty()) return 0;
    launch_force_layer(c, comp, fa, fixed, a0, na, b0, nb, c.tmp);
    MCX_HIP(hipMemcpyAsync(ave.data(), c.tmp, sizeof(double) * ave.size(), hipMemcpyDeviceToHost, c.stream));
    MCX_HIP(hipStreamSynchronize(c.stream));
    return 0;
  };
  int rc;
  if (g.bc_type == MCX_BC_BENDING) {
    // calc_force_bending src/forces.c:58-106: ranks owning x = NX-1 (owned corner, :75),
    // their last x layer of elements, ey outer / ez inner, stress_ave[3] * dy * dz
    if (g.xs + g.nx == g.NX && cnt[0] > 0) {
      if ((rc = layer(3, 0, lo[0] + cnt[0] - 1, lo[1], cnt[1], lo[2], cnt[2]))) return rc;
      for (int ey = 0; ey < cnt[1]; ++ey)
        for (int ez = 0; ez < cnt[2]; ++ez) mpi_force += ave[(size_t)ey * cnt[2] + ez] * c.dy * g.dz;
    }
  } else {
    // calc_force_circle src/forces.c:115-166: ghost corners si, sj, sk with the owned ny
    // (:130-133), top element layer, ex outer / ez inner, elements whose centre is inside
    // the radius, stress_ave[1] * dx * dz
    const int si = lo[0], sj = lo[1], sk = lo[2];
    if (sj + g.ny == g.NY && cnt[1] > 0) {
      if ((rc = layer(1, 1, lo[1] + cnt[1] - 1, lo[0], cnt[0], lo[2], cnt[2]))) return rc;
      for (int ex = 0; ex < cnt[0]; ++ex)
        for (int ez = 0; ez < cnt[2]; ++ez) {
          const double x = g.lx / 2. - ((si + ex) * g.dx + g.dx / 2.);
          const double z = g.lz / 2. - ((sk + ez) * g.dz + g.dz / 2.);
          if ((x * x + z * z) < 1 * (g.rad * g.rad)) mpi_force += ave[(size_t)ex * cnt[2] + ez] * g.dx * g.dz;
        }
    }
  }
  // MPI_Reduce(SUM) src/forces.c:47 (here every rank receives the total)
  if ((rc = host_allreduce(c, &mpi_force, 1, 0))) return rc;
  if (force) *force = mpi_force;
  return 0;
} MCX_CATCH

int mcx_time_step(void* ctx, int time_s, int* newton_its, double* res, int* ksp_its, double* ksp_rnorm) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  int rc;
  double U = mcx_get_displacement(ctx, time_s);
  if ((rc = mcx_apply_bc_u(ctx, U))) return rc;
  double norm = 0., norm_0 = 0.;
  int it = 0;
  while (it < c.o.newton_max_its) {
    if ((rc = mcx_set_strains(ctx)) || (rc = mcx_homogenize(ctx)) || (rc = mcx_assembly_res(ctx, &norm))) return rc;
    if (res) res[it] = norm;
    if (it == 0) norm_0 = norm;
    if (norm < c.o.newton_min_tol || norm < norm_0 * c.o.newton_rel_tol) break;
    int kits = 0, reason = 0;
    double rn = 0.;
    if ((rc = mcx_assembly_jac(ctx)) || (rc = mcx_solve(ctx, &kits, &rn, &reason)) || (rc = mcx_update_u(ctx)))
      return rc;
    if (ksp_its) ksp_its[it] = kits;
    if (ksp_rnorm) ksp_rnorm[it] = rn;
    it++;
  }
  if (newton_its) *newton_its = it;
  if ((rc = mcx_update_vars(ctx))) return rc;  // src/main.c:83
  MCX_HIP(hipEventRecord(c.ev_chunk[0], c.stream));
  return comm_wait(c, c.ev_chunk[0], "time step end");
} MCX_CATCH

// ---------------------------------------------------------------- data access
int mcx_get_u(void* ctx, double* host) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  launch_copy_pad_to_owned(c, c.u_pad, c.tmp);
  MCX_HIP(hipMemcpyAsync(host, c.tmp, sizeof(double) * 3 * c.g.nown, hipMemcpyDeviceToHost, c.stream));
  MCX_HIP(hipStreamSynchronize(c.stream));
  return 0;
} MCX_CATCH

int mcx_set_u(void* ctx, const double* host) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  MCX_HIP(hipMemcpyAsync(c.tmp, host, sizeof(double) * 3 * c.g.nown, hipMemcpyHostToDevice, c.stream));
  launch_copy_owned_to_pad(c, c.tmp, c.u_pad);
  MCX_HIP(hipStreamSynchronize(c.stream));
  return 0;
} MCX_CATCH

static int get_owned(Ctx& c, const double* d, double* host) {
  MCX_HIP(hipMemcpyAsync(host, d, sizeof(double) * 3 * c.g.nown, hipMemcpyDeviceToHost, c.stream));
  MCX_HIP(hipStreamSynchronize(c.stream));
  return 0;
}

int mcx_get_b(void* ctx, double* host) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  return get_owned(c, c.b, host);
} MCX_CATCH

int mcx_get_du(void* ctx, double* host) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  return get_owned(c, c.du, host);
} MCX_CATCH

static int get_gp(Ctx& c, const double* d, double* host) {
  const Geo& g = c.g;
  const int64_t E = g.nelem;
  std::vector<double> all(6 * 8 * E);
  MCX_HIP(hipMemcpyAsync(all.data(), d, sizeof(double) * all.size(), hipMemcpyDeviceToHost, c.stream));
  MCX_HIP(hipStreamSynchronize(c.stream));
  // PETSc-owned elements: lower-left node in [xs - (xs>0), xe - 2] per direction
  int lo[3], hi[3], s[3] = {g.xs, g.ys, g.zs}, w[3] = {g.nx, g.ny, g.nz};
  for (int dd = 0; dd < 3; dd++) {
    lo[dd] = s[dd] > 0 ? s[dd] - 1 : s[dd];
    hi[dd] = s[dd] + w[dd] - 2;
  }
  int64_t ie = 0;
  for (int ez = lo[2]; ez <= hi[2]; ez++)
    for (int ey = lo[1]; ey <= hi[1]; ey++)
      for (int ex = lo[0]; ex <= hi[0]; ex++, ie++) {
        int64_t le = (ex - g.ex0) + (int64_t)(ey - g.ey0) * g.nex + (int64_t)(ez - g.ez0) * g.nex * g.ney;
        for (int gp = 0; gp < 8; gp++)
          for (int k = 0; k < 6; k++) host[(ie * 8 + gp) * 6 + k] = all[((int64_t)k * 8 + gp) * E + le];
      }
  return 0;
}

int mcx_get_strain(void* ctx, double* host) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  return get_gp(c, c.eps, host);
} MCX_CATCH

int mcx_get_stress(void* ctx, double* host) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  return get_gp(c, c.sig, host);
} MCX_CATCH

int mcx_owned_dofs(void* ctx, int64_t* petsc, int64_t* natural) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  const Geo& g = c.g;
  const int64_t off = 3 * c.rank_node_off[c.rank];
  for (int64_t n = 0; n < g.nown; n++) {
    int64_t i = n % g.nx, j = (n / g.nx) % g.ny, k = n / ((int64_t)g.nx * g.ny);
    int64_t nat = (g.xs + i) + (g.ys + j) * (int64_t)g.NX + (g.zs + k) * (int64_t)g.NX * g.NY;
    for (int d = 0; d < 3; d++) {
      if (petsc) petsc[3 * n + d] = off + 3 * n + d;
      if (natural) natural[3 * n + d] = 3 * nat + d;
    }
  }
  return 0;
} MCX_CATCH

int mcx_dump_csr(void* ctx, int64_t* rowptr, int64_t* colidx, double* vals) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  if (vals && !c.assembled) {
    set_error("mcx_dump_csr: no matrix assembled (call mcx_assembly_jac first)");
    return 5;
  }
  const Geo& g = c.g;
  const bool up = c.fmt == FMT_U || c.fmt == FMT_SPLIT;  // values from the upper blocks
  std::vector<double> V;
  std::vector<uint16_t> Dh;
  std::vector<unsigned char> Ih;
  std::vector<double> dict;
  std::vector<double> Xh;  // exception nodes' blocks
  if (vals && c.fmt == FMT_VI && c.vi_block && c.vi_nexc) {  // AoSoA (exc_base)
    Xh.resize((size_t)c.g.xld * 27 * 9);
    MCX_HIP(hipMemcpyAsync(Xh.data(), c.vi_exc, Xh.size() * sizeof(double), hipMemcpyDeviceToHost, c.stream));
  }
  if (vals && c.fmt == FMT_VI) {
    Ih.resize((size_t)c.vi_idx_bytes);
    dict.resize(c.vi_block ? VI_MAX * VIB_STRIDE : std::max(VI_MAX, NSLOT * 16));
    MCX_HIP(hipMemcpyAsync(Ih.data(), c.vi_idx, Ih.size(), hipMemcpyDeviceToHost, c.stream));
    MCX_HIP(hipMemcpyAsync(dict.data(), c.vi_block ? c.vi_bdict : c.vi_dict, dict.size() * sizeof(double),
                           hipMemcpyDeviceToHost, c.stream));
    MCX_HIP(hipStreamSynchronize(c.stream));
  } else if (vals) {
    V.resize(up ? c.npgroups * UPAIR * 128 : c.ngroups * NPAIR * 128);
    MCX_HIP(hipMemcpyAsync(V.data(), up ? c.U : c.V, sizeof(double) * V.size(), hipMemcpyDeviceToHost, c.stream));
    if (c.fmt == FMT_SPLIT && c.dsl.L) {
      Dh.resize((size_t)c.npgroups * c.dsl.Lq * 64 * 8);
      MCX_HIP(hipMemcpyAsync(Dh.data(), c.D, sizeof(uint16_t) * Dh.size(), hipMemcpyDeviceToHost, c.stream));
    }
    MCX_HIP(hipStreamSynchronize(c.stream));
  }
  // AIJ-split escapes: residual of (owned node, slot) added to its bf16 hi
  std::unordered_map<int64_t, double> escmap;
  if (vals && c.fmt == FMT_SPLIT && c.dsl.esc && c.dsl.nesc) {
    std::vector<unsigned> en(g.nown);
    std::vector<double> er(c.dsl.nesc);
    std::vector<unsigned char> es(c.dsl.nesc);
    MCX_HIP(hipMemcpyAsync(en.data(), c.esc_node, sizeof(unsigned) * en.size(), hipMemcpyDeviceToHost, c.stream));
    MCX_HIP(hipMemcpyAsync(er.data(), c.esc_res, sizeof(double) * er.size(), hipMemcpyDeviceToHost, c.stream));
    MCX_HIP(hipMemcpyAsync(es.data(), c.esc_slot, es.size(), hipMemcpyDeviceToHost, c.stream));
    MCX_HIP(hipStreamSynchronize(c.stream));
    for (int64_t n = 0; n < g.nown; n++)
      if (en[n]) {
        const unsigned m = en[n] >> 24, base = (en[n] & 0xffffffu) - 1u;
        for (unsigned t = 0; t < m; t++) escmap[n * 128 + es[base + t]] = er[base + t];
      }
  }
  auto escres = [&](int64_t n, int s, double& v) -> bool {
    if (escmap.empty()) return false;
    auto it = escmap.find(n * 128 + s);
    if (it == escmap.end()) return false;
    v = it->second;
    return true;
  };
  // AIJ-split: packed position of each correction slot (-1: no correction stored), stored with
  // the row node (u_of index): nb*9 + r*3 + c
  int dpos[126];
  for (int s = 0; s < 126; s++) dpos[s] = -1;
  for (int p = 0; p < c.dsl.L; p++) dpos[c.dsl.s[p]] = p;
  auto corr = [&](int64_t u, int s) -> double {
    const int p = dpos[s];
    if (p < 0) return 0.;
    const int per = c.dsl.wide ? 4 : 8;
    const int64_t q = ((u >> 6) * c.dsl.Lq + p / per) * 64 + (u & 63);
    uint32_t f = c.dsl.wide ? (uint32_t)Dh[q * 8 + 2 * (p % 4)] | ((uint32_t)Dh[q * 8 + 2 * (p % 4) + 1] << 16)
                            : (uint32_t)Dh[q * 8 + p % 8] << 16;
    float fv;
    std::memcpy(&fv, &f, 4);
    return (double)fv;
  };
  auto uval = [&](int64_t p, int s) { return V[(p >> 6) * (UPAIR * 128) + (int64_t)(s >> 1) * 128 + 2 * (p & 63) + (s & 1)]; };
  int64_t pos = 0;
  if (rowptr) rowptr[0] = 0;
  std::vector<std::pair<int64_t, double>> row;
  for (int64_t n = 0; n < g.nown; n++) {
    int64_t i = n % g.nx, j = (n / g.nx) % g.ny, k = n / ((int64_t)g.nx * g.ny);
    int64_t gi = g.xs + i, gj = g.ys + j, gk = g.zs + k;
    for (int r = 0; r < 3; r++) {
      row.clear();
      for (int nb = 0; nb < 27; nb++) {
        int64_t hi = gi + nb % 3 - 1, hj = gj + (nb / 3) % 3 - 1, hk = gk + nb / 9 - 1;
        if (hi < 0 || hj < 0 || hk < 0 || hi >= g.NX || hj >= g.NY || hk >= g.NZ) continue;
        int64_t col0 = 3 * petsc_node(c, hi, hj, hk);
        for (int cc = 0; cc < 3; cc++) {
          double v = 0.;
          if (vals && up) {
            // storage index u_of (kernels.hip): 64-aligned rows of UX nodes
            const int64_t pc = 64 + i + (j + 1) * (int64_t)g.UX + (k + 1) * (int64_t)g.UXY;
            const int64_t q = pc + (nb % 3 - 1) + ((nb / 3) % 3 - 1) * (int64_t)g.UX + (nb / 9 - 1) * (int64_t)g.UXY;
            static const int dsl[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
            double er = 0.;
            if (nb < 13) {
              v = uval(q, 6 + 9 * (12 - nb) + cc * 3 + r);
              if (c.fmt == FMT_SPLIT) {  // exact AIJ lower value (an escape: mirror + (hi + residual))
                const int s = nb * 9 + r * 3 + cc;
                v = escres(n, s, er) ? v + (corr(pc, s) + er) : v + corr(pc, s);
              }
            }
            else if (nb == 13) {
              v = uval(pc, dsl[r][cc]);
              if (c.fmt == FMT_SPLIT && r > cc) {  // lower triangle
                const int s = 13 * 9 + r * 3 + cc;
                v = escres(n, s, er) ? v + (corr(pc, s) + er) : v + corr(pc, s);
              }
            }
            else v = uval(pc, 6 + 9 * (nb - 14) + r * 3 + cc);
          } else if (vals && c.fmt == FMT_VI) {
            const int s = nb * 9 + r * 3 + cc;
            if (c.vi_block) {  // byte nb of 2 chunks of 16 B: the block's dictionary entry
              uint32_t xs = 0;  // exception slot + 1 in bytes 28-31
              std::memcpy(&xs, &Ih[(((n >> 6) * 2 + 1) * 64 + (n & 63)) * 16 + 12], 4);
              if (xs && !Xh.empty()) v = Xh[exc_base(xs - 1) + (nb * 9 + r * 3 + cc) * 64];
              else v = dict[Ih[(((n >> 6) * 2 + (nb >> 4)) * 64 + (n & 63)) * 16 + (nb & 15)] * VIB_STRIDE + r * 3 + cc];
            } else if (c.vi_bits == 8) {
              v = dict[Ih[(((n >> 6) * VI_CHUNKS + (s >> 4)) * 64 + (n & 63)) * 16 + (s & 15)]];
            } else {  // nibble s of 8 chunks of 16 B, low nibble first
              const unsigned char byte = Ih[(((n >> 6) * 8 + (s >> 5)) * 64 + (n & 63)) * 16 + ((s & 31) >> 1)];
              v = dict[s * 16 + ((s & 1) ? byte >> 4 : byte & 15)];
            }
          } else if (vals) {
            int s = nb * 9 + r * 3 + cc;
            v = V[(n >> 6) * (NPAIR * 128) + (int64_t)(s >> 1) * 128 + 2 * (n & 63) + (s & 1)];
          }
          row.emplace_back(col0 + cc, v);
        }
      }
      std::sort(row.begin(), row.end(), [](auto& a, auto& b) { return a.first < b.first; });
      for (auto& e : row) {
        if (colidx) colidx[pos] = e.first;
        if (vals) vals[pos] = e.second;
        pos++;
      }
      if (rowptr) rowptr[3 * n + r + 1] = pos;
    }
  }
  return 0;
} MCX_CATCH

int mcx_dump_dirichlet(void* ctx, int64_t* idx, int64_t* n) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  const Geo& g = c.g;
  const int64_t off = 3 * c.rank_node_off[c.rank];
  int64_t cnt = 0;
  for (int64_t q = 0; q < g.nown; q++) {
    int i = (int)(q % g.nx), j = (int)((q / g.nx) % g.ny), k = (int)(q / ((int64_t)g.nx * g.ny));
    int m = dirichlet_mask_host(g, g.xs + i, g.ys + j, g.zs + k);
    for (int d = 0; d < 3; d++)
      if (m >> d & 1) {
        if (idx && cnt < *n) idx[cnt] = off + 3 * q + d;
        cnt++;
      }
  }
  if (idx && cnt > *n) {
    *n = cnt;
    set_error("mcx_dump_dirichlet: capacity too small");
    return 4;
  }
  *n = cnt;
  return 0;
} MCX_CATCH

int mcx_spmv(void* ctx, const double* x_host, double* y_host) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  if (!c.assembled) {
    set_error("mcx_spmv: no matrix assembled (call mcx_assembly_jac first)");
    return 5;
  }
  MCX_HIP(hipMemcpyAsync(c.tmp, x_host, sizeof(double) * 3 * c.g.nown, hipMemcpyHostToDevice, c.stream));
  launch_copy_owned_to_pad(c, c.tmp, c.p_pad);
  int rc = halo_exchange(c, c.p_pad);
  if (rc) return rc;
  launch_spmv(c, c.p_pad, c.tmp, false, false);
  MCX_HIP(hipGetLastError());
  MCX_HIP(hipMemcpyAsync(y_host, c.tmp, sizeof(double) * 3 * c.g.nown, hipMemcpyDeviceToHost, c.stream));
  MCX_HIP(hipStreamSynchronize(c.stream));
  return 0;
} MCX_CATCH

int mcx_pc_apply(void* ctx, const double* r_host, double* z_host) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  if (!c.assembled) {
    set_error("mcx_pc_apply: no matrix assembled (call mcx_assembly_jac first)");
    return 5;
  }
  const int64_t n3 = 3 * (int64_t)c.g.nown;
  MCX_HIP(hipMemcpyAsync(c.tmp, r_host, sizeof(double) * n3, hipMemcpyHostToDevice, c.stream));
  if (c.pc_type == 1) {
    int rc = pcmg_apply(c, c.tmp);
    if (rc) return rc;
    launch_copy_pad_to_owned(c, c.mg.L[0].x.as<double>(), c.tmp);
  } else {
    launch_jacobi(c);
    launch_pcmg_jacobi(c, n3, c.tmp, c.dinv, c.w);
  }
  MCX_HIP(hipGetLastError());
  MCX_HIP(hipMemcpyAsync(z_host, c.pc_type == 1 ? c.tmp : c.w, sizeof(double) * n3, hipMemcpyDeviceToHost, c.stream));
  MCX_HIP(hipStreamSynchronize(c.stream));
  return 0;
} MCX_CATCH

int mcx_pc_mg_info(void* ctx, int* nlevels, int64_t* nxyz, double* lmax, int64_t* bytes) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  if (nlevels) *nlevels = 0;
  if (bytes) *bytes = 0;
  if (c.pc_type != 1) return 0;
  if (c.assembled) {
    int rc = pcmg_ensure(c);
    if (rc) return rc;
  }
  int n[PCMG_MAXLEV][3], nl = 0;
  pcmg_dims(c, c.pc_mg_levels, &nl, n);
  if (nlevels) *nlevels = nl;
  for (int l = 0; l < PCMG_MAXLEV; l++) {
    for (int a = 0; a < 3; a++)
      if (nxyz) nxyz[3 * l + a] = l < nl ? n[l][a] : 0;
    if (lmax) lmax[l] = l < nl && c.mg.built ? c.mg.L[l].lmax : 0.;
  }
  if (bytes) *bytes = c.mg.bytes;
  return 0;
} MCX_CATCH

int mcx_pc_mg_dump_csr(void* ctx, int level, int64_t* rowptr, int64_t* colidx, double* vals) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  if (c.pc_type != 1 || !c.assembled) {
    set_error("mcx_pc_mg_dump_csr: needs pc_type 1 and an assembled matrix");
    return 5;
  }
  int rc = pcmg_ensure(c);
  if (rc) return rc;
  if (level < 1 || level >= c.mg.nlev) {
    set_error("mcx_pc_mg_dump_csr: level 1 .. " + std::to_string(c.mg.nlev - 1));
    return 2;
  }
  // rows: the rank's owned coarse nodes in the natural order of its box; columns: the level's global
  // natural numbering (one rank: the same thing)
  const PcmgLevel& v = c.mg.L[level];
  std::vector<double> blk;
  if (vals) {  // a float level's values widened (exactly)
    blk.resize((size_t)243 * v.nn);
    std::vector<float> blk32(v.f32 ? blk.size() : 0);
    MCX_HIP(hipMemcpyAsync(v.f32 ? (void*)blk32.data() : (void*)blk.data(), v.A.p,
                           (v.f32 ? sizeof(float) : sizeof(double)) * blk.size(), hipMemcpyDeviceToHost, c.stream));
    MCX_HIP(hipStreamSynchronize(c.stream));
    for (size_t q = 0; q < blk32.size(); q++) blk[q] = blk32[q];
  }
  int64_t pos = 0;
  if (rowptr) rowptr[0] = 0;
  for (int64_t p = 0; p < v.nn; p++) {
    const int i = (int)(p % v.n[0]) + v.s[0], j = (int)((p / v.n[0]) % v.n[1]) + v.s[1],
              k = (int)(p / ((int64_t)v.n[0] * v.n[1])) + v.s[2];
    for (int r = 0; r < 3; r++) {
      for (int nb = 0; nb < 27; nb++) {  // ascending neighbour = ascending column
        const int ii = i + nb % 3 - 1, jj = j + (nb / 3) % 3 - 1, kk = k + nb / 9 - 1;
        if (ii < 0 || jj < 0 || kk < 0 || ii >= v.N[0] || jj >= v.N[1] || kk >= v.N[2]) continue;
        const int64_t q = ii + (int64_t)v.N[0] * (jj + (int64_t)v.N[1] * kk);
        for (int cc = 0; cc < 3; cc++) {
          if (colidx) colidx[pos] = 3 * q + cc;
          if (vals) vals[pos] = blk[(size_t)(nb * 9 + r * 3 + cc) * v.nn + p];
          pos++;
        }
      }
      if (rowptr) rowptr[3 * p + r + 1] = pos;
    }
  }
  return 0;
} MCX_CATCH

// host-only: the box of rank `rank` of the rank grid o->px x py x pz on every level
int mcx_pc_mg_plan(const mcx_opts* o, int rank, int levels, int* nlevels, int64_t* start, int64_t* count) try {
  MCX_ENTRY();
  if (!o || o->px < 1 || o->py < 1 || o->pz < 1 || levels < 0 || levels == 1 || levels > PCMG_MAXLEV) {
    set_error("mcx_pc_mg_plan: needs options with the rank grid given (-da_processors_x/y/z >= 1) and levels 0 or 2 .. " +
              std::to_string(PCMG_MAXLEV));
    return 1;
  }
  if (o->NX < 2 || o->NY < 2 || o->NZ < 2 || o->NX > INT32_MAX || o->NY > INT32_MAX || o->NZ > INT32_MAX) {
    set_error("mcx_pc_mg_plan: grid needs 2 .. 2^31 - 1 nodes per direction");
    return 1;
  }
  const int N0[3] = {(int)o->NX, (int)o->NY, (int)o->NZ}, mnp[3] = {o->px, o->py, o->pz};
  if (rank < 0 || rank >= mnp[0] * mnp[1] * mnp[2]) {
    set_error("mcx_pc_mg_plan: rank outside the rank grid");
    return 1;
  }
  PcmgPlan P;
  std::string err;
  if (int rc = pcmg_plan_checked(N0, mnp, rank, levels, &P, &err)) {
    set_error(err);
    return rc;
  }
  if (nlevels) *nlevels = P.nlev;
  for (int l = 0; l < PCMG_MAXLEV; l++)
    for (int a = 0; a < 3; a++) {
      if (start) start[3 * l + a] = l < P.nlev ? P.s[l][a] : 0;
      if (count) count[3 * l + a] = l < P.nlev ? P.n[l][a] : 0;
    }
  return 0;
} MCX_CATCH

int mcx_pc_mg_box(void* ctx, int level, int64_t* start, int64_t* count) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  PcmgPlan P;
  if (int rc = pcmg_plan_ctx(c, c.pc_mg_levels, &P)) return rc;
  if (level < 0 || level >= P.nlev) {
    set_error("mcx_pc_mg_box: level 0 .. " + std::to_string(P.nlev - 1));
    return 2;
  }
  for (int a = 0; a < 3; a++) {
    if (start) start[a] = P.s[level][a];
    if (count) count[a] = P.n[level][a];
  }
  return 0;
} MCX_CATCH

int mcx_get_ksp_history(void* ctx, double* hist, int64_t* n) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  int64_t have = (int64_t)c.last_hist.size();
  int64_t k = std::min(have, *n);
  if (hist) std::memcpy(hist, c.last_hist.data(), sizeof(double) * k);
  *n = have;
  return 0;
} MCX_CATCH

int mcx_set_timing(void* ctx, int on) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  c.timing = on != 0;
  return 0;
} MCX_CATCH

int mcx_get_timing(void* ctx, mcx_timing* t) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  MCX_HIP(hipStreamSynchronize(c.stream));
  double* ph[6] = {&c.t.strains_ms, &c.t.homogenize_ms, &c.t.residual_ms, &c.t.jacobian_ms, &c.t.solve_ms,
                   &c.t.update_ms};
  for (int k = 0; k < 6; k++)
    if (c.phase_rec[k]) {
      float ms = 0.f;
      MCX_HIP(hipEventElapsedTime(&ms, c.ev_phase[k][0], c.ev_phase[k][1]));
      *ph[k] = ms;
    }
  *t = c.t;
  // algorithmic bytes of one SpMV in this format: the stencil-block values actually present
  // (AIJ nonzeros of the owned rows x 8 B), x read once, y written once
  // (value-indexed: vi_bits per nonzero; the pad up to whole 16-B chunks per node is not counted)
  t->spmv_bytes_per_launch =
      (c.fmt == FMT_V    ? c.nnz_local * 8
       : c.fmt == FMT_VI ? (c.vi_block ? c.nnz_local / 9 : (c.nnz_local * c.vi_bits + 7) / 8)
                         : c.nupper_local * 8) +
      2 * 3 * (int64_t)c.g.nown * 8;
  if (c.fmt == FMT_SPLIT) t->spmv_bytes_per_launch += (int64_t)c.g.nown * c.dsl.Lq * 16;
  if (c.fmt == FMT_VI && c.vi_block) t->spmv_bytes_per_launch += c.vi_nexc * 27 * 9 * 8;  // exception blocks
  if (st_used(c)) {  // default stencil: no index bytes but the listed nodes'; the patch masks
    t->spmv_bytes_per_launch += c.st_n * 32 - c.nnz_local / 9 + (int64_t)c.st_npx * c.st_npy * c.g.nz * 8;
  } else if (wd_used(c)) {  // wave descriptors: 128 B per wave and plane, index bytes for the waves that still read per-lane words
    const int64_t nwp = (int64_t)c.wd_npx * c.wd_npy * c.g.nz;
    t->spmv_bytes_per_launch += nwp * 128 - c.nnz_local / 9 +
                                (!c.vi_fma ? c.wd_blocks_exact : c.vi_wdesc == 2 ? c.wd_blocks_two : c.wd_blocks_fma);
  }
  // the fused p update (cg_fusep): r and the diagonal index read, p(i) written
  if (c.fusep_used) t->spmv_bytes_per_launch += (int64_t)c.g.nown * (24 + 1 + 24);
  t->cg_vec_bytes_per_iter = cg_vec_bytes_per_node(c) * (int64_t)c.g.nown;
  return 0;
} MCX_CATCH

int mcx_set_option(void* ctx, const char* name, double value) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  if (!std::strcmp(name, "micro_rtol")) {  // -mat_law micro: the cell's CG stopping rule; C_hom is recomputed
    if (!(value > 0.)) {
      set_error("micro_rtol: > 0");
      return 1;
    }
    c.micro.rtol = value;
    c.micro_dirty = true;
    return 0;
  }
  if (!std::strcmp(name, "micro_nl_rtol")) {  // -mat_law micro_nl: the cell's Newton stopping rule
    if (!(value > 0.)) {
      set_error("micro_nl_rtol: > 0");
      return 1;
    }
    c.mnl_rtol = value;
    return 0;
  }
  if (!std::strcmp(name, "micro_nl_max_it")) {
    if (!(value >= 1.)) {
      set_error("micro_nl_max_it: >= 1");
      return 1;
    }
    c.mnl_max_it = (int)value;
    return 0;
  }
  if (!std::strcmp(name, "micro_nl_start")) {  // the cell's first Newton iterate; other laws: no effect
    if (value != 0. && value != 1.) {
      set_error("micro_nl_start: 0 (zero: the boundary values, 0 inside) or 1 (elastic: the superposed unit-strain fields inside)");
      return 1;
    }
    c.mnl_start = (int)value;
    return 0;
  }
  if (!std::strcmp(name, "micro_nl_ls")) {  // the Newton step's lengths 2^-j, j = 0 .. K; 0: full steps
    if (!(value >= 0. && value <= 16.) || value != (double)(int)value) {
      set_error("micro_nl_ls: an integer 0 (full Newton steps) .. 16 (step lengths down to 2^-16)");
      return 1;
    }
    c.mnl_ls = (int)value;
    return 0;
  }
  if (!std::strcmp(name, "micro_nl_slots")) {  // 0: what fits 2 GiB, at most the local Gauss points
    if (!(value >= 0.)) {
      set_error("micro_nl_slots: >= 0");
      return 1;
    }
    c.mnl_slots_opt = (int64_t)value;
    return 0;
  }
  if (!std::strcmp(name, "micro_max_it")) {  // 0: 10 x the interior dofs
    c.micro_max_it = std::max(0, (int)value);
    c.micro_dirty = true;
    return 0;
  }
  if (!std::strcmp(name, "micro_mem_blocks")) {  // testing: micro_mem 1's workspaces (0: 2 x compute units)
    if (!(value >= 0.) || value > 65535.) {
      set_error("micro_mem_blocks: 0 .. 65535");
      return 1;
    }
    c.mnl_ws_blocks_opt = (int)value;
    return 0;
  }
  if (!std::strcmp(name, "micro_mem")) {  // where the cell solvers' nodal vectors live: 0 LDS, 1 device memory
    if (value != 0. && value != 1.) {
      set_error("micro_mem: 0 (the cell solvers' vectors in LDS, micro_n <= " + std::to_string(MICRO_NMAX) +
                ") or 1 (in device memory, micro_n <= " + std::to_string(MICRO_NMAX_DEV) + ")");
      return 1;
    }
    if ((int)value == c.micro_mem) return 0;
    if (c.mnl_used > 0) {  // the histories would outlive the solver that wrote them
      set_error("micro_mem: " + std::to_string(c.mnl_used) +
                " history slots are in use; the memory mode is chosen before the first non-linear point");
      return 2;
    }
    c.micro_mem = (int)value;
    c.micro_dirty = true;  // C_hom and the concentration tensors are recomputed, the workspaces resized
    return 0;
  }
  if (!std::strcmp(name, "micro_solver")) {  // who solves the six unit-strain problems of -mat_law micro
    if (value != 0. && value != 1.) {
      set_error("micro_solver: 0 (one workgroup per load case, micro_n <= " + std::to_string(MICRO_NMAX) + " / " +
                std::to_string(MICRO_NMAX_DEV) + " by micro_mem) or 1 (grid-wide, one workgroup per tile, micro_n <= " +
                std::to_string(MICRO_NMAX_GRID) + ")");
      return 1;
    }
    if ((int)value == c.micro_solver) return 0;
    if (value == 1. && c.mat.law == MCX_LAW_MICRO_NL) {
      set_error("micro_solver 1: not with -mat_law micro_nl (its linear shortcut needs the unit-strain fields and its "
                "per-point solver ends at micro_n " + std::to_string(MICRO_NMAX_DEV) + ")");
      return 2;
    }
    c.micro_solver = (int)value;
    c.micro_dirty = true;  // C_hom is recomputed by the other solver
    if (!c.micro_solver) return micro_resize(c, &c.micro_grid_ws, &c.micro_grid_bytes, 0);
    return 0;
  }
  if (!std::strcmp(name, "micro_nl_solver")) {  // who solves the cells of -mat_law micro_nl
    if (value != 0. && value != 1.) {
      set_error("micro_nl_solver: 0 (one workgroup per Gauss point, micro_n <= " + std::to_string(MICRO_NMAX) + " / " +
                std::to_string(MICRO_NMAX_DEV) + " by micro_mem) or 1 (grid-wide, one workgroup per tile, micro_n <= " +
                std::to_string(MICRO_NMAX_NL_GRID) + ")");
      return 1;
    }
    if ((int)value == c.mnl_solver) return 0;
    if (c.mnl_used > 0) {  // the histories would outlive the solver that wrote them
      set_error("micro_nl_solver: " + std::to_string(c.mnl_used) +
                " history slots are in use; the solver is chosen before the first non-linear point");
      return 2;
    }
    c.mnl_solver = (int)value;
    if (c.mat.law != MCX_LAW_MICRO_NL) return 0;  // accepted, no effect
    c.micro_dirty = true;  // C_hom and the concentration tensors are recomputed by the other solver
    if (!c.mnl_solver) return micro_resize(c, &c.micro_grid_ws, &c.micro_grid_bytes, 0);
    return 0;
  }
  if (!std::strcmp(name, "micro_nl_tangent")) {  // how solver 1 runs a point's six tangent columns
    if (value != 0. && value != 1.) {
      set_error("micro_nl_tangent: 0 (seq: the six tangent columns one after the other) or 1 (block: micro_nl_solver 1 "
                "advances them together, 26 vectors of 3 micro_n^3 per solve in flight)");
      return 1;
    }
    if ((int)value == c.mnl_tangent) return 0;
    if (c.mnl_used > 0) {  // the workspace's layout follows the option: micro_nl_solver's rule
      set_error("micro_nl_tangent: " + std::to_string(c.mnl_used) +
                " history slots are in use; the tangent solves are chosen before the first non-linear point");
      return 2;
    }
    c.mnl_tangent = (int)value;  // solver 0 and the other laws: accepted, no effect
    // solver 1: the workspace follows the option (grid_ws_bytes), now if there is one, else at the next solve
    if (micro_nl_grid(c) && c.micro_grid_ws) return micro_resize(c, &c.micro_grid_ws, &c.micro_grid_bytes, grid_ws_bytes(c));
    return 0;
  }
  if (!std::strcmp(name, "micro_nl_apply")) {  // how solver 1 forms a CG iteration's q = K_T p
    if (value != 0. && value != 1.) {
      set_error("micro_nl_apply: 0 (split: the Gauss-point pass writes the work stresses, the node gather reads them) or 1 "
                "(fused: micro_nl_solver 1 forms q = K_T p and p.q in one launch, no work stresses written)");
      return 1;
    }
    c.mnl_apply = (int)value;  // neither the workspace nor the slots follow it: any time; solver 0 and the other laws: no effect
    return 0;
  }
  if (!std::strcmp(name, "micro_nl_warm")) {  // solver 1 starts a slotted point from its last solution
    if (value != 0. && value != 1.) {
      set_error("micro_nl_warm: 0 (off: every cell solve starts as micro_nl_start says) or 1 (on: micro_nl_solver 1 starts a "
                "slotted point's Newton loop and tangent columns from the slot's last converged solution)");
      return 1;
    }
    c.mnl_warm = (int)value;  // any time; the store follows at the next solve; solver 0 and the other laws: no effect
    if (!c.mnl_warm) {
      c.mnl_warm_hit.clear();
      return micro_resize(c, &c.mnl_warm_store, &c.mnl_warm_store_bytes, 0);
    }
    return 0;
  }
  if (!std::strcmp(name, "pc_mg_dist")) {  // 1: pc_type 1 on a context with a communicator (the distributed hierarchy)
    if (value != 0. && value != 1.) {
      set_error("pc_mg_dist: 0 (pc_type mg on one rank only) or 1 (the hierarchy distributed over the ranks)");
      return 1;
    }
    const bool multi = c.nranks > 1 || c.comm || c.lg;
    if (value == 0. && c.pc_mg_dist && c.pc_type == 1 && multi) {
      set_error("pc_mg_dist 0: pc_type is 1 on rank " + std::to_string(c.rank) + " of " + std::to_string(c.nranks) +
                " (set pc_type 0 first)");
      return 2;
    }
    c.pc_mg_dist = (int)value;  // without a communicator it changes nothing
    return 0;
  }
  if (!std::strcmp(name, "pc_mg_precision")) {  // the storage of the hierarchy's levels >= 1
    if (value != 0. && value != 1.) {
      set_error("pc_mg_precision: 0 (double: the whole hierarchy in double) or 1 (single: the levels >= 1 stored in float)");
      return 1;
    }
    if ((int)value != c.pc_mg_precision) pcmg_free(c);  // the next use builds the hierarchy in the other type
    c.pc_mg_precision = (int)value;
    return 0;
  }
  if (!std::strcmp(name, "pc_type")) {  // the macro CG's preconditioner: 0 Jacobi, 1 geometric multigrid
    if (value != 0. && value != 1.) {
      set_error("pc_type: 0 (jacobi) or 1 (mg)");
      return 2;
    }
    if (value == 1.) {
      if (int rc = pcmg_check(c, c.pc_mg_levels)) return rc;
    } else {
      pcmg_free(c);
    }
    c.pc_type = (int)value;
    return 0;
  }
  if (!std::strcmp(name, "pc_mg_levels")) {  // 0: automatic (coarsen until every axis has <= 5 nodes)
    if (value != (double)(int)value || (value != 0. && (value < 2. || value > (double)PCMG_MAXLEV))) {
      set_error("pc_mg_levels: 0 (automatic) or 2 .. " + std::to_string(PCMG_MAXLEV));
      return 2;
    }
    // the level sizes are known now: refuse a coarsest level that is too large (pc_mg_dist: or a level
    // that leaves a rank without a node; every rank decides alike, from the options alone)
    if ((c.nranks == 1 && !c.comm && !c.lg) || c.pc_mg_dist)
      if (int rc = pcmg_check(c, (int)value)) return rc;
    if ((int)value != c.pc_mg_levels) pcmg_free(c);
    c.pc_mg_levels = (int)value;
    return 0;
  }
  if (!std::strcmp(name, "pc_mg_smooth")) {  // Chebyshev degree of the pre- and the post-smoother
    if (value != (double)(int)value || value < 1. || value > 8.) {
      set_error("pc_mg_smooth: 1 .. 8");
      return 2;
    }
    c.pc_mg_smooth = (int)value;
    return 0;
  }
  if (!std::strcmp(name, "micro_grid_poll")) {  // tuning / testing: CG iterations enqueued between two host polls
    if (!(value >= 1.) || value > 4096. || value != (double)(int)value) {
      set_error("micro_grid_poll: an integer 1 .. 4096");
      return 1;
    }
    c.micro_grid_poll = (int)value;
    return 0;
  }
  if (!std::strcmp(name, "spmv_subl")) {
    const int old = c.spmv_subl;
    c.spmv_subl = (int)value;
    if (!partials_fit(c)) {
      c.spmv_subl = old;
      set_error("spmv_subl: partials buffer too small");
      return 2;
    }
    return 0;
  }
  if (!std::strcmp(name, "spmv_zblocks")) {
    const int old = c.spmv_zblocks;
    c.spmv_zblocks = (int)value;
    if (!partials_fit(c)) {
      c.spmv_zblocks = old;
      set_error("spmv_zblocks: partials buffer too small");
      return 2;
    }
    return 0;
  }
  if (!std::strcmp(name, "split_wide")) {  // testing: f32 corrections even when bf16 is exact
    c.split_wide = value != 0.;
    return 0;
  }
  if (!std::strcmp(name, "split_maxq")) {  // takes effect at the next mcx_assembly_jac
    c.split_declined = false;
    c.split_maxq = std::max(0, std::min(30, (int)value));
    return 0;
  }
  if (!std::strcmp(name, "split_dense")) {  // takes effect at the next mcx_assembly_jac
    c.split_declined = false;
    c.split_dense = value != 0.;
    return 0;
  }
  if (!std::strcmp(name, "split_dbg")) {
    c.split_dbg = std::max(0, std::min(2047, (int)value));  // (k_spmv_sp DBG: bits, see the kernel)
    return 0;
  }
  if (!std::strcmp(name, "face_dbg")) {  // timing-only (wrong products): bits 1 listed rows, 2 x faces, 4 y/z faces dropped
    c.face_dbg = std::max(0, std::min(7, (int)value));
    return 0;
  }
  if (!std::strcmp(name, "split_tx")) {
    const int v = (int)value;
    if (v != 0 && v != 64 && v != 128 && v != 256) {
      set_error("split_tx: 0, 64, 128 or 256");
      return 2;
    }
    const int old = c.split_tx;
    c.split_tx = v;
    if (!partials_fit(c)) {
      c.split_tx = old;
      set_error("split_tx: partials buffer too small");
      return 2;
    }
    return 0;
  }
  if (!std::strcmp(name, "cg_fuse")) {
    c.fuse = value != 0.;
    return 0;
  }
  if (!std::strcmp(name, "comm_timeout")) {  // seconds a host wait on collective work may take
    if (!(value > 0.)) {
      set_error("comm_timeout: seconds > 0");
      return 1;
    }
    c.comm_timeout = value;
    return 0;
  }
  if (!std::strcmp(name, "halo_overlap")) {
    c.overlap = value != 0.;
    return 0;
  }
  if (!std::strcmp(name, "split_ty")) {
    const int v = (int)value;
    if (v != 0 && v != 2 && v != 4 && v != 8 && v != 16) {
      set_error("split_ty: 0, 2, 4, 8 or 16");
      return 2;
    }
    const int old = c.split_ty;
    c.split_ty = v;
    if (!partials_fit(c)) {
      c.split_ty = old;
      set_error("split_ty: partials buffer too small");
      return 2;
    }
    return 0;
  }
  if (!std::strcmp(name, "vi_bits")) {  // takes effect at the next mcx_assembly_jac
    const int v = (int)value;
    if (v != 4 && v != 8) {
      set_error("vi_bits: 4 (per-slot nibbles where every slot has <= 16 values) or 8");
      return 2;
    }
    c.vi_bits_max = v;
    return 0;
  }
  if (!std::strcmp(name, "vi_block")) {  // takes effect at the next mcx_assembly_jac
    c.vi_block_on = value != 0.;
    return 0;
  }
  if (!std::strcmp(name, "cg_pdb")) {  // 0 | 1 (two p buffers) | 4 (four, the default)
    if (!(value == 0. || value == 1. || value == 4.)) {
      set_error("cg_pdb: 0, 1 (two p buffers) or 4 (four)");
      return 1;
    }
    c.cg_pdb = (int)value;
    return 0;
  }
  if (!std::strcmp(name, "cg_rev")) {
    c.cg_rev = value != 0.;
    return 0;
  }
  if (!std::strcmp(name, "cg_par")) {  // 0 | 1 (the host's parity hint) | 2 (a skewed hint: testing)
    if (!(value == 0. || value == 1. || value == 2.)) {
      set_error("cg_par: 0, 1 or 2 (testing: a wrong hint)");
      return 1;
    }
    c.cg_par = (int)value;
    return 0;
  }
  if (!std::strcmp(name, "vi_exc_list")) {
    if (value < 0. || value > VI_EXC_LIST) {
      set_error("vi_exc_list: 0 .. 2048");
      return 1;
    }
    c.vi_exc_list = (int)value;
    return 0;
  }
  if (!std::strcmp(name, "split_esc")) {  // takes effect at the next mcx_assembly_jac
    c.split_esc = value != 0.;
    c.split_declined = false;
    return 0;
  }
  if (!std::strcmp(name, "vi_lg")) {
    if (!(value == 1. || value == 2. || value == 3.)) {
      set_error("vi_lg: 1, 2 or 3");
      return 1;
    }
    c.vi_lg = (int)value;
    return 0;
  }
  if (!std::strcmp(name, "cg_p2d")) {
    c.cg_p2d = value != 0.;
    return 0;
  }
  if (!std::strcmp(name, "vi_st_faces")) {  // rebuilds the default-stencil structures if built
    const int old = c.vi_st_faces;
    c.vi_st_faces = (int)value & 0x7f;  // 1: all 6 faces; else bit c = face class c (1..6)
    if ((c.st_ok || c.st_pending) && build_st(c)) return 1;
    if (!partials_fit(c)) {
      c.vi_st_faces = old;
      set_error("vi_st_faces: partials buffer too small");
      return (c.st_ok || c.st_pending) && build_st(c) ? 1 : 2;
    }
    return 0;
  }
  if (!std::strcmp(name, "vi_st_pair")) {
    const int old = c.vi_st_pair;
    c.vi_st_pair = value != 0.;
    if (!partials_fit(c)) {
      c.vi_st_pair = old;
      set_error("vi_st_pair: partials buffer too small");
      return 2;
    }
    return 0;
  }
  if (!std::strcmp(name, "vi_st_fstream")) {
    c.vi_st_fstream = value != 0.;
    return 0;
  }
  if (!std::strcmp(name, "vi_st_l16")) {
    if (!(value == -1. || value == 0. || value == 1.)) {
      set_error("vi_st_l16: -1 (by the list's length), 0 or 1");
      return 1;
    }
    const int old = c.vi_st_l16;
    c.vi_st_l16 = (int)value;
    if (!partials_fit(c)) {
      c.vi_st_l16 = old;
      set_error("vi_st_l16: partials buffer too small");
      return 2;
    }
    return 0;
  }
  if (!std::strcmp(name, "vi_st_dma")) {  // same grid and partials as k_spmv_st: nothing to re-check
    if (!(value == -1. || value == 0. || value == 1.)) {
      set_error("vi_st_dma: -1 (where eligible), 0 or 1");
      return 1;
    }
    c.vi_st_dma = (int)value;
    return 0;
  }
  if (!std::strcmp(name, "vi_st_pf")) {
    if (!(value == 1. || value == 2. || value == 3.)) {  // 3: timing-only, the ring never refilled (wrong rows)
      set_error("vi_st_pf: 1 or 2");
      return 1;
    }
    c.vi_st_pf = (int)value;
    return 0;
  }
  if (!std::strcmp(name, "vi_st_ty")) {
    if (!(value == 8. || value == 16.)) {
      set_error("vi_st_ty: 8 or 16");
      return 1;
    }
    const int old = c.vi_st_ty;
    c.vi_st_ty = (int)value;
    if (!partials_fit(c)) {
      c.vi_st_ty = old;
      set_error("vi_st_ty: partials buffer too small");
      return 2;
    }
    return 0;
  }
  if (!std::strcmp(name, "vi_st_tail")) {
    const int old = c.vi_st_tail;
    c.vi_st_tail = value != 0.;
    if (!partials_fit(c)) {
      c.vi_st_tail = old;
      set_error("vi_st_tail: partials buffer too small");
      return 2;
    }
    return 0;
  }
  if (!std::strcmp(name, "vi_st")) {  // takes effect at once if the structures were built (they are by default)
    if (!(value == -1. || value == 0. || value == 1.)) {
      set_error("vi_st: -1 (by size), 0 or 1");
      return 1;
    }
    const int old = c.vi_st;
    c.vi_st = (int)value;
    if (c.st_pending && st_wanted(c) && build_st(c)) return 1;  // built lazily: the path turned on
    if (!partials_fit(c)) {
      c.vi_st = old;
      set_error("vi_st: partials buffer too small");
      return 2;
    }
    return 0;
  }
  if (!std::strcmp(name, "vi_exc_kernel")) {
    const bool old = c.vi_exc_kernel;
    c.vi_exc_kernel = value != 0.;
    if (!partials_fit(c)) {
      c.vi_exc_kernel = old;
      set_error("vi_exc_kernel: partials buffer too small");
      return 2;
    }
    return 0;
  }
  if (!std::strcmp(name, "vi_lg_exc")) {
    c.vi_lg_exc = value != 0.;
    return 0;
  }
  if (!std::strcmp(name, "cg_xs")) {  // takes effect at the next solve (with cg_pdb 4)
    c.cg_xs = value != 0.;
    return 0;
  }
  if (!std::strcmp(name, "cg_ublocks")) {
    if (value < 0 || value > (1 << 30) || value != (double)(int)value) {
      set_error("cg_ublocks: 0 (uncapped) or a block count");
      return 1;
    }
    c.cg_ublocks = (int)value;
    return 0;
  }
  if (!std::strcmp(name, "vi_wdesc")) {
    if (!(value == 0. || value == 1. || value == 2.)) {
      set_error("vi_wdesc: 0, 1 or 2");
      return 1;
    }
    c.vi_wdesc = (int)value;
    return 0;
  }
  if (!std::strcmp(name, "vi_ypair")) {
    c.vi_ypair = value != 0.;
    return 0;
  }
  if (!std::strcmp(name, "vi_wmap")) {
    c.vi_wmap = value != 0.;
    return 0;
  }
  if (!std::strcmp(name, "vi_ring3")) {
    c.vi_ring3 = value != 0.;
    return 0;
  }
  if (!std::strcmp(name, "vi_tx")) {  // validated before it is stored: a refused width leaves the tiling as it was
    const int v = (int)value;
    if (!(v == 0 || v == 64 || v == 128 || v == 256) || (double)v != value) {
      set_error("vi_tx: 0 (default), 64, 128 or 256");
      return 1;
    }
    const int old = c.vi_tx;
    c.vi_tx = v;
    if (!partials_fit(c)) {
      c.vi_tx = old;
      set_error("vi_tx: partials buffer too small");
      return 7;
    }
    return 0;
  }
  if (!std::strcmp(name, "cg_fusep")) {
    c.cg_fusep = value != 0.;
    return 0;
  }
  if (!std::strcmp(name, "vi_exc_max")) {  // takes effect at the next mcx_assembly_jac
    c.vi_exc_max = std::max(0, std::min(1000, (int)value));
    c.vi_declined = false;
    return 0;
  }
  if (!std::strcmp(name, "vib_onepass")) {  // takes effect at the next mcx_assembly_jac
    c.vib_onepass = value != 0.;
    return 0;
  }
  if (!std::strcmp(name, "vi_fma")) {
    c.vi_fma = value != 0.;
    return 0;
  }
  if (!std::strcmp(name, "vi_patch")) {
    c.vi_patch = value != 0.;
    return 0;
  }
  if (!std::strcmp(name, "vi_uni")) {
    c.vi_uni = value != 0.;
    return 0;
  }
  if (!std::strcmp(name, "vi_xread")) {
    c.vi_xread = value != 0.;
    return 0;
  }
  if (!std::strcmp(name, "vi_stage")) {
    const int old = c.vi_stage;
    c.vi_stage = value < 0. ? -1 : (value != 0. ? 1 : 0);
    if (!partials_fit(c)) {
      c.vi_stage = old;
      set_error("vi_stage: partials buffer too small");
      return 2;
    }
    return 0;
  }
  if (!std::strcmp(name, "aij_vi")) {  // takes effect at the next mcx_assembly_jac
    if (c.o.mat_type != MCX_MAT_AIJ) {
      set_error("aij_vi: -dm_mat_type aij only");
      return 2;
    }
    c.vi_declined = false;
    c.aij_vi = value != 0.;
    return 0;
  }
  if (!std::strcmp(name, "aij_split")) {  // takes effect at the next mcx_assembly_jac
    c.split_declined = false;
    if (value != 0. && !c.d_mask) {
      set_error("aij_split: context created with -mat_aij_split 0 (no split storage)");
      return 2;
    }
    c.aij_split = value != 0.;
    return 0;
  }
  if (!std::strcmp(name, "cg_dix")) {
    c.cg_dix = value != 0.;
    return 0;
  }
  if (!std::strcmp(name, "cg_nt")) {
    c.cg_nt = (int)value;
    return 0;
  }
  if (!std::strcmp(name, "spmv_nt")) {
    c.spmv_nt = (int)value;
    return 0;
  }
  if (!std::strcmp(name, "spmv_kernel")) {
    const int old = c.spmv_kernel;
    c.spmv_kernel = (int)value;
    if (!partials_fit(c)) {
      c.spmv_kernel = old;
      set_error("spmv_kernel: partials buffer too small");
      return 2;
    }
    return 0;
  }
  set_error(std::string("unknown option ") + name);
  return 2;
} MCX_CATCH

// the command-line flags without an mcx_opts field (kApplyFlags): each goes through mcx_set_option
int mcx_apply_args(void* ctx, int argc, const char* const* argv) try {
  MCX_ENTRY();
  if (!ctx) {
    set_error("mcx_apply_args: null context");
    return 1;
  }
  for (int a = 0; a + 1 < argc; a++) {
    const char* k = argv[a];
    if (!k || !argv[a + 1] || !apply_flag(k)) continue;
    const char* v = argv[++a];
    double value;
    if (!std::strcmp(k, "-micro_mem")) {
      if (std::strcmp(v, "lds") && std::strcmp(v, "device")) {
        set_error(std::string("-micro_mem: lds or device, got ") + v);
        return 2;
      }
      value = std::strcmp(v, "device") ? 0. : 1.;
    } else if (!std::strcmp(k, "-micro_solver")) {
      if (std::strcmp(v, "cell") && std::strcmp(v, "grid")) {
        set_error(std::string("-micro_solver: cell or grid, got ") + v);
        return 2;
      }
      value = std::strcmp(v, "grid") ? 0. : 1.;
    } else if (!std::strcmp(k, "-micro_nl_solver")) {
      if (std::strcmp(v, "cell") && std::strcmp(v, "grid")) {
        set_error(std::string("-micro_nl_solver: cell or grid, got ") + v);
        return 2;
      }
      value = std::strcmp(v, "grid") ? 0. : 1.;
    } else if (!std::strcmp(k, "-micro_nl_start")) {
      if (std::strcmp(v, "zero") && std::strcmp(v, "elastic")) {
        set_error(std::string("-micro_nl_start: zero or elastic, got ") + v);
        return 2;
      }
      value = std::strcmp(v, "elastic") ? 0. : 1.;
    } else if (!std::strcmp(k, "-micro_nl_ls")) {
      if (!micro_nl_ls_word(v)) {
        set_error(std::string("-micro_nl_ls: an integer 0 .. 16, got ") + v);
        return 2;
      }
      value = std::atof(v);
    } else if (!std::strcmp(k, "-micro_nl_tangent")) {
      if (std::strcmp(v, "seq") && std::strcmp(v, "block")) {
        set_error(std::string("-micro_nl_tangent: seq or block, got ") + v);
        return 2;
      }
      value = std::strcmp(v, "block") ? 0. : 1.;
    } else if (!std::strcmp(k, "-micro_nl_apply")) {
      if (std::strcmp(v, "split") && std::strcmp(v, "fused")) {
        set_error(std::string("-micro_nl_apply: split or fused, got ") + v);
        return 2;
      }
      value = std::strcmp(v, "fused") ? 0. : 1.;
    } else if (!std::strcmp(k, "-micro_nl_warm")) {
      if (std::strcmp(v, "off") && std::strcmp(v, "on")) {
        set_error(std::string("-micro_nl_warm: off or on, got ") + v);
        return 2;
      }
      value = std::strcmp(v, "on") ? 0. : 1.;
    } else if (!std::strcmp(k, "-pc_mg_precision")) {
      if (std::strcmp(v, "double") && std::strcmp(v, "single")) {
        set_error(std::string("-pc_mg_precision: double or single, got ") + v);
        return 2;
      }
      value = std::strcmp(v, "single") ? 0. : 1.;
    } else if (!std::strcmp(k, "-pc_type")) {
      if (std::strcmp(v, "jacobi") && std::strcmp(v, "mg")) {
        set_error(std::string("only -ksp_type cg / -pc_type jacobi / mg are implemented, got ") + v);
        return 2;
      }
      value = std::strcmp(v, "mg") ? 0. : 1.;
    } else {
      value = std::atof(v);
    }
    if (int rc = mcx_set_option(ctx, !std::strcmp(k, "-mg_levels_ksp_max_it") ? "pc_mg_smooth" : k + 1, value)) return rc;
  }
  return 0;
} MCX_CATCH

int mcx_time_spmv(void* ctx, int iters, double* avg_ms) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  if (!c.assembled) {
    set_error("mcx_time_spmv: no matrix assembled");
    return 5;
  }
  launch_spmv(c, c.p_pad, c.w, true, false);  // warm
  MCX_HIP(hipEventRecord(c.ev_a, c.stream));
  for (int q = 0; q < iters; q++) launch_spmv(c, c.p_pad, c.w, true, false);
  MCX_HIP(hipEventRecord(c.ev_b, c.stream));
  MCX_HIP(hipEventSynchronize(c.ev_b));
  float ms = 0.f;
  MCX_HIP(hipEventElapsedTime(&ms, c.ev_a, c.ev_b));
  *avg_ms = ms / std::max(iters, 1);
  return 0;
} MCX_CATCH

int mcx_synchronize(void* ctx) try {
  MCX_ENTRY();
  GUARD(ctx);
  CTX(ctx);
  MCX_HIP(hipEventRecord(c.ev_chunk[0], c.stream));  // the stream may hold collectives: bounded wait
  return comm_wait(c, c.ev_chunk[0], "mcx_synchronize");
} MCX_CATCH

}  // extern "C"
