// mcx_internal.h — context, geometry and kernel-launcher declarations of the MI355X
// MacroC hot path.  See DESIGN.md for the HBM layout; include/macroc_amd.h for the ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/macroc_amd.h"
#include "pcmg_plan.h"

namespace mcx {

constexpr int NGP = 8, NPE = 8, NVOI = 6;
constexpr int NSLOT = 243;   // 27 neighbour blocks x 3x3
constexpr int NPAIR = 122;   // slots stored as double2 pairs (slot 243 = zero pad)
constexpr int GROUP = 64;    // nodes per AoSoA group (= one wavefront)
constexpr int USLOT = 123;   // sbaij: 6 upper-triangle diagonal values + 13 upper blocks x 9
constexpr int UPAIR = 62;

void set_error(const std::string& s);

// Geometry of one rank's subdomain, passed by value to every kernel.
struct Geo {
  int NX, NY, NZ;          // global node counts
  int xs, ys, zs;          // first owned node (global)
  int nx, ny, nz;          // owned node counts
  int PX, PY, PZ;          // padded box = owned + 1 ghost layer each side
  int UX, UXY;             // sbaij storage pitch: rows of UX = roundup(nx+2, 64) nodes (u_of)
  int ncu;                 // compute units (z-marching grid sizing)
  int nown;                // nx*ny*nz
  int ex0, ey0, ez0;       // first element evaluated on this device (global)
  int nex, ney, nez;       // extended element counts (owned + upper ghost layer)
  int64_t nelem;           // nex*ney*nez
  int64_t xld;             // value-indexed exception blocks: slot capacity of exc (a multiple of 64, exc_base)
  int bc_type;
  double lx, lz, dx, dz, rad, wg;
};

// device-side state of the CG loop (PETSc KSPSolve_CG scalars)
struct CgState {
  double beta, betaold, dpi, dpiold, alpha, dp, ttol, rnorm0, bcoef;
  double rtol, abstol, dtol;
  int i, its, reason, maxits, hist_on;
  int xpend;  // x += alpha p of the last iteration not yet applied (k_cg_pupdate / k_cg_xfinal apply it)
  int xp;     // the last iteration whose alpha step succeeded (-1: none); the fused path's pending x update
  double alpha_prev;  // alpha of the iteration before (the fused path's every-second-iteration x update)
  double ah[8];       // alpha of iteration j at ah[j & 7] (quad-buffered p: x every fourth iteration)
};

struct Material {
  int law;                 // MCX_LAW_ELASTIC | MCX_LAW_PLASTIC | MCX_LAW_EXTERNAL | MCX_LAW_MICRO
  double E, nu, Sy, Ka;
  double C[36];            // isotropic elastic tangent (Voigt, engineering shear); -mat_law micro: C_hom
};

// -mat_law micro: the two-phase unit cell homogenised on the device (k_micro_rve)
constexpr int MICRO_NMAX = 10;      // nodes per edge (micro_n) with the cell solvers' vectors in LDS (micro_mem 0)
constexpr int MICRO_NMAX_DEV = 20;  // ... with the vectors in device memory (micro_mem 1): one workgroup
                                    // per cell still, and the phase bytes (19^3) stay in LDS
constexpr int MICRO_NMAX_GRID = 128;  // ... with the grid-wide solver (option micro_solver 1): one
                                      // workgroup per 8x8x8-node tile of a load case, -mat_law micro only
constexpr int MICRO_NMAX_NL_GRID = 64;  // ... of -mat_law micro_nl with its grid-wide solver (option micro_nl_solver 1,
                                        // DESIGN §18): a history slot is 224 B x 8 (n-1)^3, 448 MB at n = 64
constexpr int MICRO_DOFS = 3 * MICRO_NMAX * MICRO_NMAX * MICRO_NMAX;  // LDS vectors are sized for it
constexpr int MICRO_TPB = 512;
constexpr int MICRO_OUT = 16;  // doubles a load case leaves: 6 average stresses, iterations, relative norm, converged
struct MicroArgs {
  int n, type;          // -micro_n, -micro_type
  double E[2], nu[2];   // phase 0 = micro_mat_1, phase 1 = micro_mat_2
  double rtol;          // stopping rule: |D^-1 r| <= rtol |D^-1 r_0|
  int max_it;
};
// phase of micro element (i, j, k), indices 0 .. ne-1, in exact integer arithmetic: type 0 a
// centred sphere of radius 0.5, type 1 a flat layer in y
__host__ __device__ inline int micro_phase(int type, int ne, int i, int j, int k) {
  if (type == 0) {
    const int a = 2 * i + 1 - ne, b = 2 * j + 1 - ne, c = 2 * k + 1 - ne;
    return a * a + b * b + c * c < ne * ne;
  }
  return 2 * j + 1 < ne;
}

// option micro_solver 1: the six unit-strain solves spread over the device, one
// workgroup per tile of MG_T^3 nodes of a load case and one kernel launch per CG phase.  One
// allocation holds, in this order: the six load cases' five vectors ([6][5][3 n^3]: x, r, p, q,
// D^-1), the two element matrices, the partial sums ([6][MG_NPART][npart]) and the six state records.
constexpr int MG_T = 8;       // nodes per tile edge: MG_T^3 = MICRO_TPB threads, one per node
constexpr int MG_H = MG_T + 2;  // ... of the tile's halo of p in LDS
constexpr int MG_NPART = 6;   // partial sums a workgroup leaves at most (the stress average's six)
struct MicroGridState {       // one per load case, written by the scalar kernels only
  double rz, pq, alpha, beta, norm0, rel;
  int its, conv, done, pad;
};
struct MicroGridWs {
  double* vec;           // [6][5][ndof]
  double* ske;           // [2][24][24]
  double* part;          // [6][MG_NPART][npart]
  MicroGridState* st;    // [6]
  int ntile, npart;      // tiles per axis; max(tiles, vector blocks) = the partial arrays' length
};
inline int mg_ntile(int n) { return (n + MG_T - 1) / MG_T; }
inline int64_t mg_npart(int n) {
  const int64_t t = mg_ntile(n), nt = t * t * t, nvb = (3 * (int64_t)n * n * n + MICRO_TPB - 1) / MICRO_TPB;
  return nt > nvb ? nt : nvb;
}
inline int64_t mg_ws_bytes(int n) {
  const int64_t ndof = 3 * (int64_t)n * n * n;
  return (int64_t)sizeof(double) * (6 * 5 * ndof + 2 * 576 + 6 * MG_NPART * mg_npart(n)) + 6 * (int64_t)sizeof(MicroGridState);
}

// -mat_law micro_nl: the same cell with J2-plastic phases, solved per macro Gauss point.
// A solved point owns a slot of the pool: MNL_WS doubles per micro Gauss point, component-major
// ([comp][8 (n-1)^3]): committed history 7, new history 7, tangent data 8 (theta, theta-bar, n[6]),
// work stresses 6
constexpr int MNL_H0 = 0, MNL_H1 = 7, MNL_TAN = 14, MNL_SIG = 22, MNL_WS = 28;
constexpr int MNL_CONC = 38;  // per micro Gauss point: strain concentration 6x6, 2G, sqrt(2/3) Sy
struct MicroNlArgs {
  MicroArgs m;          // the cell, phase E / nu, the CG's rtol and max_it
  double Sy[2], Ka[2];
  double nl_rtol;       // Newton: |D^-1 R| <= nl_rtol |D^-1 R_0|
  int nl_max_it;
  int nl_start, nl_ls;  // options micro_nl_start, micro_nl_ls: elastic predictor, step lengths 2^-j, j <= nl_ls
};

// option micro_nl_solver 1: the listed points' Newton / CG solves spread over the device,
// one workgroup per tile of MG_T^3 nodes (or elements) of one solve and one kernel launch per phase;
// up to `batch` solves share a launch (blockIdx.y).  One allocation holds, in this order: the solves'
// six vectors ([batch][6][3 n^3]: u, x, r, p, q, D^-1), the partial sums ([batch][MNLG_NPART][npart])
// and the state records.  A record's stage gates every kernel: the scalar kernels alone write it.
constexpr int MNLG_NVEC = 6;
constexpr int MNLG_NPART = 9;  // 0, 1: the dot products; 2 .. 7: the stress sums; 8: the largest trial f
enum { MNLG_CG = 0, MNLG_TRANS = 1, MNLG_TSTART = 2, MNLG_DONE = 3 };
// what k_mnlg_prep does to u before a Newton solve's next state pass
enum { MNLG_PEND_NONE = 0, MNLG_PEND_PRED = 1, MNLG_PEND_BACK = 2 };
// option micro_nl_warm 1: a slot's warm record, the last converged interior field and
// tangent columns ([slot][7][3 n^3]: u_w, W_0 .. W_5) and its header ([slot]); two more stages,
// the second start pass of a tangent column (MNLG_TSTART2) or of a block (MNLG_BSTART2)
enum { MNLG_TSTART2 = 7, MNLG_BSTART2 = 8 };
struct MnlWarmHdr {
  double eps[6];  // the macro strain the record belongs to
  int valid;      // set by a solve that ended converged, cleared when the slot's next solve starts
  int pad[3];
};
static_assert(sizeof(MnlWarmHdr) == 64, "the documented record: 7 x 24 n^3 + 64 bytes");
inline int64_t mnl_warm_bytes(int n) {  // per slot
  return (int64_t)sizeof(double) * 7 * 3 * n * n * n + (int64_t)sizeof(MnlWarmHdr);
}
struct MnlGridState {
  double rz, pq, alpha, beta, norm0;  // the running CG
  double nnorm0, nrel;                // Newton: the first norm, the last relative one
  double col[36];                     // the tangent's columns as they arrive
  int64_t q;                          // the macro Gauss point
  int slot;
  int stage;   // MNLG_CG: a CG runs; MNLG_TRANS: the next transition starts a Newton step or ends a column;
               // MNLG_TSTART: (inside a transition) the tangent solve of column lc starts; MNLG_DONE
  int lc;      // -1: Newton; 0 .. 5: the tangent's column
  int fresh;   // no state pass yet: u takes its boundary values, D is built
  int nits, cgits, its, status;  // Newton steps, CG iterations (all, the running CG), 0 ok / 1 Newton / 2 CG
  // options micro_nl_start / micro_nl_ls
  int pend;                      // MNLG_PEND_*: the predictor or a shorter trial is owed to u
  int trial, rejects;            // the trial under test (-1: none; its length is 2^-trial), rejected trials
  int warm;                      // option micro_nl_warm: the slot's record was valid when the solve began
  double nacc, lam, minstep;     // the norm at the last accepted iterate, 2^-trial, the smallest accepted length
};
static_assert(sizeof(MnlGridState) == 8 * 53, "warm sits in the padding: the workspace's size is micro_nl_warm 0's");
struct MnlGridWs {
  double* vec;
  double* part;
  MnlGridState* st;
  int ntile, npart;
  double* warm;      // option micro_nl_warm 1: the warm store's fields, else null
  MnlWarmHdr* whdr;  // and its headers
};
inline int64_t mnlg_ws_bytes(int n, int64_t batch) {
  const int64_t ndof = 3 * (int64_t)n * n * n;
  return batch * ((int64_t)sizeof(double) * (MNLG_NVEC * ndof + MNLG_NPART * mg_npart(n)) + (int64_t)sizeof(MnlGridState));
}

// option micro_nl_tangent 1: the six tangent columns of a solve advance together, each
// with its own CG record.  Column 0 keeps the solve's x, r, p, q and the slot's work stresses; the
// columns 1 .. 5 have theirs behind the layout above, in this order: the vectors
// ([batch][5][4][3 n^3]: x, r, p, q), the work stresses ([batch][5][6][8 (n-1)^3]), the partial sums
// ([batch][6][MNLB_NPART][npart]) and the column records ([batch][6]).  Three more stages, which the
// k_mnlg_* kernels of the sequential columns do not know and so pass by.
constexpr int MNLB_NPART = 8;  // per column: 0, 1 the dot products; 2 .. 7 the stress sums
enum { MNLG_BSTART = 4, MNLG_BCG = 5, MNLG_BTRANS = 6 };
struct MnlBlockCol {
  double rz, pq, alpha, beta, norm0;  // the column's CG
  int its, done, status, pad;         // its iterations; ended; 0 converged / 2 not
};
struct MnlBlockWs {
  double* vec;
  double* sig;
  double* part;
  MnlBlockCol* col;
};
inline int64_t mnlb_vec_bytes(int n) { return (int64_t)sizeof(double) * 5 * 4 * 3 * n * n * n; }
inline int64_t mnlb_sig_bytes(int n) { return (int64_t)sizeof(double) * 5 * 6 * 8 * (n - 1) * (n - 1) * (n - 1); }
inline int64_t mnlb_ws_bytes(int n, int64_t batch) {  // what the block adds to mnlg_ws_bytes
  return batch * (mnlb_vec_bytes(n) + mnlb_sig_bytes(n) + (int64_t)sizeof(double) * 6 * MNLB_NPART * mg_npart(n) +
                  6 * (int64_t)sizeof(MnlBlockCol));
}

// -pc_type mg: geometric multigrid preconditioner of the macro CG, one rank.  Level 0
// is the assembled matrix (launch_spmv, whatever its storage); a coarser level keeps its Galerkin
// operator as plain stencil blocks, slot-major: value (nb, r, c) of node n at A[(nb*9 + r*3 + c) * nn + n].
// (PCMG_MAXLEV, PCMG_COARSE_MAX and the planner: pcmg_plan.h)
// where node (i, j, k) of a rank's box lives in a vector: (i + off) + (j + off) PX + (k + off) PXY.
// Owned and one-rank coarse vectors: PX = nx, PXY = nx ny, off = 0; a padded box (the fine level's SpMV
// input; with pc_mg_dist every vector read through a stencil, P or P^T): off = 1.  gs / gn: the box's
// global start and the level's global node counts (one rank: 0 and nx, ny, nz) — what decides by the
// global index (coarse or not, the last-node rule, probe colours, the seed, the domain's edge) uses them.
struct PcmgLay {
  int nx, ny, nz, PX, PXY, off;
  int gs[3], gn[3];
};
struct PcmgXfer {  // a level and the next coarser one: owned counts, global starts, global counts
  int fn[3], cn[3];
  int fs[3], cs[3], FN[3], CN[3];
};
struct HaloPlan {
  std::vector<int> nbr_rank;          // neighbour ranks (<= 26)
  std::vector<int64_t> send_off, send_cnt, recv_off, recv_cnt;  // in nodes
  int* d_send_idx = nullptr;          // padded node index of each sent node
  int* d_recv_idx = nullptr;          // padded node index of each received node
  void* d_sendbuf = nullptr;         // 3 values per node, esz bytes each
  void* d_recvbuf = nullptr;
  int esz = 8;                        // 8: double; 4: a float level of the multigrid (pc_mg_precision 1)
  int64_t nsend = 0, nrecv = 0;
  int* d_bnd = nullptr;               // owned node index of every sent node, each once
  int64_t nbnd = 0;
  int level = -1;                     // -1: the context's plan (Ctx::halo); l >= 1: multigrid level l's box (pc_mg_dist)
};

// A vector or an operator of a multigrid level together with its storage type: double, or float on a
// level >= 1 under pc_mg_precision 1.  The type travels with the pointer from where it was
// allocated, and the launchers ask for the typed pointer: using one as the other type is an error
// (std::logic_error, which every C entry turns into MCX_EXC), never a silent reinterpretation.
struct PcmgVec {
  void* p = nullptr;
  bool f32 = false;
  PcmgVec() = default;
  PcmgVec(std::nullptr_t) {}
  PcmgVec(double* q) : p(q), f32(false) {}
  PcmgVec(const double* q) : p(const_cast<double*>(q)), f32(false) {}
  PcmgVec(float* q) : p(q), f32(true) {}
  explicit operator bool() const { return p != nullptr; }
  template <class T>
  T* as() const {  // a null vector has any type
    if (p && f32 != std::is_same<T, float>::value)
      throw std::logic_error("multigrid: a level's vector used as the other storage type");
    return static_cast<T*>(p);
  }
};

struct PcmgLevel {
  int n[3] = {0, 0, 0};        // owned nodes of this rank's box
  int64_t nn = 0;              // ... their product
  int s[3] = {0, 0, 0};        // the box's global start
  int N[3] = {0, 0, 0};        // the level's global node counts (one rank: n)
  // pc_mg_precision 1: on a level >= 1 the operator and every vector below are float
  // (f32; each PcmgVec carries it too), loaded and widened, computed in double and narrowed on the
  // store; level 0 is double always
  bool f32 = false;
  PcmgVec rp;                  // pc_mg_dist: the residual masked by its owner, padded box (what P^T reads after a halo)
  void* rp_base = nullptr;     // ... its allocation on level 0 (aligned as x)
  HaloPlan halo;               // pc_mg_dist, level >= 1: the box's ghost fill (level 0 uses Ctx::halo)
  PcmgVec A;                   // [243][nn] (levels >= 1)
  PcmgVec x;                   // the cycle's iterate (level 0: padded box, shifted by pad_off from x_base)
  void* x_base = nullptr;
  PcmgVec b, r, d, dinv;       // level 0: b = the cycle's argument, r = c.w, d = c.z, dinv = c.dinv
  unsigned char* mask = nullptr;  // [nn] bit d: dof d is a Dirichlet dof (level >= 1: its Galerkin diagonal was 0)
  double lmax = 0.;            // estimate of the largest eigenvalue of D^-1 A
};
struct Pcmg {
  int nlev = 0;
  PcmgLevel L[PCMG_MAXLEV];
  double* ainv = nullptr;      // dense inverse of the coarsest operator [nc][nc]
  int nc = 0;                  // its dofs (global)
  // pc_mg_dist on a context with a communicator: every level's box per the plan, x and rp
  // padded, and the coarsest level gathered by one all-reduce: arin (each rank's owned entries, zeros
  // elsewhere) -> arout on every rank; xfull = Ainv arout, of which each rank keeps its box
  bool dist = false;
  double *arin = nullptr, *arout = nullptr, *xfull = nullptr;
  int64_t ar_cap = 0;          // doubles of arin / arout (the coarsest operator's 243 NN blocks)
  double** d_ar_ptrs = nullptr;  // in-process transport: every member's arin
  int64_t bytes = 0;           // device memory of the hierarchy (counted in Ctx::device_bytes)
  bool alloc = false;
  bool built = false;          // operators, eigenvalue estimates and the inverse belong to the current matrix
};

struct Ctx;

// value-indexed exception blocks, AoSoA: groups of 64 slots, each group value-major (243 runs of 64
// doubles, one per value (nb, r, c)), so a wave of 64 consecutive slots reads one 512-B run per value
// and a group's values are contiguous (124 KB); value v of slot s at exc[exc_base(s) + v * 64]
__host__ __device__ inline int64_t exc_base(int64_t s) { return (s >> 6) * (243 * 64) + (s & 63); }

// Matrix storage of a context.  FMT_V: AIJ stencil blocks (all 27 blocks per node, every row
// summed in the reference's MatMult order (inode column pairs)).  FMT_U: MATSBAIJ (upper blocks, lower mirrored).  FMT_SPLIT:
// the AIJ matrix held exactly as its upper blocks U plus, per owned node, the bf16 correction
// lower - mirror(upper) of the correction slots that are non-zero somewhere in the matrix
// (every AIJ value reconstructs bit for bit; rows summed in the z-marching order).
// FMT_VI: the AIJ matrix held exactly as small indices into dictionaries of its distinct values
// (value-indexed CSR, Kourtis et al. 2008): a nibble per value into the slot's own dictionary
// (every slot takes at most 16 values) or a byte per value into one dictionary (at most 256),
// all 27 blocks per node in FMT_V's slot order — every row summed in the reference's MatMult order (inode column pairs).
enum Fmt { FMT_V = 0, FMT_U = 1, FMT_SPLIT = 2, FMT_VI = 3 };
constexpr int VI_MAX = 256;     // dictionary entries (one index byte per value)
constexpr int VI_EXC_LIST = 2048;  // staged value-indexed SpMV: exception nodes a tile defers to its block-wide pass
constexpr int VI_HASH = 4096;   // open-addressing set of the distinct values (bit patterns)
constexpr int VI_CHUNKS = 16;   // 16-B index chunks per node: 243 slots + 13 zero pad bytes
// vi_st -1: the default-stencil SpMV from this many owned nodes (at 256^3 it saves 2 % of a CG
// iteration, at 128^3 the faces' share makes it 6 % slower: profiles/r05p_*)
constexpr int64_t ST_MIN_NODES = int64_t(1) << 23;
constexpr int ST_CLASSES = 7;   // default-stencil SpMV: the interior + the 6 domain faces (k_st_setup)
struct StFaces {  // the face phase of the default-stencil SpMV: class c's patches (64 x 4 nodes) are [u[c-1], u[c])
  int64_t u[7];
};
constexpr int VIB_STRIDE = 10;  // doubles per dictionary block (9 values + pad: 16-B aligned)
constexpr int VB_GSV = 64;      // single-pass block build: entries of each slot's global value set (6-bit positions)

// AIJ-split correction slots, passed by value: slot = nb*9 + r*3 + c of the row node's lower
// block nb < 13 holds A(n, nb)[r][c] - U(m, 26-nb)[c][r], m = n + off(nb); nb = 13 (the
// diagonal block, stored as its upper triangle) holds A(n,n)[r][c] - A(n,n)[c][r] for r > c
struct DSlots {
  int L = 0, Lq = 0;        // active slots; 16-B quads per node ([u_of/64][Lq][64])
  int wide = 0;             // 0: 8 bf16 per quad; 1: 4 f32 per quad (some correction not exact in bf16)
  unsigned char s[120];     // ascending active slot ids (at most 117 + 3)
  unsigned short m9[14];    // per lower block nb (13: diagonal): active (r*3+c) bits
  unsigned char pos[14];    // per block: index of its first active slot
  int xc[24];               // slot p < 24: (x offset from 3 * padded index of the row node) * 4 + row
  int dense = 0;            // 1: all 120 slots stored in canonical order (nb*9 + r*3 + c, then the diagonal's
                            // (1,0) (2,0) (2,1)) and applied by a second pass, k_split_dense
  int esc = 0;              // dense bf16 with escapes: a correction not exact in bf16 keeps its truncated bf16
                            // hi in D plus the exact residual d - hi in the escape arrays (Ctx::esc_*)
  int nesc = 0;             // escaped corrections of the current matrix
};

// In-process transport: several contexts (one host thread each) exchanging halos and partial
// sums by device copies + events.  Used to run the multi-rank path on one GPU (tests) and for
// a single process driving several GPUs; the RCCL transport is the multi-process path.
struct LocalGroup {
  int nranks = 0;
  std::vector<Ctx*> members;
  std::vector<hipEvent_t> ev_packed, ev_halo_done, ev_red, ev_sum;
  double** d_red_ptrs = nullptr;   // device array: red_loc of every member
  int device = 0;
  bool dev_ready = false;          // events + d_red_ptrs created (by the first mcx_init_local)
  // host barrier: every crossing is tagged with the collective it belongs to, so members that
  // reach different collectives (one rank finalizing while another exchanges a halo) fail
  // instead of pairing up; a member that never arrives fails the others after timeout_s
  void* mtx = nullptr;
  void* cv = nullptr;
  int count = 0, generation = 0;
  int cur_tag = 0, cur_rank = -1;  // the first arrival of the open generation
  double timeout_s = 300.;         // MCX_COMM_TIMEOUT (seconds) at creation
  bool broken = false;             // a mismatch or a timeout happened: every later crossing fails
  std::string why;                 // ... and what it was
};
// barrier tags (which collective a crossing belongs to)
enum { BAR_INIT = 1, BAR_HALO_PACKED, BAR_HALO_DONE, BAR_RED_IN, BAR_RED_SUM, BAR_FINALIZE, BAR_USER, BAR_MG_ALLOC };
int group_barrier(LocalGroup* g, int rank, int tag, double timeout_s);  // 0, or 23 with the reason in mcx_last_error
double comm_timeout_default();                       // MCX_COMM_TIMEOUT, default 300 s

struct Ctx {
  mcx_opts o;
  int rank = 0, nranks = 1, device = 0;
  int m = 1, n = 1, p = 1, pi = 0, pj = 0, pk = 0;
  std::vector<int64_t> wx, wy, wz, sx, sy, sz;  // ownership widths / starts per rank column
  std::vector<int64_t> rank_node_off;           // nranks + 1
  Geo g{};
  double dy = 0;
  Material mat{};
  hipStream_t stream = nullptr;
  hipStream_t comm_stream = nullptr;            // halo exchange (overlaps interior work on `stream`)
  hipEvent_t ev_pack = nullptr, ev_comm = nullptr;
  int overlap = 1;                              // CG: interior p update overlaps the halo (option halo_overlap)
  void* comm = nullptr;                         // ncclComm_t when nranks > 1 (RCCL transport)
  LocalGroup* lg = nullptr;                     // in-process transport
  double comm_timeout = 300.;                   // seconds a host wait on collective work may take (option comm_timeout)
  bool comm_broken = false;                     // the communicator was aborted (timeout / async error): collectives fail
  std::string comm_why;
  HaloPlan halo;

  // device arrays
  double* u_pad = nullptr;   // displacement, padded ghosted box [PX*PY*PZ][3]
  int pad_align = 1;         // padded box: 1 = row pitch PX a multiple of 16 nodes and node (0, j, k) of
                             // every row at a 128-B line (pad_off 104), 2 = the same pitch with the
                             // ghost column (-1, j, k) at a line (pad_off 0), 0 = PX = nx + 2 (round 4)
  int pad_off = 104;         // bytes from an allocation's base to padded node 0
  std::vector<void*> pad_bases;  // allocations of the padded vectors (freed by base)
  double* p_pad = nullptr;   // CG search direction, padded
  double* p_pad2 = nullptr;  // its second buffer (single rank: the p update fused into the SpMV, cg_fusep)
  double* p_pad3 = nullptr;  // third and fourth buffers (cg_pdb 4), allocated at the first solve that uses them
  double* p_pad4 = nullptr;
  double* p_pad58[4] = {nullptr, nullptr, nullptr, nullptr};  // buffers 5-8 (cg_xs)
  int cg_xs = 0;             // quad-buffered p: the four owed VecAXPY(x) terms on a side stream (option cg_xs)
  bool xs_used = false;      // this solve: eight p buffers, k_cg_xwin on x_stream
  hipStream_t x_stream = nullptr;
  hipStream_t f_stream = nullptr;                  // k_spmv_face beside the march (vi_st_fstream)
  hipEvent_t ev_fx = nullptr, ev_fd = nullptr;     // p ready for the face stream / the faces done
  int vi_st_fstream = 0;                           // option vi_st_fstream
  hipEvent_t ev_xp = nullptr, ev_xd[2] = {nullptr, nullptr};
  int cg_fusep = 0;          // option cg_fusep: fuse the CG p update into the value-indexed SpMV (single rank; A/B: no gain)
  bool fusep_used = false;   // the last solve ran the fused kernel (timing: its bytes per launch)
  int cg_pdb = 4;            // option cg_pdb: 1 = p double-buffered (p_pad / p_pad2), VecAXPY(x) every second
                             // iteration; 4 = four buffers, x every fourth iteration; 0 = one buffer, x every iteration
  bool pdb_used = false;     // the current solve runs the double-buffered p update
  bool pqb_used = false;     // ... the quad-buffered one (cg_pdb 4; pdb_used too)
  int cg_rev = 1;            // option cg_rev: PDB p update from the last node down (the update kernel's last r writes hit the Infinity Cache)
  int cg_par = 1;            // option cg_par: PDB p update specialised per iteration parity (host count cg_it)
  int* xdone = nullptr;      // PDB: the last odd iteration whose p update applied the x terms owed
  int cg_it = 0;             // iteration index of the cg_iteration being launched
  double* b = nullptr;       // residual (owned, PETSc-local order)
  double* du = nullptr;      // CG solution x
  double* r = nullptr;
  double* z = nullptr;
  double* w = nullptr;
  double* dinv = nullptr;    // Jacobi inverse diagonal (inside the jdd buffer: jdd + 3 VI_MAX)
  unsigned char* jix = nullptr;  // block-indexed storage: each owned node's diagonal-block index
  double* jdd = nullptr;         // block-indexed storage: the dictionary's inverse diagonals [VI_MAX][3]
  int cg_dix = 1;                // CG kernels: Jacobi from jix/jdd, z recomputed from r (option cg_dix)
  double* V = nullptr;       // aij stencil-block matrix, AoSoA [ngroups][NPAIR][64] double2
  double* U = nullptr;       // sbaij upper stencil blocks over the padded box [npgroups][UPAIR][64] double2
  uint16_t* D = nullptr;     // AIJ-split: bf16 corrections of the padded box [u_of/64][dsl.Lq][64] x 8
  int64_t D_bytes = 0;       // allocated bytes of D (grown to the active slots' quads)
  unsigned* esc_node = nullptr;   // AIJ-split escapes: per owned node count << 24 | (first entry + 1), 0 = none
  double* esc_res = nullptr;      // escaped corrections' residuals d - hi, a node's entries in slot order
  unsigned char* esc_slot = nullptr;  // their slots (nb*9 + r*3 + c)
  int64_t esc_cap = 0;            // allocated escape entries
  int split_esc = 1;              // option split_esc: dense corrections as bf16 + escapes when some are not bf16-exact
  unsigned* d_mask = nullptr;  // AIJ-split assembly: [0..13] slot masks per lower block, [14] inexact
  // value-indexed AIJ (FMT_VI): index bytes [ngroups][VI_CHUNKS][64] x 16 B, the dictionary
  // (VI_MAX doubles, ascending bit pattern), the build's value set and its slot -> index map
  unsigned char* vi_idx = nullptr;
  int64_t vi_idx_bytes = 0;               // allocated bytes of vi_idx (grown to the mode's 32 / 128 / 256 B per node)
  double* vi_dict = nullptr;
  unsigned long long* vi_keys = nullptr;  // [VI_HASH] the value set, [NSLOT][32] the slots' sets, [VI_HASH] the block set
  unsigned char* vi_slot = nullptr;       // index of every set entry ([VI_HASH] or [NSLOT][32]), then the blocks'
  unsigned* vi_ctl = nullptr;             // [0] distinct values, [1] > VI_MAX, [2] a slot > 16, [3 + S] per slot, blocks'
                                          // [3 + NSLOT] count, [4 + NSLOT] > VI_MAX
  int vi_n = 0;                           // distinct values of the current matrix
  int vi_bits = 8;                        // 4: per-slot nibble indices, 8: one byte per value
  int vi_bits_max = 4;                    // option vi_bits: 8 = never use nibble indices
  bool vi_block = false;                  // one byte per 3x3 block into a dictionary of blocks (k_spmv_vib)
  int vi_block_on = 1;                    // option vi_block: try the block dictionary (needs nibbles)
  int vi_nblocks = 0;                     // distinct blocks of the current matrix (block mode)
  double* vi_bdict = nullptr;             // [VI_MAX][VIB_STRIDE] dictionary blocks
  // single-pass block build (k_vib_build + k_vib_remap): per-slot value sets [NSLOT][VB_GSV] and
  // the block-code set [VI_HASH] (one buffer), its control words, every (block position, owned
  // node)'s block-set position [27][nown], and the pinned host images of what crosses PCIe
  unsigned long long* vib_keys = nullptr;
  unsigned* vib_ctl = nullptr;
  unsigned short* vib_pos = nullptr;
  int64_t vib_pos_bytes = 0;
  unsigned long long* h_vib_keys = nullptr;  // readback: sets + ctl
  unsigned char* h_vib_map = nullptr;        // upload: block-set position -> dictionary index [VI_HASH]
  double* h_vib_dict = nullptr;              // upload: [VI_MAX][VIB_STRIDE]
  int vib_onepass = 1;       // option vib_onepass: the single-pass block build (0: round 2's three passes)
  // exception nodes (per-GP-tangent laws, one-pass block build): an owned node touching an
  // element whose tangent differs from the law's reference tangent at some Gauss point keeps its
  // 27 blocks as plain values, [slot][27][9]; its index chunk carries slot + 1 in bytes 28-31
  unsigned char* elem_plain = nullptr;  // [nelem] 1 = every GP tangent equals cref bit for bit
  double* cref = nullptr;               // [36] the reference tangent (plastic: the elastic branch's C)
  unsigned* vi_xslot = nullptr;         // [nown] exception slot + 1, 0 = indexed node
  int* vi_xlist = nullptr;              // [nown] exception slot -> owned node
  unsigned* vi_xcnt = nullptr;          // [node blocks + 1] exception nodes per block, then their exclusive scan
  double* vi_exc = nullptr;             // block values [slot/64][27 x 9][slot%64] (exc_base)
  int64_t vi_exc_bytes = 0;             // allocated bytes of vi_exc
  int64_t vi_nexc = 0;                  // exception nodes of the current matrix
  bool plain_ke = false;                // this assembly formed kref + the non-plain elements' Ke only
  int vi_exc_max = 300;                 // option vi_exc_max: per-mille of owned nodes beyond which the
                                        // assembly falls back to AIJ-split (0: no exceptions)
  double* ke_uni = nullptr;  // elastic law: the element matrix [8 a][8 b][9], the same for every element
  int aij_vi = 1;            // aij: assemble in FMT_VI when the matrix has at most VI_MAX distinct values
  int vi_fma = 1;            // staged block-indexed SpMV: fused multiply-add rows (-mat_vi_fma, option vi_fma;
                             // rounding-level, not bit-exact); implies vi_uni + vi_patch
  int vi_patch = 1;          // with vi_uni: 16 x 4 node patches per wave (option vi_patch)
  int vi_ring3 = 0;          // A/B: the 3-slot x ring (two barriers per plane) for 64x16 tiles (option vi_ring3)
  int vi_exc_list = VI_EXC_LIST;  // staged block-indexed SpMV: exception nodes per tile deferred to its block pass (option vi_exc_list)
  int vi_wmap = 1;           // staged block-indexed SpMV: 16x4 patches on SIMDs as a Latin square (option vi_wmap; 0: row-major)
  int vi_tx = 0;             // staged block-indexed SpMV tile width 256 | 128 | 64 (0: 64; option vi_tx)
  int vi_uni = 1;            // staged block-indexed SpMV: wave-uniform blocks from scalar loads (option vi_uni)
  int vi_ypair = 0;          // with vi_uni: y of lane pairs as 16-B stores (option vi_ypair; A/B)
  int cg_ublocks = 0;        // k_cg_update grid cap (grid-stride; option cg_ublocks, 0 = one node per thread; A/B)
  int vi_lg = 2;             // staged block-indexed SpMV, LDS-dictionary waves: blocks whose reads are issued together (option vi_lg: 1, 2, 3)
  int cg_p2d = 0;            // quad-buffered p update on a (rows, x chunks) grid: no per-node divisions (option cg_p2d; A/B)
  int vi_lg_exc = 1;         // vi_lg 2 also in the exception-node kernel (option vi_lg_exc; 0: per-block waits)
  int vi_st = -1;            // default-stencil SpMV (k_spmv_st + k_spmv_face, option vi_st; FMA rows, 64 x 16 tiles):
                             // -1 (default) from ST_MIN_NODES owned nodes up or with <= 10 % exception nodes, 0 off, 1 on
  int vi_st_faces = 1;       // the domain faces as stencil classes of their own (option vi_st_faces: 1 all, 0 none (listed), else bit c = class c)
  int vi_st_l16 = -1;        // k_spmv_face's listed rows: 16 lanes per node, loads in parallel (option vi_st_l16 1; 0: one
                             // thread per node, st_tail; -1: 16 lanes while the list is short, kernels.hip st_l16)
  int vi_st_pf = 1;          // k_spmv_st's prefetch distance in steps (option vi_st_pf 1 | 2)
  int vi_st_ty = 16;         // k_spmv_sp's tile height (option vi_st_ty: 8 = 512-thread blocks, two per CU; 16 = 1024)
  int vi_st_pair = 0;        // the march as k_spmv_sp (x-pair lanes, round 6; option vi_st_pair 1; the fused p update
                             // on this path needs it): 0.2920 vs 0.2757 ms for k_spmv_st + k_spmv_face (r06t)
  int vi_st_tail = 0;        // its faces and listed rows in the march's blocks after the march (option vi_st_tail; 0: k_spmv_face)
  int vi_st_dma = -1;        // the march as k_spmv_st_dma (direct-to-LDS staging, 5-slot ring; option vi_st_dma): -1 / 1 where
                             // eligible (kernels.hip st_dma_ok), 0 off; same rows bitwise
  int st_dma_last = 0;       // the last SpMV launched k_spmv_st_dma (mcx_get_st_dma)
  double* st_coef = nullptr;            // [ST_CLASSES][27][VIB_STRIDE] the stencil classes' blocks
  unsigned* st_ids = nullptr;           // [ST_CLASSES][8] their 7 index words, [7] = class usable
  unsigned* st_slot = nullptr;          // [nown] list position + 1 of a non-default node, 0 = default
  int* st_list = nullptr;               // [nown] non-default nodes in owned-node order
  unsigned* st_cnt = nullptr;           // [node blocks + 1] scan scratch
  unsigned long long* st_mask = nullptr;  // [nz][npy][npx] 16 x 4 patch masks (bit = the march leaves the lane: faces, listed rows)
  int64_t st_mask_bytes = 0, st_n = 0;
  int st_npx = 0, st_npy = 0;
  bool st_ok = false;                   // built for the current block indices
  bool st_pending = false;              // not built: the last assembly's SpMV did not want the path
  unsigned st_fm = 0;                   // bit c: stencil class c usable (k_st_setup)
  StFaces st_faces = {};                // the face phase's units per class
  int vi_exc_kernel = 1;     // staged SpMV: exception rows in their own kernel after the march (k_spmv_exc, option
                             // vi_exc_kernel; 0: round 4's block-wide pass in each tile's tail)
  int vi_wdesc = 1;          // staged block-indexed SpMV: wave descriptors (option vi_wdesc): 1 = uniform waves (default since round 5: -2.1 % per CG iteration), 2 = also two-set waves (FMA rows), 0 = per-lane index words
  unsigned* wd = nullptr;    // wave descriptors [plane][npy][npx][8] + 2 counters (build_wdesc)
  int64_t wd_bytes = 0;
  bool wd_ok = false;        // descriptors built for the current block indices
  int wd_npx = 0, wd_npy = 0;
  int64_t wd_blocks_fma = 0, wd_blocks_exact = 0, wd_blocks_two = 0;  // present blocks of the nodes in waves that read per-lane words
  int vi_xread = 1;          // staged block-indexed SpMV: x as unpaired 8-B LDS reads (option vi_xread; 0: compiler's pairs)
  int vi_stage = -1;         // FMT_VI SpMV: 1 = x staged in LDS, z-marching tiles; 0 = x gathered; -1 = by grid (vi_staged)
  bool vi_declined = false;  // a per-GP-tangent law overflowed the dictionary: skip the attempt
  int fmt = FMT_V;           // storage the matrix is currently assembled in
  bool assembled = false;    // a matrix has been assembled (mcx_assembly_jac)
  int aij_split = 1;         // aij: assemble in FMT_SPLIT when every correction is exact in bf16
  int split_maxq = 4;        // AIJ-split only while the corrections fit this many 16-B quads per node
  int split_dense = 1;       // corrections beyond split_maxq quads: 1 = all 120 slots + a second pass, 0 = AIJ blocks
  bool split_declined = false;  // a correction was not exact (or dense ones are refused): assemble AIJ blocks directly
  int split_dbg = 0;         // timing-only diagnostics of the split SpMV (option split_dbg)
  int face_dbg = 0;          // timing-only: k_spmv_face without (1) listed rows, (2) x-face, (4) y/z-face patches
  int split_wide = 0;        // force f32 corrections (testing the wide path)
  int split_tx = 0;          // AIJ-split tile width (0: by subdomain width, 4 rows; else 1024 / split_tx rows)
  int split_ty = 0;          // AIJ-split: 2 with split_tx 256 selects 256x2 tiles (option split_ty)
  DSlots dsl;
  int64_t npgroups = 0;
  int64_t nupper_local = 0;  // sbaij: stored upper values of the owned rows
  int spmv_subl = 0;         // SpMV sweep: lines per sub-slab of an XCD's slab (0 = whole slab, -1 = linear order)
  int spmv_kernel = 0;       // sbaij: 0 = pull, 1..4 = z-marching push/pull tiles (shapes, see z_shape)
  int cg_nt = 0;             // CG vector kernels: non-temporal stores of x, r, z, p
  int spmv_zblocks = 0;      // z-marching: target block count (0: one resident round, CUs x blocks/CU)
  int ncu = 0;               // compute units of the device
  int spmv_nt = 2;           // aij: 1 = non-temporal matrix loads, 2 = + non-temporal y stores (-3 %, spmv_ab)
  int64_t partials_cap = 0;
  double* eps = nullptr;     // [6][8][nelem]
  double* sig = nullptr;     // [6][8][nelem]
  double* ctan = nullptr;    // [36][8][nelem] per-GP tangent (plastic / external laws only)
  double* Ke = nullptr;      // [576][nelem] element matrices (plastic / external laws only)
  double* hist_old = nullptr; // plastic law: [7][8][nelem] plastic strain (tensor comps) + alpha
  double* hist_new = nullptr;
  double* ftrial = nullptr;  // [8][nelem]
  double* partials = nullptr;
  double* partials2 = nullptr;  // second half of partials: the CG update's z.z / z.r partial sums
  int fuse = 1;              // single rank: CG scalar steps folded into the vector kernels (option cg_fuse)
  double* red = nullptr;     // reduction results (device)
  double* red_loc = nullptr; // local sums before all-reduce
  CgState* cg = nullptr;     // [2]: cg[0] the state the host polls; cg[1] the fused path's post-alpha state
  double* hist = nullptr;
  double* tmp = nullptr;     // owned-vector scratch for host copies
  CgState* h_cg = nullptr;   // pinned mirror
  int64_t ngroups = 0;
  int64_t device_bytes = 0;
  int64_t nnz_local = 0, nnz_global = 0;

  // -mat_law micro: the cell's two materials and solver settings, the homogenised tangent (also in
  // mat.C) with each load case's CG iterations and final relative norm; dirty = C_hom has to be
  // (re)computed before it is next used (after init, mcx_material_set, a micro_* option)
  MicroArgs micro{};
  int micro_max_it = 0;      // option micro_max_it (0: 10 x interior dofs)
  bool micro_dirty = true;
  double* micro_out = nullptr;  // device [6][MICRO_OUT]
  int micro_its[6] = {};
  double micro_rnorm[6] = {};
  // option micro_mem: 0 the cell solvers' nodal vectors in LDS, 1 in device memory:
  // k_micro_rve's six workspaces and k_mnl_solve's mnl_ws_blocks workspaces (allocated when first
  // needed, sized by n; the block count does not grow with the number of points)
  int micro_mem = 0;
  double* micro_ws = nullptr;  // [6][5][3 n^3]
  double* mnl_ws = nullptr;    // [mnl_ws_blocks][6][3 n^3]
  int64_t micro_ws_bytes = 0, mnl_ws_bytes = 0;
  int mnl_ws_blocks = 0;       // min(2 x compute units, local Gauss points)
  int mnl_ws_blocks_opt = 0;   // option micro_mem_blocks (testing the walk): > 0 replaces 2 x compute units
  // option micro_solver: 0 k_micro_rve (one workgroup per load case, micro_mem decides
  // where its vectors live), 1 the grid-wide solver (-mat_law micro only, micro_n <= MICRO_NMAX_GRID);
  // micro_grid_poll = CG iterations enqueued between two host polls of the six done flags
  int micro_solver = 0, micro_grid_poll = 16;
  double* micro_grid_ws = nullptr;  // mg_ws_bytes(n), allocated at the solver's first use; under micro_nl_solver 1
                                    // the larger of that and mnlg_ws_bytes: the two solvers never run together
  int64_t micro_grid_bytes = 0;

  // -mat_law micro_nl: phase Sy / Ka and the Newton settings; the unit-strain fields' strain
  // concentration tensors (with C_hom, after ensure_micro); the slot of every local Gauss point
  // (-1: linear shortcut), the compacted list of points to solve, the pool (allocated at the first
  // non-linear point) and each point's solver record
  double mnl_Sy[2] = {}, mnl_Ka[2] = {};
  double mnl_rtol = 1e-10;
  int mnl_max_it = 20;
  // option micro_nl_solver: 0 k_mnl_solve (one workgroup per listed point), 1 the grid-wide
  // solver: C_hom by the k_mg_* sequence, the listed points by the k_mnlg_* launches, micro_n <=
  // MICRO_NMAX_NL_GRID; micro_mem is ignored, micro_mem_blocks > 0 replaces the solves per launch
  int mnl_solver = 0;
  int mnl_start = 0, mnl_ls = 0;  // options micro_nl_start, micro_nl_ls: the globalised Newton loop
  // option micro_nl_tangent: 1 = solver 1 advances a point's six tangent columns together;
  // mnl_col_its: [6][ngp] the columns' CG iterations of the points the last call solved that way (else 0)
  int mnl_tangent = 0;
  std::vector<int> mnl_col_its;
  // option micro_nl_apply: 1 = solver 1 forms a CG iteration's q = K_T p and p.q in one launch
  // (k_mnlg_apply / k_mnlb_apply) that never writes the work stresses; the launches of the last mcx_homogenize
  int mnl_apply = 0;
  long long mnl_apply_launches = 0;
  // option micro_nl_warm: solver 1 starts a slotted point's Newton loop and tangent columns
  // from the slot's warm record; the store ([mnl_cap] fields, then [mnl_cap] headers) exists while the
  // option is 1 and a pool exists; mnl_warm_hit: [ngp] the points the last call solved from their record
  int mnl_warm = 0;
  double* mnl_warm_store = nullptr;
  int64_t mnl_warm_store_bytes = 0;
  std::vector<char> mnl_warm_hit;
  int mnl_last_nsolve = 0;  // the points the last mcx_homogenize listed (mnl_list)
  int64_t mnl_slots_opt = 0;     // option micro_nl_slots (0: what fits 2 GiB, at most the local Gauss points)
  int64_t mnl_cap = 0, mnl_used = 0;
  double* mnl_ufield = nullptr;  // [6][3 n^3] unit-strain solutions
  double* mnl_conc = nullptr;    // [MNL_CONC][8 (n-1)^3]
  int64_t mnl_ufield_bytes = 0, mnl_conc_bytes = 0;  // sized by the cell in use (ensure_micro)
  int* mnl_slot = nullptr;       // [ngp]
  int* mnl_list = nullptr;       // [ngp] points to solve, ascending
  int* mnl_cnt = nullptr;        // [2] new points, points to solve
  int* mnl_its = nullptr;        // [4][ngp] Newton iterations, CG iterations, status (0 ok, 1 Newton, 2 CG), rejected trials
  double* mnl_rn = nullptr;      // [2][ngp] final relative Newton residual, smallest accepted step length
  double* mnl_pool = nullptr;    // [mnl_cap][MNL_WS][8 (n-1)^3]

  // options pc_type (0 Jacobi, 1 multigrid), pc_mg_levels (0: automatic), pc_mg_smooth (Chebyshev degree)
  int pc_type = 0, pc_mg_levels = 0, pc_mg_smooth = 2;
  int pc_mg_dist = 0;  // option pc_mg_dist: 1 accepts pc_type 1 on a context with a communicator
  int pc_mg_precision = 0;  // option pc_mg_precision: 1 keeps the levels >= 1 of the hierarchy in float
  Pcmg mg;

  // external Gauss-point law (-mat_law external): host MicroPP-shaped callbacks or a device law
  mcx_micropp_api mpp{};
  bool has_mpp = false;
  mcx_device_law dlaw{};
  bool has_dlaw = false;
  std::vector<double> h_gp;  // host staging of eps / sig / ctan for the host callbacks

  // timing
  bool timing = false;
  mcx_timing t{};
  std::vector<hipEvent_t> ev_pool;
  hipEvent_t ev_a = nullptr, ev_b = nullptr;
  // per-phase event pairs (strains, homogenize, residual, jacobian, solve, update): recorded
  // without a host wait, resolved by mcx_get_timing
  hipEvent_t ev_phase[6][2] = {};
  bool phase_rec[6] = {};
  hipEvent_t ev_chunk[2] = {nullptr, nullptr};
  int last_its = 0;
  std::vector<double> last_hist;
};

// ---- decomposition (dmda.cpp)
int dmda_decide(int64_t M, int64_t N, int64_t P, int size, int* m, int* n, int* p);
int setup_decomposition(Ctx& c);
int64_t petsc_node(const Ctx& c, int64_t i, int64_t j, int64_t k);
// the ghost fill of a box of n owned nodes in a padded vector of row pitch PX and plane pitch PXY
// (the neighbours are the rank grid's); *bytes grows by the device memory taken
int build_halo_plan(Ctx& c, HaloPlan& h, const int n[3], int PX, int PXY, int64_t* bytes);
void free_halo_plan(HaloPlan& h);
void plan_halo(const Ctx& c, HaloPlan& h, const int n[3], int PX, int PXY, std::vector<int>& sidx, std::vector<int>& ridx);
int64_t pad_to_natural(const Ctx& c, int p);
int64_t count_nnz_rows(const Ctx& c, int64_t xs, int64_t ys, int64_t zs, int64_t nx, int64_t ny, int64_t nz);
void compute_B_table(double B[8][6][24]);
int64_t count_upper_values(const Ctx& c);

// ---- communication (comm.cpp)
int comm_init(Ctx& c, const void* id);
void comm_destroy(Ctx& c);
// xpad: double, or float for the plan of a float level of the multigrid (h.esz 4)
int halo_exchange(Ctx& c, HaloPlan& h, void* xpad);   // halo_start + halo_finish
int halo_start(Ctx& c, HaloPlan& h, void* xpad);      // pack + exchange on the comm stream
int halo_finish(Ctx& c, HaloPlan& h, void* xpad);     // compute stream waits, unpacks
// the context's own plan: its padded vectors (u, p, the multigrid's level 0)
inline int halo_exchange(Ctx& c, double* xpad) { return halo_exchange(c, c.halo, xpad); }
inline int halo_start(Ctx& c, double* xpad) { return halo_start(c, c.halo, xpad); }
inline int halo_finish(Ctx& c, double* xpad) { return halo_finish(c, c.halo, xpad); }
int allreduce_sum(Ctx& c, const double* in, double* out, int count);
int allreduce_max(Ctx& c, const double* in, double* out, int count);
// the multigrid's large sums (pc_mg_dist): in = mg.arin of every rank, up to mg.ar_cap doubles
int allreduce_sum_mg(Ctx& c, double* out, int count);
int allreduce_prepare(Ctx& c);
// host wait for work that depends on other ranks (CG chunk polls, all-reduced norms): the RCCL
// transport polls the event and the communicator's asynchronous error against c.comm_timeout and
// aborts the communicator on either; one rank without a communicator waits plainly
int comm_wait(Ctx& c, hipEvent_t ev, const char* what);
int comm_check(Ctx& c);  // a communicator aborted earlier: fail the collective
int comm_query(Ctx& c, int* n, int* r, int* dev);  // ncclCommCount / UserRank / CuDevice (1, 0, device: none)
int group_setup(Ctx& c);  // the in-process group's events (first member on the device)
void launch_group_sum(Ctx& c, const double* const* ptrs, int nranks, int count, double* out, int op = 0);
void launch_vtu_cells(Ctx& c, const int* lo, const int* cnt, double* out);
void launch_force_layer(Ctx& c, int comp, int fa, int fixed, int a0, int na, int b0, int nb, double* out);

// ---- kernel launchers (kernels.hip)
int upload_constants(Ctx& c);
void launch_apply_bc_u(Ctx& c, double U);
void launch_strains(Ctx& c);
void launch_homogenize(Ctx& c);
void launch_residual(Ctx& c);          // b + partial sums of b.b
void launch_element_ke(Ctx& c);        // Ke of a per-GP-tangent law
int launch_plain_ke(Ctx& c);           // plain elements, kref, the other elements' Ke (exception-node build)
void launch_elastic_ke(Ctx& c);        // the elastic law's one element matrix (ke_uni); -mat_law micro: from C_hom
void launch_micro_rve(Ctx& c, const MicroArgs& m);  // the six unit-strain solves of the micro cell -> micro_out
// option micro_solver 1: the same six solves, grid-wide
MicroGridWs mg_layout(double* base, int n);
void launch_mg_setup(Ctx& c, const MicroArgs& m, const MicroGridWs& w);   // Ke, x, D^-1, r0, p0, the first norm
void launch_mg_iterate(Ctx& c, const MicroArgs& m, const MicroGridWs& w);  // one gated CG iteration
void launch_mg_finish(Ctx& c, const MicroArgs& m, const MicroGridWs& w);  // average stresses, state -> micro_out
// -mat_law micro_nl
void launch_mnl_conc(Ctx& c, const MicroNlArgs& a);    // mnl_ufield -> mnl_conc
void launch_mnl_linear(Ctx& c, const MicroNlArgs& a);  // linear test, sigma = C_hom eps, compaction -> mnl_cnt
void launch_mnl_solve(Ctx& c, const MicroNlArgs& a, int nsolve);
// option micro_nl_solver 1: the listed points base .. base + cnt - 1, grid-wide
MnlGridWs mnlg_layout(double* base, int n, int64_t batch);
void launch_mnlg_start(Ctx& c, const MnlGridWs& w, int base, int cnt);
void launch_mnlg_transition(Ctx& c, const MicroNlArgs& a, const MnlGridWs& w, int cnt);  // CG ended -> next CG started
void launch_mnlg_iterate(Ctx& c, const MicroNlArgs& a, const MnlGridWs& w, int cnt);     // one gated CG iteration
// option micro_nl_tangent 1: the same two with the six columns as one block (bw behind w's layout)
MnlBlockWs mnlb_layout(double* base, int n, int64_t batch);
void launch_mnlb_transition(Ctx& c, const MicroNlArgs& a, const MnlGridWs& w, const MnlBlockWs& bw, int cnt);
void launch_mnlb_iterate(Ctx& c, const MicroNlArgs& a, const MnlGridWs& w, const MnlBlockWs& bw, int cnt);
void launch_mnl_commit(Ctx& c, const MicroNlArgs& a);  // new history -> committed history, used slots
void launch_gather_matrix(Ctx& c);
void launch_gather_matrix_sym(Ctx& c);
int build_split(Ctx& c, bool* exact);  // AIJ-split corrections from U (exact = usable)
int build_vi(Ctx& c, bool* ok);        // value-indexed AIJ (ok = at most VI_MAX distinct values)
void launch_jacobi(Ctx& c);
void launch_spmv(Ctx& c, const double* xpad, double* y, bool dot, bool gated);
void launch_update_u(Ctx& c);
int launch_cg_xfinal(Ctx& c);
void launch_cg_pupdate(Ctx& c, int part);  // 0 all owned nodes, 1 the sent (subdomain-face) nodes, 2 the rest
void launch_reduce(Ctx& c, int nvals, int nparts, double* out);
void launch_cg_init(Ctx& c);
int cg_iteration(Ctx& c, hipEvent_t spmv_start, hipEvent_t spmv_stop, bool first, bool last);
int cg_finish_init(Ctx& c);
void launch_pack(Ctx& c, const HaloPlan& h, const void* xpad);  // xpad: double, or float for a plan with esz 4
void launch_unpack(Ctx& c, const HaloPlan& h, void* xpad);
void launch_copy_owned_to_pad(Ctx& c, const double* owned, double* pad);
void launch_copy_pad_to_owned(Ctx& c, const double* pad, double* owned);
int64_t spmv_grid_blocks(const Ctx& c);
int64_t spmv_nparts(const Ctx& c);
bool partials_fit(const Ctx& c);     // the SpMV's and the node blocks' partials fit half the buffer
bool st_wanted(const Ctx& c);        // option vi_st asks for the default-stencil SpMV   // partial sums the CG's SpMV leaves (its own grid, or the dense pass's)
int64_t node_blocks(const Ctx& c);
bool vi_staged(const Ctx& c);
int build_wdesc(Ctx& c);    // wave descriptors of the block-indexed storage (after build_vi)
bool wd_used(const Ctx& c);  // the staged SpMV reads them
int build_st(Ctx& c);       // default-stencil SpMV structures (after build_vi)
bool st_used(const Ctx& c);  // the SpMV runs k_spmv_st + k_spmv_face
bool fusep(const Ctx& c);  // the CG's p update runs inside the value-indexed SpMV
bool cg_pdb(const Ctx& c);  // the CG's p update double-buffered (x every second iteration)
int64_t cg_vec_bytes_per_node(const Ctx& c);  // the last solve's CG vector kernels, bytes per owned node and iteration
// z-marching SpMV tile of the current storage (tx, ty, planes per chunk); all 0 for gathered kernels
void spmv_tile(const Ctx& c, int* tx, int* ty, int* kc);
int dirichlet_mask_host(const Geo& g, int gi, int gj, int gk);

// ---- -pc_type mg: kernels (kernels.hip) and the hierarchy, cycle and PCG loop (pcmg.cpp)
void launch_pcmg_mask0(Ctx& c, unsigned char* mask);
// A level's vectors and operator come as PcmgVec: the launchers start the kernel's instantiation for
// the storage type they carry.
// xf (layout lx) = or += P xc; probe >= 0: xc (null) is the indicator of colour probe / 3, component probe % 3
// xc in layout lc
void launch_pcmg_prolong(Ctx& c, const PcmgXfer& t, const PcmgLay& lx, const PcmgLay& lc, PcmgVec xc, int probe,
                         const unsigned char* fmask, PcmgVec xf, bool add);
// bc = P^T (b - w), b in layout lb; w and fmask (owned order) may be null: pc_mg_dist hands over the
// masked residual in a padded box, ghosts filled
void launch_pcmg_restrict(Ctx& c, const PcmgXfer& t, const PcmgLay& lb, PcmgVec b, PcmgVec w, const unsigned char* fmask,
                          PcmgVec bc);
// r = b - A x (b null: A x), x in layout lx
void launch_pcmg_spmv(Ctx& c, const PcmgLevel& l, const PcmgLay& lx, PcmgVec x, PcmgVec b, PcmgVec r);
void launch_pcmg_scatter(Ctx& c, const PcmgLevel& l, const PcmgLay& lx, PcmgVec t, int colour, int d);
// pc_mg_dist: rp (layout lx, padded) = b - w (w null: b) with the level's Dirichlet dofs zeroed by their owner
void launch_pcmg_resid(Ctx& c, const PcmgLay& lx, int64_t nn, PcmgVec b, PcmgVec w, const unsigned char* mask,
                       PcmgVec rp);
// pc_mg_dist, the coarsest level: owned vector -> its entries of the level's global vector; the global
// vector -> the rank's padded box, ghosts included (0 outside the grid); owned operator blocks -> global
// [243][NN].  The global side is double always
void launch_pcmg_to_full(Ctx& c, const PcmgLay& lx, int64_t nn, PcmgVec v, double* full);
void launch_pcmg_from_full(Ctx& c, const PcmgLay& lx, const double* full, PcmgVec xpad);
void launch_pcmg_blocks_to_full(Ctx& c, const PcmgLevel& l, const PcmgLay& lx, int64_t NN, double* full);
void launch_pcmg_diag(Ctx& c, const PcmgLevel& l);
void launch_pcmg_cheb(Ctx& c, const PcmgLay& lx, int64_t nn, PcmgVec b, PcmgVec w, PcmgVec dinv, PcmgVec d, PcmgVec x,
                      double ca, double cb, bool dfirst, bool xzero);
void launch_pcmg_gemv(Ctx& c, int n, const double* ainv, PcmgVec b, PcmgVec x);  // x = Ainv b; b and x of one type
void launch_pcmg_seed(Ctx& c, const PcmgLay& lx, int64_t nn, PcmgVec x);
int launch_pcmg_scale_dot(Ctx& c, int64_t nn, PcmgVec dinv, PcmgVec w, PcmgVec y);  // y = dinv w, c.red[0] = y.y (all ranks')
void launch_pcmg_scaleto(Ctx& c, const PcmgLay& lx, int64_t nn, PcmgVec y, double s, PcmgVec x);
int launch_pcmg_dot(Ctx& c, const PcmgLay& la, int64_t nn, const double* a, const double* b);  // c.red[0] = a.b (all ranks')
void launch_pcmg_aypx(Ctx& c, int64_t n, const double* z, double bc, double* p, bool first);  // p = z + bc p
void launch_pcmg_xr(Ctx& c, const PcmgLay& lp, int64_t nn, double a, const double* p, const double* w, double* x,
                    double* r);  // x += a p, r -= a w
void launch_pcmg_jacobi(Ctx& c, int64_t n, const double* r, const double* dinv, double* z);  // z = r dinv
PcmgLay pcmg_lay_nat(const int n[3]);
PcmgLay pcmg_lay_pad(const Ctx& c);
PcmgLay pcmg_lay_box(const PcmgLevel& v);  // level >= 1 under pc_mg_dist: the box plus one ghost layer
bool pcmg_dist(const Ctx& c);  // pc_mg_dist on a context with a communicator: the distributed hierarchy
int pcmg_dims(const Ctx& c, int levels, int* nlev, int n[][3]);  // the (global) level sizes; levels 0: automatic
int pcmg_plan_ctx(const Ctx& c, int levels, PcmgPlan* P);  // the context's plan (one box per level), checked; 0 or 2
int pcmg_check(Ctx& c, int levels);  // option check: one rank or pc_mg_dist, the levels exist, the coarsest one fits
void pcmg_free(Ctx& c);
int pcmg_ensure(Ctx& c);                                // build or rebuild the hierarchy for the current matrix
int pcmg_apply(Ctx& c, const double* r_owned);          // mg.L[0].x (padded) = M^-1 r
int pcmg_solve(Ctx& c, int* its, double* rnorm, int* reason);

}  // namespace mcx

// Every extern "C" entry is a function-try-block: no C++ exception (std::bad_alloc from a host
// vector, std::system_error from the group barrier's mutex, ...) crosses the C ABI.  The handler
// stores the message for mcx_last_error and returns MCX_EXC (the PetscErrorCode contract of the
// functions the entries replace).  MCX_ENTRY is the test hook: MCX_TEST_THROW=<entry name> in the
// environment makes that entry throw std::bad_alloc at its start (tests/test_abi.py).
namespace mcx {
constexpr int MCX_EXC = 90;
int exc_return(const char* fn, const char* what);
void test_inject(const char* fn);
}  // namespace mcx
#define MCX_ENTRY() mcx::test_inject(__func__)
#define MCX_CATCH                                                                      \
  catch (const std::exception& e_) {                                                   \
    return mcx::exc_return(__func__, e_.what());                                       \
  }                                                                                    \
  catch (...) {                                                                        \
    return mcx::exc_return(__func__, "unknown exception");                             \
  }

#define MCX_HIP(call)                                                                  \
  do {                                                                                 \
    hipError_t e_ = (call);                                                            \
    if (e_ != hipSuccess) {                                                            \
      mcx::set_error(std::string(#call) + ": " + hipGetErrorString(e_) + " @" +        \
                     __FILE__ + ":" + std::to_string(__LINE__));                       \
      return 10;                                                                       \
    }                                                                                  \
  } while (0)
