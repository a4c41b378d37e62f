/*
 * macroc_amd.h — C-ABI of the MI355X-native MacroC Newton inner loop.
 *
 * One context = one MPI-style rank = one GPU subdomain of the DMDA box decomposition.
 * Every entry point returns 0 on success and a non-zero code on failure, mirroring the
 * reference's PetscErrorCode convention (src/assembly.c:37-42 ... CHKERRQ); the message of
 * the last failure (per calling thread) is available from mcx_last_error().  No C++ exception
 * crosses this interface: an internal one (e.g. a failed host allocation) returns 90 with its
 * message.  Multi-rank host waits (CG polls, all-reduced norms, the in-process group's barrier
 * inside collective entries) are bounded: after the context's "comm_timeout" option (default
 * MCX_COMM_TIMEOUT seconds at mcx_init, else 300), or on an RCCL asynchronous
 * error, the communicator is aborted and the call returns 24 / 25 naming the rank and the
 * operation; later collectives of that context fail at once.  Host buffers are caller-owned;
 * the context owns all device memory.  A context is not thread-safe; different contexts
 * may be driven from different threads.  No torch / HIP types appear in this interface.
 *
 * Reference interface each entry replaces (paths relative to GG1991/macroc):
 *   mcx_default_opts / mcx_parse_args  <- init() defaults + PetscOptionsGet, DMSetFromOptions,
 *                                         KSPSetFromOptions   src/init.c:47-83,93,156
 *   mcx_init                          <- init() grid/Mat/Vec/KSP part  src/init.c:85-171,
 *                                         bc_init src/bcs.c:154-195
 *   mcx_finalize                      <- finish()  src/init.c:222-237
 *   mcx_get_displacement              <- get_displacement  src/bcs.c:52-58
 *   mcx_apply_bc_u                    <- apply_bc_on_u  src/bcs.c:29-45 (-> :61-146)
 *   mcx_set_strains                   <- set_strains  src/assembly.c:25-66
 *   mcx_homogenize                    <- micropp_C_homogenize  src/main.c:62 (device-batched
 *                                         constitutive callback, see mcx_material_set)
 *   mcx_assembly_res                  <- assembly_res + VecNorm  src/assembly.c:120-176,
 *                                         src/main.c:67
 *   mcx_assembly_jac                  <- assembly_jac + apply_bc_on_jac  src/assembly.c:69-117,
 *                                         src/bcs.c:341-347
 *   mcx_solve                         <- solve_Ax -> KSPSolve(CG, Jacobi)  src/assembly.c:179-192
 *   mcx_update_u                      <- VecAXPY(u, 1., du)  src/main.c:79
 *   mcx_material_set                  <- micropp_C_material_set  src/init.c:196-201
 *   mcx_set_micropp / mcx_set_device_law / mcx_set_gp_stress / mcx_set_gp_ctan
 *                                     <- the MicroPP C-wrapper boundary itself: micropp_C_set_strain3
 *                                        src/assembly.c:59, micropp_C_homogenize src/main.c:62,
 *                                        micropp_C_get_stress3 src/assembly.c:149,
 *                                        micropp_C_get_ctan3 src/assembly.c:92,
 *                                        micropp_C_update_vars src/main.c:83,
 *                                        micropp_C_get_non_linear_gps / _get_f_trial_max
 *                                        src/util.c:71,96 (-mat_law external)
 */
#ifndef MACROC_AMD_H
#define MACROC_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCX_COMM_ID_BYTES 128 /* size of an ncclUniqueId */

/* ABI revision of this header.  Revision 3 (round 6) adds mcx_abi_version and mcx_comm_info;
   revision 2 (round 5) grew the structs mcx_info by st_listed and mcx_timing by cg_vec_bytes_per_iter, so a
   caller built against an older header passes smaller structs: check
   mcx_abi_version() == MCX_ABI_VERSION before calling mcx_get_info / mcx_get_timing / mcx_plan. */
#define MCX_ABI_VERSION 3

enum { MCX_BC_BENDING = 0, MCX_BC_CIRCLE = 1 }; /* include/macroc.h:58 */

/* KSPConvergedReason (PETSc) */
enum {
  MCX_KSP_CONVERGED_ITERATING = 0,
  MCX_KSP_CONVERGED_RTOL = 2,
  MCX_KSP_CONVERGED_ATOL = 3,
  MCX_KSP_DIVERGED_ITS = -3,
  MCX_KSP_DIVERGED_DTOL = -4,
  MCX_KSP_DIVERGED_INDEFINITE_PC = -8,
  MCX_KSP_DIVERGED_NANORINF = -9,
  MCX_KSP_DIVERGED_INDEFINITE_MAT = -10
};

/* matrix storage: -dm_mat_type aij (default, the reference's MATAIJ, src/init.c:92) or
   sbaij (PETSc MATSBAIJ semantics with -mat_ignore_lower_triangular: upper triangle kept,
   lower triangle mirrored from it) */
enum { MCX_MAT_AIJ = 0, MCX_MAT_SBAIJ = 1 };

/* constitutive laws behind the Gauss-point callback (-mat_law elastic|plastic|external|micro|micro_nl):
   device isotropic elastic, device J2 plasticity (MicroPP material type 1), an external law
   registered through mcx_set_micropp / mcx_set_device_law / mcx_set_gp_stress+ctan, or the linear
   two-phase micro cell (-micro_n, -micro_type, -micro_mat_1/2) homogenised on the device: one
   tangent C_hom, sigma = C_hom eps at every Gauss point (mcx_micro_get_ctan); micro_nl: the same
   cell with J2-plastic phases, solved per Gauss point (below) */
enum { MCX_LAW_ELASTIC = 0, MCX_LAW_PLASTIC = 1, MCX_LAW_EXTERNAL = 2, MCX_LAW_MICRO = 3, MCX_LAW_MICRO_NL = 4 };

typedef struct {
  int64_t NX, NY, NZ;          /* -da_grid_x/y/z          (default 40 3 40, include/macroc.h:44-46) */
  int px, py, pz;              /* -da_processors_x/y/z    (0 = PETSC_DECIDE) */
  double lx, ly, lz;           /* -lx -ly -lz             (50 1 50) */
  double dt, final_time;       /* -dt                     (0.001, FINAL_TIME 1.0) */
  int ts;                      /* -ts                     (1) */
  int vtu_freq;                /* -vtu_freq               (-1: no VTU output; mcx_write_vtu) */
  int bc_type;                 /* -bc_type                (BC_CIRCLE) */
  double rad;                  /* load-circle radius      (1.0, src/init.c:141) */
  int newton_max_its;          /* -newton_max_its         (5) */
  double newton_min_tol;       /* -newton_min_tol         (0.1) */
  double newton_rel_tol;       /* -newton_rel_tol         (1e-4) */
  double ksp_rtol, ksp_abstol, ksp_dtol; /* -ksp_rtol -ksp_atol -ksp_divtol (1e-5 1e-50 1e4) */
  int ksp_max_it;              /* -ksp_max_it             (10000) */
  int micro_n, micro_type;     /* -micro_n -micro_type    (2, 1) */
  double micro_mat_1[4];       /* -micro_mat_1 E,nu,Sy,Ka (1e7,.25,1e4,1e7) */
  double micro_mat_2[4];       /* -micro_mat_2 */
  int device;                  /* HIP device of this rank (-1: rank % device count) */
  int ksp_monitor;             /* -ksp_monitor: keep the residual history */
  int mat_type;                /* -dm_mat_type aij|sbaij  (MCX_MAT_AIJ) */
  int mat_law;                 /* -mat_law elastic|plastic|external|micro|micro_nl (MCX_LAW_ELASTIC; plastic = J2
                                  with micro_mat_1's Sy, Ka: MicroPP material type 1; micro = the
                                  two-phase micro cell homogenised on the device) */
  int mat_aij_split;           /* -mat_aij_split 0|1 (1): hold the AIJ matrix exactly as upper blocks +
                                  bf16 lower corrections when all are exact (else plain AIJ blocks);
                                  0: AIJ blocks, rows summed in the reference's MatMult order (inode column pairs) (bit-exact SpMV) */
  int mat_aij_vi;              /* -mat_aij_vi 0|1 (1): hold the AIJ matrix exactly as one index byte per
                                  value into a dictionary of its distinct values when there are at most
                                  256 (value-indexed AIJ; rows summed in the reference's MatMult order (inode column pairs), bit-exact
                                  SpMV); otherwise -mat_aij_split decides */
  int mat_vi_fma;              /* -mat_vi_fma 0|1 (1): the value-indexed SpMV's z-marching kernel sums
                                  each row with fused multiply-adds (one rounding per term, what a
                                  PETSc built with -march=native does in MatMult), rows within
                                  1e-14 sum|a_ij x_j| of the reference's MatMult order (inode column pairs); 0: separate multiply and
                                  add in the reference's MatMult order (inode column pairs) (bit-exact SpMV) */
} mcx_opts;

typedef struct {
  int64_t NX, NY, NZ;
  int px, py, pz;              /* rank grid actually used */
  int rank, nranks;
  int64_t xs, ys, zs, nx, ny, nz;   /* owned node corners (DMDAGetCorners) */
  int64_t Xs, Ys, Zs, Nx, Ny, Nz;   /* ghost corners (DMDAGetGhostCorners) */
  int64_t ndofs_global;
  int64_t ndofs_local;          /* 3*nx*ny*nz, PETSc-global rows owned */
  int64_t dof_offset;           /* first global PETSc row of this rank */
  int64_t nnz_local;            /* AIJ nonzeros of the owned rows (pattern of DMCreateMatrix) */
  int64_t nnz_global;
  int64_t nelem_local;          /* DMDAGetElementsSizes product (PETSc-owned elements) */
  int64_t nelem_ext;            /* elements evaluated on this device (owned + upper ghost layer) */
  double dx, dy, dz, wg;        /* src/init.c:137-140 */
  int64_t device_bytes;         /* device memory held by the context */
  int device;
  int storage;                  /* matrix as last assembled: 0 AIJ blocks, 1 SBAIJ upper blocks,
                                   2 AIJ-split (upper blocks + bf16 lower corrections),
                                   3 AIJ value-indexed (index bytes + dictionary) */
  int split_slots;              /* AIJ-split: correction slots stored per node (of 117) */
  int split_bits;               /* AIJ-split: bits per correction (16 = bf16, 32 = f32) */
  /* Gauss-point box of the constitutive callback: the elements this context evaluates, x
     fastest from element (ex0, ey0, ez0) (global element = lower-left node), nelem_ext =
     nex*ney*nez; Gauss point gpi = ie*8 + gp.  One rank: DMDAGetElements' own order.  Several
     ranks: the rank's PETSc elements plus the upper ghost layer (owner computes). */
  int64_t ex0, ey0, ez0, nex, ney, nez;
  int vi_values;                /* value-indexed AIJ: distinct matrix values */
  int vi_bits;                  /* value-indexed AIJ: 4 = a nibble per value into its slot's dictionary
                                   (every slot takes <= 16 values), 8 = a byte into one dictionary */
  int vi_blocks;                /* value-indexed AIJ, block mode: distinct 3x3 blocks (one index byte per
                                   block into a dictionary of them), 0 when values are indexed one by one */
  int spmv_tx, spmv_ty, spmv_kc; /* SpMV of the last assembled storage when it is a z-marching tile kernel:
                                   tile width (x nodes), height (y rows) and planes per z-chunk; 0 for the
                                   gathered (one-node-per-thread) kernels */
  int64_t vi_exc_nodes;         /* value-indexed AIJ, block mode: owned nodes whose 27 blocks are stored as
                                   plain values (a per-GP-tangent law: the nodes touching an element whose
                                   tangent differs from the law's reference tangent) */
  int64_t split_escapes;        /* AIJ-split with dense bf16 corrections: corrections not exact in bf16, kept as
                                   their bf16 hi plus an exact double residual (0 otherwise) */
  int64_t st_listed;            /* value-indexed AIJ through the default-stencil SpMV: owned nodes whose 27 blocks
                                   differ from the default (interior) stencil's, computed from their own index
                                   bytes or exception blocks; -1 when the SpMV does not take that path */
} mcx_info;

typedef struct {
  /* wall milliseconds of the last call of each phase (HIP events on the compute stream) */
  double strains_ms, homogenize_ms, residual_ms, jacobian_ms, solve_ms, update_ms;
  /* SpMV kernel inside the last mcx_solve: HIP event pairs around every 8th launch (at most
     512), their count and summed device time */
  int64_t spmv_launches;
  double spmv_ms_total;
  int64_t spmv_bytes_per_launch; /* algorithmic bytes of one SpMV (values + x once + y once) */
  /* algorithmic bytes of the CG vector kernels per iteration of the last solve, averaged over the
     iterations (VecAXPY(r) + PCApply_Jacobi + the two dots, VecAYPX(p), the deferred VecAXPY(x)
     amortised over the iterations that apply it): with spmv_bytes_per_launch the bytes of one
     whole CG iteration */
  int64_t cg_vec_bytes_per_iter;
} mcx_timing;

const char* mcx_last_error(void);
const char* mcx_version(void);
int mcx_abi_version(void); /* MCX_ABI_VERSION of the library's build */

void mcx_default_opts(mcx_opts* o);
/* parse the reference's command-line surface (PETSc options-DB names); unknown flags are
   warned about on stderr and ignored, like the reference's options DB */
int mcx_parse_args(mcx_opts* o, int argc, const char* const* argv);

/* rank 0 creates the communicator id, the host transports it to every rank (MPI_Bcast,
   torch.distributed, a file ...).  Only needed when nranks > 1. */
int mcx_comm_unique_id(void* id /* MCX_COMM_ID_BYTES */);

/* Host-only planning (no GPU needed): the DMDA decomposition a rank would get, and its
   forward-halo plan — neighbour ranks and, per neighbour, the natural node ids
   (i + j*NX + k*NX*NY) sent and received, in message order.  Pass NULL arrays to query
   counts (*nnbr <= 26; *nsend / *nrecv = total nodes). */
int mcx_plan(const mcx_opts* o, int rank, int nranks, mcx_info* info);
int mcx_plan_halo(const mcx_opts* o, int rank, int nranks, int* nnbr, int* nbr_rank, int64_t* send_cnt,
                  int64_t* recv_cnt, int64_t* send_nat, int64_t* recv_nat, int64_t* nsend, int64_t* nrecv);

/* comm_id: rank 0's mcx_comm_unique_id, required when nranks > 1; with nranks == 1 a non-NULL id
   makes a one-rank RCCL communicator, so the reductions take the multi-rank (RCCL) path */
int mcx_init(const mcx_opts* o, int rank, int nranks, const void* comm_id, void** ctx);
/* In-process transport: `nranks` contexts on one device, each driven by its own host thread,
   exchanging halos / partial sums by device copies (multi-rank path without RCCL; every
   collective entry point must then be called by all members). */
int mcx_local_group_create(int nranks, int device, void** group);
int mcx_local_group_destroy(void* group);
/* MPI_Barrier(PETSC_COMM_WORLD) of the in-process transport (host only).  Every crossing of the
   group's barrier — this one and those inside the collective entry points — is tagged with its
   collective: a member reaching a different collective than the others, or a member missing for
   MCX_COMM_TIMEOUT seconds (environment at group creation, default 300), fails the crossing with
   a non-zero code naming the ranks and collectives, and every later crossing of that group fails
   at once (instead of pairing unrelated collectives or hanging). */
int mcx_local_group_barrier(void* group, int rank);
int mcx_init_local(const mcx_opts* o, int rank, void* group, void** ctx);
int mcx_finalize(void* ctx);
int mcx_get_info(void* ctx, mcx_info* info);
/* *on = 1 when this context's last SpMV ran the default-stencil march with direct-to-LDS staging
   (option "vi_st_dma": -1 (default) / 1 where eligible, 0 off; same product bitwise), else 0.  A
   function of its own: mcx_info keeps its size (ABI revision 3). */
int mcx_get_st_dma(void* ctx, int* on);
/* the ranks that actually joined this context's communicator (MPI_Comm_size / MPI_Comm_rank of
   PETSC_COMM_WORLD): ncclCommCount, ncclCommUserRank and ncclCommCuDevice of the RCCL
   communicator; the group size and member rank of the in-process transport; 1, 0 and the
   context's device without a communicator.  Any pointer may be NULL. */
int mcx_comm_info(void* ctx, int* comm_ranks, int* comm_rank, int* device);

/* Gauss-point constitutive model (micropp_C_material_set(id,E,nu,Sy,Ka,type)).  id 1 has to equal
   id 0 except under -mat_law micro and micro_nl, where ids 0 and 1 are the micro cell's two phases
   (micro_nl uses all four parameters of each) */
int mcx_material_set(void* ctx, int id, double E, double nu, double Sy, double Ka, int type);

/* ---- the MicroPP Gauss-point callback boundary (-mat_law external) ----
 * The reference hands every Gauss point's strain to MicroPP's C wrapper and reads stress and
 * tangent back per Gauss point (src/assembly.c:59,92,149, src/main.c:62,83).  With -mat_law
 * external the device laws are replaced by one of:
 *  (1) host callbacks with the wrapper's call shapes (a real MicroPP links straight in:
 *      api.set_strain3 = micropp_C_set_strain3, ...).  mcx_homogenize then copies the strains to
 *      the host, calls set_strain3(gpi, strain) for every Gauss point (gpi = ie*8 + gp over
 *      mcx_info's Gauss-point box, ascending), homogenize() once, get_stress3(gpi, stress) and
 *      get_ctan3(gpi, ctan) for every Gauss point, and copies stress and tangent back.
 *      mcx_update_vars calls update_vars(); the non-linear statistics come from
 *      get_non_linear_gps / get_f_trial_max when given.
 *  (2) a device law: law->homogenize(law->user, &batch) runs on the context's stream with
 *      device pointers to strain, stress and tangent (the same contract as the built-in laws).
 *  (3) batched injection: mcx_set_gp_stress / mcx_set_gp_ctan copy caller-computed values
 *      (host, [ngp][6] / [ngp][36], gpi order) into the device arrays; mcx_get_gp_strain reads
 *      the strains of the same box.
 * Stress and tangent are Voigt (xx, yy, zz, xy, xz, yz; engineering shear), the tangent row
 * major (ctan[k*6+l], src/assembly.c:99).  Pass NULL to unregister. */
typedef struct {
  void (*set_strain3)(int gpi, double* strain);  /* micropp_C_set_strain3   src/assembly.c:59 */
  void (*homogenize)(void);                      /* micropp_C_homogenize    src/main.c:62 */
  void (*get_stress3)(int gpi, double* stress);  /* micropp_C_get_stress3   src/assembly.c:149 */
  void (*get_ctan3)(int gpi, double* ctan);      /* micropp_C_get_ctan3     src/assembly.c:92 */
  void (*update_vars)(void);                     /* micropp_C_update_vars   src/main.c:83 (may be NULL) */
  int (*get_non_linear_gps)(void);               /* src/util.c:71 (may be NULL) */
  double (*get_f_trial_max)(void);               /* src/util.c:96 (may be NULL) */
} mcx_micropp_api;

typedef struct {
  int64_t nelem;      /* elements of the Gauss-point box (mcx_info.nelem_ext) */
  int64_t ngp;        /* 8 * nelem */
  const double* eps;  /* device [6][8][nelem]: component k of GP gp of element e at k*ngp + gp*nelem + e */
  double* sig;        /* device, same layout */
  double* ctan;       /* device [36][8][nelem]: ctan[k*6+l] of GP gp of element e at (k*6+l)*ngp + gp*nelem + e */
  void* stream;       /* the context's HIP stream: launch on it, or finish before returning */
} mcx_gp_batch;

typedef struct {
  int (*homogenize)(void* user, const mcx_gp_batch* batch);            /* required; 0 = OK */
  int (*update_vars)(void* user);                                      /* may be NULL */
  int (*nonlinear_stats)(void* user, int64_t* n_nonlinear, double* f_trial_max); /* may be NULL */
  void* user;
} mcx_device_law;

int mcx_set_micropp(void* ctx, const mcx_micropp_api* api);
int mcx_set_device_law(void* ctx, const mcx_device_law* law);
int mcx_set_gp_stress(void* ctx, const double* host /* [ngp][6] */);
int mcx_set_gp_ctan(void* ctx, const double* host /* [ngp][36] */);
int mcx_get_gp_strain(void* ctx, double* host /* [ngp][6] */);
/* the tangents the last mcx_homogenize left, in mcx_get_gp_strain's index order (row major 6x6 per
   Gauss point); any law with a tangent per Gauss point (plastic, external, micro_nl) */
int mcx_get_gp_ctan(void* ctx, double* host /* [ngp][36] */);

/* ---- the micro-scale cell (-mat_law micro) ----
 * The unit cube with micro_n nodes per edge (2 <= micro_n <= 10; <= 20 with the option "micro_mem" 1,
 * <= 128 with the option "micro_solver" 1, both below), ne = micro_n - 1 Q1 hexahedra per
 * edge, 2x2x2 Gauss points, physical B.  Material 0 is micro_mat_1, material 1 micro_mat_2 (E, nu;
 * isotropic elastic, Sy and Ka unused).  Element (i, j, k), 0 <= i, j, k < ne, is of material 1 iff
 *   micro_type 0 (centred sphere, radius 0.5): (2i+1-ne)^2 + (2j+1-ne)^2 + (2k+1-ne)^2 < ne^2
 *   micro_type 1 (flat layer in y):            2j+1 < ne
 * in integer arithmetic.  For each Voigt component l the boundary nodes get u = E_l x (unit
 * strain; shear cases E_ab = E_ba = 1/2) and the interior solves K_ii u_i = -K_ib u_b by
 * Jacobi-preconditioned CG from zero until the preconditioned residual norm is at most
 * "micro_rtol" (mcx_set_option, default 1e-12) times its first value, or "micro_max_it"
 * iterations (default 10 x interior dofs) have run, which fails the calling entry.  Column l of C
 * is the volume average of the Gauss-point stresses; C_hom = (C + C^T) / 2.  It is computed on
 * the device at the first mcx_homogenize, mcx_assembly_jac or mcx_micro_get_ctan after mcx_init
 * and again after mcx_material_set or a micro_* option changed it; every context of a multi-rank
 * run computes its own, bit-identical copy.
 * "micro_mem" (mcx_set_option; -micro_mem lds|device through mcx_apply_args): 0 (default) keeps the
 * cell solvers' nodal vectors in LDS, which bounds micro_n by 10; 1 keeps them in a device-memory
 * workspace (six of 5 x 3 micro_n^3 doubles here; for -mat_law micro_nl min(2 x compute units,
 * local Gauss points) of 6 x 3 micro_n^3 doubles, whatever the number of solved points) and
 * accepts micro_n <= 20.  For micro_n <= 10 both give the same bits.  The option recomputes C_hom
 * and is refused while history slots of -mat_law micro_nl are in use.
 * "micro_solver" (mcx_set_option; -micro_solver cell|grid through mcx_apply_args): 0 (default) solves
 * each load case in one workgroup, with the limits above; 1 spreads every load case over the whole
 * device, one workgroup per tile of 8x8x8 nodes and one kernel launch per CG phase, and accepts
 * 2 <= micro_n <= 128 (-mat_law micro only: a -mat_law micro_nl context refuses it with code 2; on
 * other contexts it has no effect).  Its workspace, 6 x 5 x 3 micro_n^3 doubles plus a few partial
 * sums, is counted in device_bytes and freed when the option returns to 0; "micro_mem" is ignored.
 * The definition is the same; the dot products are summed in another order, so C_hom agrees with
 * solver 0's to the CG's tolerance, not bit for bit.  Two runs give the same bits.
 * "micro_grid_poll" (1 .. 4096, default 16): the CG iterations solver 1 enqueues between two host
 * reads of the load cases' done flags; a tuning knob, the results do not depend on it. */
/* C_hom (row major, C[k*6+l]) and, per load case, the CG iterations and the final relative
   preconditioned residual norm.  Any pointer may be NULL. */
int mcx_micro_get_ctan(void* ctx, double C[36], int its[6], double rnorm[6]);
/* the elements' materials (0 / 1), x fastest: phase[i + ne*(j + ne*k)]; *n in: capacity, out:
   count ne^3 (phase may be NULL to query the count) */
int mcx_micro_get_phase(void* ctx, unsigned char* phase, int64_t* n);

/* ---- the non-linear micro-scale cell (-mat_law micro_nl) ----
 * The cell above with both phases J2-plastic (E, nu, Sy, Ka of micro_mat_1 / micro_mat_2; small
 * strain, linear isotropic hardening: the law of -mat_law plastic at every micro Gauss point, 7
 * history doubles each).  A macro Gauss point with strain eps and committed history: boundary
 * nodes carry u = E x (E_ab = eps_ab / 2 for shears), the interior solves R_i(u) = 0 by Newton from
 * zero; every step is a Jacobi-CG on the consistent tangent stiffness ("micro_rtol",
 * "micro_max_it").  Newton stops at |D^-1 R_i| <= "micro_nl_rtol" (1e-10) times its first value
 * (D: the diagonal of K_T at the first iterate) and gives up after "micro_nl_max_it" (20)
 * iterations.  sigma is the volume average of the micro stresses, the tangent the consistent
 * homogenised one (six solves with the converged K_T frozen, symmetrised), f_trial the largest
 * micro trial function.  A point whose elastic micro field (the superposition of the six
 * unit-strain fields) yields nowhere, and which never did, takes the linear shortcut: sigma =
 * C_hom eps, tangent C_hom, the bits of -mat_law micro.  Any other point takes a slot of the history
 * pool for good; the pool is allocated at the first such point with "micro_nl_slots" slots (0 =
 * default: what fits 2 GiB, at most the local Gauss points).  mcx_homogenize fails when the pool
 * is too small or a cell does not converge; mcx_update_vars commits the histories.  micro_n = 2
 * has no interior unknown: the one-element average of micro_mat_1's (micro_type 1) J2 law.
 * "micro_nl_solver" (mcx_set_option; -micro_nl_solver cell|grid through mcx_apply_args): 0 (default)
 * solves every listed point with one workgroup (micro_n <= 10, <= 20 with "micro_mem" 1); 1 solves
 * C_hom and the listed points by launches over the whole device, one workgroup per tile of 8x8x8
 * nodes and one launch per phase, 2 <= micro_n <= 64.  The definition, the slots (224 B x 8
 * (micro_n - 1)^3 each), mcx_micro_nl_get_info and mcx_micro_nl_get_pool are the same; the results
 * agree with solver 0 to the Newton / CG tolerances, not bit for bit, and are a function of the
 * strain and the committed history alone.  "micro_mem" is ignored under solver 1;
 * "micro_grid_poll" sets the CG iterations enqueued between two host reads of the solves' states.
 * The value changes only while no history slot is in use; other laws accept it without effect.
 * "micro_nl_start" (-micro_nl_start zero|elastic, 0 | 1; default 0) and "micro_nl_ls" (-micro_nl_ls K,
 * an integer 0 .. 16; default 0) globalise the Newton loop of both solvers.  Start 1: after the first
 * state pass at the zero interior (D and the first norm are the same bits as under 0) the interior
 * takes the elastic predictor sum_l eps_l w_l (the six unit-strain fields, ascending l) and the
 * state is evaluated there; a point that meets the stop then ends with 0 Newton iterations.  K > 0:
 * after a step's CG the lengths 2^-j, j = 0 .. K, are tried in turn; trial j is accepted when
 * |D^-1 R_i| at u + 2^-j dx is smaller than at the last accepted iterate, trial K regardless.
 * Both may change at any time, leave micro_n = 2 as it is and are accepted without effect by other
 * laws; the defaults keep every bit.
 * "micro_nl_tangent" (-micro_nl_tangent seq|block, 0 | 1; default 0; another number fails with code 1,
 * another word with code 2): how solver 1 runs the six frozen-K_T solves of a solved point's tangent.
 * 0 runs them one after the other; 1 advances the six columns together, each a CG of its own (its own
 * vectors, sums, alpha / beta and stop) inside the launches of one CG iteration, which read a micro
 * Gauss point's tangent data once for all columns.  Every column keeps the sequential solve's
 * arithmetic and summation order, so sigma, the tangent, f_trial, the histories and the counts of
 * mcx_micro_nl_get_info are the same bits under both values.  A solve in flight then has 26 vectors
 * of 3 micro_n^3 doubles instead of 6 and five more sets of work stresses (5 x 6 x 8 (micro_n - 1)^3
 * doubles), which shrinks the batch of solves that share a launch above micro_n = 20; device_bytes
 * counts the workspace.  Solver 0 accepts the option without effect and keeps its sequential columns
 * (its LDS is full), as do other laws.  The value changes only while no history slot is in use.
 * "micro_nl_apply" (-micro_nl_apply split|fused, 0 | 1; default 0; another number fails with code 1,
 * another word with code 2): how solver 1 forms q = K_T p in a CG iteration (Newton's, the tangent
 * columns', the block's).  0 takes two launches: a Gauss-point pass writes six work stresses per micro
 * Gauss point into the slot, a node gather reads them back.  1 takes one: a workgroup marches the
 * element layers of its tile of 8x8x8 nodes with one layer of stresses on chip and never writes the
 * work stresses.  Every node's 64 terms are added in the same order, so q, p.q and with them every
 * result and count are the same bits under both values.  Neither the workspace nor the slots follow
 * the option: it may change at any time, also with history slots in use, and device_bytes is the
 * same.  Solver 0 and other laws accept it without effect.
 * "micro_nl_warm" (-micro_nl_warm off|on, 0 | 1; default 0; another number fails with code 1, another
 * word with code 2): 1 lets solver 1 start a slotted point from its slot's warm record, the interior
 * field u_w, the six tangent columns W_l and the strain eps_w of the slot's last converged solve.  The
 * first state pass stays at the zero interior (D and the first norm keep their bits, so both stops mean
 * what they mean under every other setting); then the interior takes u_w + sum_l (eps - eps_w)_l W_l
 * instead of what "micro_nl_start" says, and tangent column l starts from W_l and ends with no
 * iteration if that already meets micro_rtol.  A point without a valid record (the first solve of its
 * slot, or after a failed solve) follows "micro_nl_start" bit for bit.  The records live in one
 * allocation of 7 x 24 micro_n^3 + 64 bytes per slot, counted in device_bytes, which exists while the
 * option is 1 and a pool exists; it is allocated with every record invalid (also when the option is
 * switched on with slots in use or "micro_nl_slots" changes) and freed when the option returns to 0.
 * mcx_update_vars does not touch it.  The results depend on the strain, the committed history, the
 * options and the record's contents only.  The option may change at any time.  Solver 0 and other laws
 * accept it without effect. */
/* per Gauss point (mcx_get_gp_strain's order): path 0 = linear shortcut, 1 = solved; Newton
   iterations, CG iterations (Newton steps and tangent solves together) and the final relative
   Newton residual of the last mcx_homogenize.  Any pointer may be NULL. */
int mcx_micro_nl_get_info(void* ctx, int* path, int* newton_its, int* cg_its, double* rnorm);
/* slots in use, slots allocated (0 before the first non-linear point) and the bytes of one slot */
int mcx_micro_nl_get_pool(void* ctx, int64_t* slots_used, int64_t* slots_allocated, int64_t* bytes_per_slot);
/* per Gauss point (the same order), of the last mcx_homogenize: the rejected step-length trials
   ("micro_nl_ls") and the smallest accepted length.  A solved point that never backtracked: 0 and
   1.0; a point on the linear shortcut: 0 and 0.0.  Either pointer may be NULL. */
int mcx_micro_nl_get_steps(void* ctx, int* ls_rejects, double* min_step);
/* the option "micro_nl_tangent" and, per Gauss point (the same order; col_its[8 nelem][6]), the CG
   iterations of each of the six tangent columns of the last mcx_homogenize where solver 1 ran them
   as a block; 0 for every other point.  Either pointer may be NULL. */
int mcx_micro_nl_get_tangent(void* ctx, int* block, int* col_its);
/* the option "micro_nl_apply" and the launches of the fused kernel that the last mcx_homogenize
   enqueued: 0 under "micro_nl_apply" 0, under solver 0 and when no point was solved.  Either pointer
   may be NULL. */
int mcx_micro_nl_get_apply(void* ctx, int* fused, long long* launches);
/* the option "micro_nl_warm" and, per Gauss point (the same order; used[8 nelem]) of the last
   mcx_homogenize: 0 not solved (the linear shortcut, micro_n = 2), 1 solved without a valid warm
   record, 2 solved from its record.  Either pointer may be NULL. */
int mcx_micro_nl_get_warm(void* ctx, int* option, int* used);

double mcx_get_displacement(void* ctx, int time_s);
int mcx_zero_u(void* ctx);                 /* VecZeroEntries(u)  src/init.c:103 */
int mcx_apply_bc_u(void* ctx, double U);
int mcx_set_strains(void* ctx);
int mcx_homogenize(void* ctx);
int mcx_assembly_res(void* ctx, double* norm2);
int mcx_assembly_jac(void* ctx);
int mcx_solve(void* ctx, int* its, double* rnorm, int* reason);
int mcx_update_u(void* ctx);
/* micropp_C_update_vars (src/main.c:83): commit the Gauss-point history of the time step */
int mcx_update_vars(void* ctx);
/* get_non_linear_gps / get_f_trial_max (src/util.c:69-102) over this rank's PETSc-owned
   elements: GPs with f_trial > 0 in the last homogenize, and the max f_trial */
int mcx_get_nonlinear_stats(void* ctx, int64_t* n_nonlinear, double* f_trial_max);

/* get_non_linear_gps + get_f_trial_max (src/util.c:69-102, called at src/main.c:88,93):
 * collective.  n_local = this rank's count (its gauss_evolution.dat column), n_total = the sum
 * over ranks (MPI_Gather + sum), f_trial_max = the max over ranks (MPI_Reduce MAX). */
int mcx_reduce_nonlinear(void* ctx, int64_t* n_local, int64_t* n_total, double* f_trial_max);

/* calc_force (src/forces.c:25-166, called at src/main.c:91): reaction force of the load case
 * from the Gauss-point stresses of the last homogenize — BC_CIRCLE: sum over the top element
 * layer inside the load circle of (sum over 8 GPs of sigma_yy) * dx * dz; BC_BENDING: last x
 * layer, sigma_xy * dy * dz; per rank in the reference's loop order and element set, then
 * summed over ranks.  Collective; every rank receives the total. */
int mcx_calc_force(void* ctx, double* force);

/* write_pvtu (src/output.c:25-267, called at src/main.c:100-108 every -vtu_freq time steps):
 * "<prefix>.pvtu" (rank 0) + "<prefix>-subdo-<rank>.vtu" with the ghosted box points, the
 * rank's elements, the ghosted displacement and cell data (part, cost = 0: no micro solver,
 * non-linear GP count, wg-weighted GP sums of strain and stress).  Collective (u halo). */
int mcx_write_vtu(void* ctx, const char* file_prefix);

/* src/main.c:57-82 for one time step; returns Newton iterations done, per-iteration
   |RES|, KSP its and KSP rnorm in caller arrays of length >= newton_max_its (may be NULL) */
int mcx_time_step(void* ctx, int time_s, int* newton_its, double* res, int* ksp_its, double* ksp_rnorm);

/* ---- data access (owned rows, PETSc-local order, host buffers) ---- */
int mcx_get_u(void* ctx, double* host);      /* ndofs_local */
int mcx_set_u(void* ctx, const double* host);
int mcx_get_b(void* ctx, double* host);
int mcx_get_du(void* ctx, double* host);
/* strains / stresses of the PETSc-owned elements, [ie*8+gp][6] (micropp gp index) */
int mcx_get_strain(void* ctx, double* host);
int mcx_get_stress(void* ctx, double* host);
/* global PETSc DOF of every owned local DOF, and its natural (i + j*NX + k*NX*NY)*3+d index */
int mcx_owned_dofs(void* ctx, int64_t* petsc, int64_t* natural);
/* owned rows of A in AIJ form: rowptr (ndofs_local+1, local offsets), global column ids
   sorted ascending, values (any pointer may be NULL) */
int mcx_dump_csr(void* ctx, int64_t* rowptr, int64_t* colidx, double* vals);
/* sorted global PETSc ids of the owned Dirichlet DOFs; *n in: capacity, out: count */
int mcx_dump_dirichlet(void* ctx, int64_t* idx, int64_t* n);
/* y = A x on owned rows (collective when nranks > 1) */
int mcx_spmv(void* ctx, const double* x_host, double* y_host);
/* KSP residual history of the last solve (ksp_monitor); *n in: capacity, out: count.  The count is the
   number of norms that solve computed: the initial one and one per completed iteration, its + 1.  A solve
   that stops inside an iteration before its norm (MCX_KSP_DIVERGED_INDEFINITE_MAT, _INDEFINITE_PC, z . r
   == 0) returns its entries: the last one is the norm of iteration its - 1, which mcx_solve's rnorm
   repeats. */
int mcx_get_ksp_history(void* ctx, double* hist, int64_t* n);

int mcx_set_timing(void* ctx, int on);
int mcx_get_timing(void* ctx, mcx_timing* t);
int mcx_synchronize(void* ctx);
/* tuning knobs ("spmv_subl": lines per sub-slab of the SpMV sweep, 0 = whole XCD slab; "micro_rtol",
   "micro_max_it", "micro_mem", "micro_solver", "micro_grid_poll": the micro cell's CG, -mat_law micro; "micro_nl_rtol", "micro_nl_max_it", "micro_nl_slots", "micro_nl_solver", "micro_nl_start", "micro_nl_ls", "micro_nl_tangent", "micro_nl_apply", "micro_nl_warm":
   -mat_law micro_nl) and a
   device-only SpMV timer (iters launches on the current search direction, HIP events) */
int mcx_set_option(void* ctx, const char* name, double value);
/* the command-line flags that have no mcx_opts field, applied to a context through mcx_set_option:
   -micro_mem lds|device ("micro_mem" 0 | 1), -micro_solver cell|grid ("micro_solver" 0 | 1), -micro_nl_solver cell|grid ("micro_nl_solver" 0 | 1),
   -micro_nl_start zero|elastic ("micro_nl_start" 0 | 1), -micro_nl_ls K ("micro_nl_ls", an integer 0 .. 16),
   -micro_nl_tangent seq|block ("micro_nl_tangent" 0 | 1),
   -micro_nl_apply split|fused ("micro_nl_apply" 0 | 1),
   -micro_nl_warm off|on ("micro_nl_warm" 0 | 1),
   -micro_rtol, -micro_max_it, -micro_nl_rtol, -micro_nl_max_it, -micro_nl_slots (each with a
   number), -pc_type jacobi|mg ("pc_type" 0 | 1), -pc_mg_levels N, -mg_levels_ksp_max_it k
   ("pc_mg_smooth"), -pc_mg_dist 0|1 ("pc_mg_dist"; give it before -pc_type), -pc_mg_precision
   double|single ("pc_mg_precision" 0 | 1).  mcx_parse_args accepts these flags and checks -micro_mem's, -micro_solver's, -micro_nl_solver's, -micro_nl_start's, -micro_nl_ls's, -micro_nl_tangent's, -micro_nl_apply's, -micro_nl_warm's and -pc_mg_precision's word; call this after mcx_init with the same argv.  Other flags are skipped. */
int mcx_apply_args(void* ctx, int argc, const char* const* argv);
int mcx_time_spmv(void* ctx, int iters, double* avg_ms);

/* The macro CG's preconditioner (options of a context; one rank only unless "pc_mg_dist" is 1, below):
 * "pc_type" (-pc_type jacobi|mg) 0 (default) Jacobi, 1 a geometric multigrid V-cycle;
 * "pc_mg_levels" (-pc_mg_levels N) 0 automatic (coarsen until every axis has <= 5 nodes), else
 * 2 .. 16 levels, refused when the coarsest level would have more than 3072 dofs;
 * "pc_mg_smooth" (-mg_levels_ksp_max_it k) the Chebyshev degree of the pre- and the post-smoother,
 * 1 .. 8, default 2.  An axis of N > 2 nodes keeps its even nodes and, when N - 1 is odd, its last
 * node; the other nodes interpolate 1/2, 1/2; rows of the interpolation at Dirichlet dofs are zero,
 * the coarse operators are the Galerkin products P^T A P (27 stencil blocks per node), the
 * coarsest one is inverted densely.  The hierarchy is rebuilt, at the next solve, after every
 * assembly of the matrix.  With pc_type 1 the solve is PCG with the norm sqrt(r . M^-1 r), the same
 * reasons, tolerances and history as with Jacobi.  pc_type 0 frees the hierarchy. */
/* "pc_mg_dist" (-pc_mg_dist 0|1, default 0; other values fail with code 1): on a context with a
 * communicator (several ranks, or one rank with a communicator id; either transport) pc_type 1 is
 * refused with code 2 ("one rank only") unless pc_mg_dist is 1, set first.  With it the hierarchy is
 * the same operator M^-1 as on one rank, up to the summation order of the dot products, distributed
 * like the grid: coarse node I of an axis sits on fine node min(2 I, N - 1) and belongs to that node's
 * owner (the fine ranges are the DMDA's), every level's vectors live in the rank's box plus one ghost
 * layer, and the coarsest level is gathered by one all-reduce and solved on every rank.  Automatic
 * levels (pc_mg_levels 0) also stop before a level on which some rank would own no node on some
 * axis; a fixed pc_mg_levels that reaches such a level is refused with code 2, the message naming
 * the level, the axis and the rank.  Every rank decides this from the options alone, so all ranks
 * refuse alike.  Setting pc_mg_dist back to 0 while pc_type is 1 on such a context fails with code 2;
 * on a context without a communicator the option is accepted and changes nothing.  With it,
 * mcx_solve, mcx_pc_apply, mcx_pc_mg_info and mcx_pc_mg_dump_csr are collective (every rank calls
 * them in the same order), and every rank gets the same iteration count, norms and history.
 * Off by default: the RCCL transport's send/recv has not run between two GPUs yet. */
/* "pc_mg_precision" (-pc_mg_precision double|single; 0 double, the default, or 1 single; other values
 * fail with code 1, another word with code 2): with 1 every level >= 1 of the hierarchy, the coarsest
 * one included, keeps its operator (243 values per node) and its vectors in float, under pc_mg_dist
 * also the padded residual and the level's halo buffers.  Values are widened as they are loaded, every
 * expression and every sum is the double hierarchy's, in double, and the result is rounded once, on the
 * store; level 0 (the assembled matrix, its smoother), the transfers' fine side, the coarsest level's
 * dense inverse, every dot product and the PCG stay double.  Level 1's operator is the double
 * hierarchy's rounded to float entry by entry; mcx_pc_mg_dump_csr returns the stored values widened.
 * M^-1 stays deterministic (the same bits for the same input) and symmetric to float rounding, about
 * 1e-7 relative, which makes it a slightly variable preconditioner: the PCG took the double
 * hierarchy's iteration count on every grid measured, at -ksp_rtol 1e-8 and, on 17^3, at 1e-12
 * (DESIGN §17); a tolerance near the double rounding may cost a few iterations more.  Changing the
 * value frees a built hierarchy (device_bytes follows); the next use builds it again.  It combines
 * with pc_mg_levels, pc_mg_smooth, pc_mg_dist, every storage and every law.
 * mcx_pc_mg_get_precision: the option's value. */
int mcx_pc_mg_get_precision(void* ctx, int* single);
/* z = M^-1 r on the owned rows with the current preconditioner (owned rows in, owned rows out) */
int mcx_pc_apply(void* ctx, const double* r_host, double* z_host);
/* the hierarchy of pc_type 1 (nlevels 0 otherwise): node counts nxyz[16][3] from the fine level
   down, the estimates lmax[16] of the largest eigenvalue of D^-1 A per smoothed level (0 before a
   matrix is assembled, and for the coarsest level), the hierarchy's device bytes (pc_mg_dist: the
   global node counts, the same lmax on every rank, this rank's bytes) */
int mcx_pc_mg_info(void* ctx, int* nlevels, int64_t* nxyz, double* lmax, int64_t* bytes);
/* the operator of level >= 1 in the conventions of the fine level's CSR dump, coarse nodes in
   natural order (i + j*nx + k*nx*ny)*3+d, every in-grid stencil entry present: rowptr has
   3*nodes + 1 entries; with colidx and vals NULL only rowptr (and so the entry count) is written.
   pc_mg_dist: the rows are the rank's owned coarse nodes in the natural order of its box (x fastest,
   mcx_pc_mg_box), colidx is in the level's global natural numbering */
int mcx_pc_mg_dump_csr(void* ctx, int level, int64_t* rowptr, int64_t* colidx, double* vals);
/* Host-only (no GPU, no context): the box rank `rank` of the rank grid o->px x o->py x o->pz (all
   three given, rank = pi + px (pj + py pk)) owns on every level of the distributed hierarchy of the
   grid o->NX x NY x NZ with pc_mg_levels `levels` (0: automatic): *nlevels, and global start[16][3]
   and count[16][3] from the fine level down (0 beyond *nlevels; any pointer may be NULL).  Code 1:
   bad arguments; code 2: what "pc_type" 1 would refuse (a rank without a node, a coarsest level
   above 3072 dofs, no coarser level). */
int mcx_pc_mg_plan(const mcx_opts* o, int rank, int levels, int* nlevels, int64_t* start, int64_t* count);
/* the same for a live context and one level: global start[3] and count[3] of the box this rank owns
   (the whole level without pc_mg_dist or without a communicator) */
int mcx_pc_mg_box(void* ctx, int level, int64_t* start, int64_t* count);

#ifdef __cplusplus
}
#endif
#endif
