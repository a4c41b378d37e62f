"""Every stop reason of the device CG against the oracle, on every CG path.

The rows come from tests/ksp_stop_cases.py (proven on the CPU by tests/test_ksp_stops_cpu.py: the
reasons, the iteration counts and the margins that make the count independent of the summation
order of the dot products).  What follows a stop is what is checked: the VecAXPY(x) terms the p
update still owes (k_cg_xfinal / k_cg_xfinal_qb / k_cg_xwin, one fewer after INDEFINITE_MAT), the
reason gating every later launch of the chunk, the same stop on every rank, the history's length.

Every run: (its, reason) the oracle's exactly, rnorm to 1e-9 (NaN / Inf by kind), |du - du_oracle|
<= 1e-10 |du_oracle| (du == 0 for a stop at iteration 0), the history the oracle's to
1e-9 with as many entries as the solve computed norms.  Variants the suite already holds bitwise
equal for a -ksp_max_it stop are bitwise equal here.  Each context first solves the ordinary problem
(nu = 0.25), so a stale history entry is non-zero, and solves it again after the stopped solves with
every option restored: bitwise the first solve, so nothing of a stopped solve survives.
"""
import collections
import threading

import numpy as np
import pytest
import scipy.sparse as sp

import ksp_stop_cases as K
import macroc_amd as M
from oracle import oracle as O

pytestmark = pytest.mark.gpu

DU_BAR = 1e-10
Run = collections.namedtuple("Run", "label its rnorm reason du hist bytes_per_node")

# (cg_pdb, cg_par, cg_rev, cg_xs, cg_p2d) of test_gpu_parity.py:test_cg_pdb_bitwise
PDB_TUPLES = ((0, 0, 0, 0, 0), (1, 0, 0, 0, 0), (0, 1, 0, 0, 0), (1, 1, 0, 0, 0), (1, 1, 1, 0, 0),
              (1, 0, 1, 0, 0), (4, 0, 0, 0, 0), (4, 1, 0, 0, 0), (4, 1, 1, 0, 0), (4, 1, 0, 1, 0),
              (4, 0, 1, 1, 0), (4, 1, 0, 0, 1), (4, 2, 0, 0, 0), (4, 2, 1, 0, 0), (1, 2, 0, 0, 0))
# the library's defaults of every option a variant touches (mcx_internal.h)
DEFAULTS = dict(cg_fuse=1, cg_pdb=4, cg_par=1, cg_rev=1, cg_xs=0, cg_p2d=0, cg_dix=1, cg_fusep=0, halo_overlap=1)
DEFAULTS_STORAGE = dict(aij_vi=1, vi_stage=-1, vi_st=-1, vi_st_pair=0)


def argv_of(case, extra=()):
    NX, NY, NZ = K.GRIDS[case.grid]
    a = ["-da_grid_x", NX, "-da_grid_y", NY, "-da_grid_z", NZ, "-ksp_rtol", repr(K.RTOL), "-ksp_monitor"]
    kw = case.kw
    if "bc_type" in kw:
        a += ["-bc_type", kw["bc_type"]]
    if "abstol" in kw:
        a += ["-ksp_atol", repr(kw["abstol"])]
    if "dtol" in kw:
        a += ["-ksp_divtol", repr(kw["dtol"])]
    if "maxits" in kw:
        a += ["-ksp_max_it", kw["maxits"]]
    return a + list(extra)


def set_opts(m, opts):
    for k, v in opts.items():
        m.set_option(k, v)


def assemble(m, nu, poison=None, grid=None):
    """material, time step 0 then 1 (from u = 0), the assembled system; poison: one dof of u overwritten"""
    m.material_set(0, K.E, nu)
    m.zero_u()
    for ts in (0, 1):
        m.apply_bc_on_u(m.get_displacement(ts))
    if poison is not None:
        _, nat = m.owned_dofs()
        u = m.u()
        u[nat == K.poison_dof(grid)] = K.POISON[poison]  # the owner's row; no row on the other ranks
        m.set_u(u)
    m.set_strains()
    m.homogenize()
    m.assembly_res()
    m.assembly_jac()


def assemble_case(m, case):
    assemble(m, case.kw.get("nu", 0.25), case.poison, case.grid)


def solve(m, label):
    its, rn, reason = m.solve_Ax()
    return Run(label, its, rn, reason, m.du(), m.ksp_history(), m.timing()["cg_vec_bytes_per_iter"] // (m.n // 3))


def rel_err(du, ref):
    n = np.linalg.norm(ref)
    return float(np.linalg.norm(du - ref) / n) if n > 0 else float(np.abs(du).max())


def check_run(case, r, out, du_ref, du=None):
    """one solve against the oracle's (du: the gathered iterate of a decomposed run)"""
    du = r.du if du is None else du
    err = rel_err(du, du_ref)
    assert (r.its, r.reason) == (out["its"], out["reason"]) == (case.its, case.reason), (case.id, r.label, r.its, r.reason)
    assert K.same_rnorm(r.rnorm, out["rnorm"]), (case.id, r.label, r.rnorm, out["rnorm"])
    if case.its == 0:
        assert not du.any(), (case.id, r.label)
    else:
        assert np.linalg.norm(du_ref) > 0 and err <= DU_BAR, (case.id, r.label, err)
    assert len(r.hist) == K.norms_computed(case.its, case.reason), (case.id, r.label, len(r.hist))
    np.testing.assert_allclose(r.hist, out["history"], rtol=1e-9, err_msg=f"{case.id} {r.label}")
    return err


def check_bitwise(case, runs):
    for r in runs[1:]:
        assert (r.its, r.reason) == (runs[0].its, runs[0].reason), (case.id, r.label, runs[0].label)
        assert np.array_equal(r.du, runs[0].du, equal_nan=True), (case.id, r.label, runs[0].label)
        assert np.array_equal(r.hist, runs[0].hist, equal_nan=True), (case.id, r.label, runs[0].label)


def check_stale(case, first):
    """the ordinary solve wrote the history entry a too-long copy of the stopped solve's would return"""
    n = K.norms_computed(case.its, case.reason)
    if case.reason == K.REASONS["indef"]:
        assert len(first.hist) > n and first.hist[n] != 0.0, (case.id, len(first.hist))


def check_restored(case, first, again):
    assert (again.its, again.reason) == (first.its, first.reason), (case.id, again.its, first.its)
    assert np.array_equal(again.du, first.du) and np.array_equal(again.hist, first.hist), case.id
    assert np.array_equal(again.rnorm, first.rnorm), case.id


def report(case, errs, margin=None):
    print(f"KSPSTOP {case.id} reason {case.reason} its {case.its} runs {len(errs)} max|du-du_oracle|/|du_oracle| "
          f"{max(errs):.3e}" + (f" min|p.Ap|margin {margin:.3e}" if margin is not None else ""))


def oracle_of(case):
    P, out = K.oracle_case(case)
    margin = None
    if case.kind == "indef":
        c = K.restated(P)
        margin = min(c["pap_margin"][case.its - 2:case.its])
    return P, out, P.du(), margin


# ------------------------------------------------------------------ a. one rank, 8x8x8: every row
G8 = K.cases_for("g8")


@pytest.mark.parametrize("case", G8, ids=[c.id for c in G8])
def test_one_rank_small(case):
    """the fused scalar steps (the default: k_cg_update_fa / k_cg_pupdate_fb and their two CgState
    buffers) and the separate ones (cg_fuse 0) over the p-buffer variants, with the Jacobi scaling
    from the diagonal index (cg_dix 1) and from the dinv / z vectors (cg_dix 0)"""
    P, out, du_ref, margin = oracle_of(case)
    with M.Macroc(argv_of(case)) as m:
        assemble(m, 0.25)
        first = solve(m, "ordinary")
        assemble_case(m, case)
        assert np.array_equal(m.dump_csr()[2], P.A_values())
        fused, unfused = [], []
        for dix in (1, 0):
            set_opts(m, dict(DEFAULTS, cg_dix=dix))
            fused.append(solve(m, f"default dix{dix}"))
        for dix in (1, 0):
            for pdb, par, rev, xs, p2d in PDB_TUPLES:
                set_opts(m, dict(cg_fuse=0, cg_dix=dix, cg_pdb=pdb, cg_par=par, cg_rev=rev, cg_xs=xs, cg_p2d=p2d))
                unfused.append(solve(m, f"fuse0 dix{dix} pdb{pdb} par{par} rev{rev} xs{xs} p2d{p2d}"))
        set_opts(m, DEFAULTS)
        assemble(m, 0.25)
        again = solve(m, "ordinary again")
    P.close()
    check_stale(case, first)
    errs = [check_run(case, r, out, du_ref) for r in fused + unfused]
    check_bitwise(case, fused)    # cg_dix 0 / 1: test_gpu_multirank.py:test_cg_dix_bitwise
    check_bitwise(case, unfused)  # the tuples: test_gpu_parity.py:test_cg_pdb_bitwise
    # the paths ran: the fused small-grid path keeps one p buffer, cg_fuse 0 the double / quad buffers
    assert len({r.bytes_per_node for r in unfused if "dix1" in r.label}) > 1
    check_restored(case, first, again)
    report(case, errs, margin)


# ------------------------------------------------------------------ b. one rank, 70x20x12
G70 = ([K.indef_case("g70", nu) for nu in (1.5, 2.0, 3.0, -2.0)] + [K.dtol_case("g70", k) for k in K.DTOL_K["g70"]]
       + [K.atol_case("g70", k) for k in K.ATOL_K["g70"]])
STORAGES = {"vi": dict(aij_vi=1, vi_stage=0), "vi_staged": dict(aij_vi=1, vi_stage=1), "split": dict(aij_vi=0)}
FUSEP_BYTES = 73 + 48  # cg_vec_bytes_per_node with the p update inside the SpMV (kernels.hip)


@pytest.mark.parametrize("case", G70, ids=[c.id for c in G70])
def test_one_rank_storages(case):
    """cg_fuse 0 on a grid of several update blocks: the value-indexed storage gathered and staged
    (the z march) and the AIJ-split storage, each over the p-buffer variants; then the p update
    inside the SpMV (cg_fusep 0 / 1 / 0) on the staged storage, k_spmv_vibm's march (vi_st 0) and
    the default-stencil one (vi_st 1 + vi_st_pair 1)"""
    P, out, du_ref, margin = oracle_of(case)
    groups = []
    with M.Macroc(argv_of(case)) as m:
        assemble(m, 0.25)
        first = solve(m, "ordinary")
        assemble_case(m, case)
        assert np.array_equal(m.dump_csr()[2], P.A_values())
        m.set_option("cg_fuse", 0)
        for name, sopts in STORAGES.items():
            set_opts(m, sopts)
            m.assembly_jac()  # aij_vi takes effect at the assembly
            assert m.get_info()["storage"] == (2 if name == "split" else 3), name
            runs = []
            for pdb, par, rev, xs, p2d in PDB_TUPLES:
                set_opts(m, dict(cg_pdb=pdb, cg_par=par, cg_rev=rev, cg_xs=xs, cg_p2d=p2d))
                runs.append(solve(m, f"{name} pdb{pdb} par{par} rev{rev} xs{xs} p2d{p2d}"))
            groups.append(runs)
        set_opts(m, dict(DEFAULTS, cg_fuse=0, aij_vi=1, vi_stage=1))
        m.assembly_jac()
        for st in (0, 1):
            set_opts(m, dict(vi_st=st, vi_st_pair=st))
            runs = []
            for fusep in (0, 1, 0):
                m.set_option("cg_fusep", fusep)
                runs.append(solve(m, f"st{st} fusep{fusep}"))
            # the fused p update ran (and only when asked for)
            assert [r.bytes_per_node == FUSEP_BYTES for r in runs] == [False, True, False], (case.id, st)
            groups.append(runs)
        set_opts(m, dict(DEFAULTS, **DEFAULTS_STORAGE))
        assemble(m, 0.25)
        again = solve(m, "ordinary again")
    P.close()
    check_stale(case, first)
    errs = []
    for runs in groups:
        errs += [check_run(case, r, out, du_ref) for r in runs]
        check_bitwise(case, runs)
    check_restored(case, first, again)
    report(case, errs, margin)


@pytest.mark.parametrize("st", [0, 1])
@pytest.mark.parametrize("maxits", [None, 5, 6])
def test_fused_p_update_with_separate_scalar_steps(maxits, st):
    """cg_fusep takes effect only beside the separate scalar steps: at 70x20x12 (17 update blocks) the
    default folds them into the vector kernels and keeps one p buffer whatever cg_fusep says, so
    test_gpu_parity.py:test_cg_fused_p_update_bitwise compares that path with itself.  Its cases under
    cg_fuse 0, with the proof that the p update ran inside the SpMV: converged and stopped by
    -ksp_max_it after an odd and an even number of iterations, bitwise the separate kernels' solve."""
    NX, NY, NZ = K.GRIDS["g70"]
    argv = ["-da_grid_x", NX, "-da_grid_y", NY, "-da_grid_z", NZ, "-ksp_rtol", repr(K.RTOL), "-ksp_monitor"]
    with M.Macroc(argv + (["-ksp_max_it", maxits] if maxits else [])) as m:
        set_opts(m, dict(cg_fuse=0, vi_stage=1, vi_st=st, vi_st_pair=st))
        assemble(m, 0.25)
        runs = []
        for fusep in (0, 1, 0):
            m.set_option("cg_fusep", fusep)
            runs.append(solve(m, f"st{st} fusep{fusep}"))
    assert [r.bytes_per_node == FUSEP_BYTES for r in runs] == [False, True, False]
    for r in runs[1:]:
        assert (r.its, r.reason) == (runs[0].its, runs[0].reason)
        assert np.array_equal(r.du, runs[0].du) and np.array_equal(r.hist, runs[0].hist)
    assert (runs[0].its, runs[0].reason) == ((maxits, K.REASONS["its"]) if maxits else (runs[0].its, K.REASONS["rtol"]))
    assert len(runs[0].hist) == runs[0].its + 1 and np.linalg.norm(runs[0].du) > 0


# ------------------------------------------------------------------ c. decomposed grids, in-process transport
def run_group(argv, nranks, fn, timeout=120):
    """test_gpu_multirank.py:run_group: one host thread per rank; the join timeout is the hang check"""
    g = M.LocalGroup(nranks)
    results, errors = [None] * nranks, []

    def worker(r):
        try:
            m = M.Macroc(argv, rank=r, nranks=nranks, group=g)
            try:
                results[r] = fn(m)
            finally:
                m.finish()
        except Exception as e:  # surfaced below
            errors.append((r, e))

    ts = [threading.Thread(target=worker, args=(r,), daemon=True) for r in range(nranks)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout)
    assert not any(t.is_alive() for t in ts), f"group hung; errors={errors}"
    assert not errors, errors
    g.destroy()
    return results


DECOMP = {"g20": (2, 2, 1), "g12": (2, 2, 2)}
DECOMPOSED = [c for g in DECOMP for c in K.decomposed_cases(g)]
RANK_VARIANTS = [(pdb, ov) for pdb in (0, 1, 4) for ov in (0, 1)]


@pytest.mark.parametrize("case", DECOMPOSED, ids=[c.id for c in DECOMPOSED])
def test_decomposed(case):
    """20x12x10 over 2x2x1 and 12x10x14 over 2x2x2: every rank stops in the same iteration for the
    same reason (RED_STORE + all-reduce + k_cg_logic), none hangs, and the gathered iterate is the
    one-rank oracle's; cg_pdb 0 / 1 / 4 and halo_overlap 0 / 1 bitwise equal
    (test_gpu_multirank.py:test_cg_pdb_multirank_bitwise, test_halo_overlap_bitwise)"""
    px, py, pz = DECOMP[case.grid]
    nr = px * py * pz
    NX, NY, NZ = K.GRIDS[case.grid]
    P, out, du_ref, margin = oracle_of(case)  # one rank: the PETSc order is the natural order
    argv = argv_of(case, ["-da_processors_x", px, "-da_processors_y", py, "-da_processors_z", pz])

    def fn(m):
        petsc, nat = m.owned_dofs()
        assemble(m, 0.25)
        first = solve(m, "ordinary")
        assemble_case(m, case)
        csr = m.dump_csr()
        runs = []
        for pdb, ov in RANK_VARIANTS:
            set_opts(m, dict(cg_pdb=pdb, halo_overlap=ov))
            runs.append(solve(m, f"pdb{pdb} overlap{ov}"))
        set_opts(m, DEFAULTS)
        assemble(m, 0.25)
        return dict(petsc=petsc, nat=nat, csr=csr, first=first, runs=runs, again=solve(m, "ordinary again"))

    res = run_group(argv, nr, fn)
    # the assembled rows, bit for bit the one-rank matrix (columns back to the natural numbering)
    D = O.Problem(NX, NY, NZ, nranks=nr, m=px, n=py, p=pz)
    inv = np.empty(P.ndofs, dtype=np.int64)
    inv[D.dof_map()] = np.arange(P.ndofs)
    D.close()
    Aref = K.matrix(P)
    rows, cols, vals = [], [], []
    for o in res:
        rp, ci, v = o["csr"]
        rows.append(np.repeat(o["nat"], np.diff(rp)))
        cols.append(inv[ci])
        vals.append(v)
    A = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=Aref.shape)
    assert A.nnz == Aref.nnz and (A != Aref).nnz == 0
    P.close()
    errs = []
    for q in range(len(RANK_VARIANTS)):
        du = np.zeros(len(du_ref))
        for o in res:
            du[o["nat"]] = o["runs"][q].du
        for o in res:  # every rank the same scalars
            r, r0 = o["runs"][q], res[0]["runs"][q]
            assert (r.its, r.reason) == (r0.its, r0.reason) and np.array_equal(r.hist, r0.hist, equal_nan=True), r.label
            assert np.array_equal(r.rnorm, r0.rnorm, equal_nan=True), r.label
        errs.append(check_run(case, res[0]["runs"][q], out, du_ref, du))
    for o in res:
        check_stale(case, o["first"])
        check_bitwise(case, o["runs"])
        check_restored(case, o["first"], o["again"])
    report(case, errs, margin)


# ------------------------------------------------------------------ d. -pc_type mg, one rank, 17x17x17
MG_ARGV = ["-da_grid_x", 17, "-da_grid_y", 17, "-da_grid_z", 17, "-bc_type", 0, "-ksp_rtol", "1e-8", "-ksp_monitor",
           "-pc_type", "mg"]
MG_TOL = dict(rtol=1e-8, abstol=1e-50, dtol=1e4, maxits=10000)  # the library's defaults but rtol
MG_POISON = 3 * (8 + 17 * (8 + 17 * 8))


def mg_assemble(m, poison=False):
    m.zero_u()
    for ts in (0, 1):
        m.apply_bc_on_u(m.get_displacement(ts))
    if poison:
        u = m.u()
        u[MG_POISON] = float("nan")
        m.set_u(u)
    m.set_strains()
    m.homogenize()
    m.assembly_res()
    m.assembly_jac()


def mg_reference(m, **tol):
    """float64 numpy PCG in pcmg_solve's norm sqrt(r . z) on the dumped fine matrix, the device's
    V-cycle (m.pc_apply: a fixed linear operator, the same bits at every call) as preconditioner"""
    rp, ci, v = m.dump_csr()
    A = sp.csr_matrix((v, ci, rp), shape=(m.n, m.n))
    return K.cg_petsc(A, m.b(), pc=m.pc_apply, norm="natural", **dict(MG_TOL, **tol))


@pytest.fixture(scope="module")
def mg_history():
    """the reference's history of the problem without -ksp_atol: the thresholds sit between its entries"""
    with M.Macroc(MG_ARGV) as m:
        mg_assemble(m)
        h = mg_reference(m, maxits=4)["history"]
    assert len(h) == 5
    return h


def mg_check(m, ref):
    its, rn, reason = m.solve_Ax()
    du, hist = m.du(), m.ksp_history()
    assert (its, reason) == (ref["its"], ref["reason"])
    # both sides apply the same cycle and differ by the summation order of two dot products per
    # iteration over at most 3 iterations: rtol's order, as for du
    assert K.same_rnorm(rn, ref["rnorm"], 1e-8)
    assert len(hist) == K.norms_computed(its, reason) == len(ref["history"])
    np.testing.assert_allclose(hist, ref["history"], rtol=1e-8)
    err = rel_err(du, ref["x"])
    if its == 0:
        assert not du.any()
    else:
        assert err <= 1e-8
    its2, rn2, reason2 = m.solve_Ax()  # and the solve repeats itself
    assert (its2, reason2) == (its, reason) and np.array_equal(m.du(), du) and np.array_equal(rn2, rn, equal_nan=True)
    print(f"KSPSTOP mg reason {reason} its {its} max|du-du_ref|/|du_ref| {err:.3e}")
    return its, reason


@pytest.mark.parametrize("k", [1, 2, 3])
def test_mg_atol(mg_history, k):
    h = mg_history
    assert h[k - 1] / h[k] >= K.GAP and np.all(h[:k] > np.sqrt(h[k - 1] * h[k]))
    with M.Macroc(MG_ARGV + ["-ksp_atol", repr(float(np.sqrt(h[k - 1] * h[k])))]) as m:
        mg_assemble(m)
        ref = mg_reference(m, abstol=float(np.sqrt(h[k - 1] * h[k])))
        assert (ref["its"], ref["reason"]) == (k, K.REASONS["atol"])
        assert mg_check(m, ref) == (k, K.REASONS["atol"])


def test_mg_dtol_at_iteration_0():
    with M.Macroc(MG_ARGV + ["-ksp_divtol", "1.0"]) as m:
        mg_assemble(m)
        assert mg_check(m, mg_reference(m, dtol=1.0)) == (0, K.REASONS["dtol"])


def test_mg_nan():
    with M.Macroc(MG_ARGV) as m:
        mg_assemble(m)
        its0, _, reason0 = m.solve_Ax()
        du0 = m.du()
        assert reason0 == K.REASONS["rtol"] and its0 > 3
        mg_assemble(m, poison=True)
        assert mg_check(m, mg_reference(m)) == (0, K.REASONS["nan"])
        mg_assemble(m)  # and nothing of it survives
        its, _, reason = m.solve_Ax()
        assert (its, reason) == (its0, reason0) and np.array_equal(m.du(), du0)
