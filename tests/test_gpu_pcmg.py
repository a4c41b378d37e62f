"""-pc_type mg on the GPU: the level sizes, the Galerkin operators against P^T A P built with scipy,
the V-cycle against a numpy restatement of the same cycle, the PCG solve against Jacobi's, the
Newton loop, the refusals and the memory accounting.

The hierarchy's rule (include/macroc_amd.h) is restated here independently: an axis of
N > 2 nodes keeps its even nodes and, when N - 1 is odd, its last node; the other nodes take 1/2,
1/2 of their two neighbours; P is the tensor product times I_3 with zero rows at Dirichlet dofs."""
import os
import re
import subprocess
import threading

import numpy as np
import pytest
import scipy.sparse as sp

import macroc_amd as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# grid -> (expected level sizes, bound on the PCG iterations: the prototype's count times 1.5)
GRIDS = {
    (17, 17, 17): ([(17, 17, 17), (9, 9, 9), (5, 5, 5)], 12),
    (16, 16, 16): ([(16, 16, 16), (9, 9, 9), (5, 5, 5)], 12),
    (24, 9, 13): ([(24, 9, 13), (13, 5, 7), (7, 3, 4), (4, 2, 3)], 12),
    (40, 3, 40): ([(40, 3, 40), (21, 2, 21), (11, 2, 11), (6, 2, 6), (4, 2, 4)], 57),
}


# ---------------------------------------------------------------- the rule, restated
def axis_coarse(N):
    """fine indices of the coarse nodes of an axis"""
    if N <= 2:
        return list(range(N))
    c = list(range(0, N, 2))
    if (N - 1) % 2:
        c.append(N - 1)
    return c


def axis_P(N):
    cn = axis_coarse(N)
    pos = {f: q for q, f in enumerate(cn)}
    P = sp.lil_matrix((N, len(cn)))
    for f in range(N):
        if f in pos:
            P[f, pos[f]] = 1.0
        else:
            P[f, pos[f - 1]] = 0.5
            P[f, pos[f + 1]] = 0.5
    return P.tocsr()


def level_sizes(n):
    out = [tuple(n)]
    while True:
        cur = out[-1]
        if len(out) >= 2 and max(cur) <= 5:
            break
        nxt = tuple(len(axis_coarse(N)) for N in cur)
        if nxt == cur:
            break
        out.append(nxt)
    return out


def prolongation(n, dirichlet):
    """P of the level with node counts n (x fastest) and the boolean Dirichlet mask of its dofs"""
    Pn = sp.kron(axis_P(n[2]), sp.kron(axis_P(n[1]), axis_P(n[0])))
    P = sp.kron(Pn, sp.identity(3)).tocsr()
    return sp.diags(np.where(dirichlet, 0.0, 1.0)) @ P


def galerkin(A, P):
    """(P^T A P with a unit diagonal on its empty dofs, the mask of those dofs)"""
    Ac = (P.T @ A @ P).tocsr()
    empty = Ac.diagonal() == 0.0
    return (Ac + sp.diags(np.where(empty, 1.0, 0.0))).tocsr(), empty


def csr_of(t, n):
    rp, ci, v = t
    return sp.csr_matrix((v, ci, rp), shape=(n, n))


# ---------------------------------------------------------------- contexts
def assembled(argv, steps=()):
    """a context at time step 1 after assembly_jac (or after the time steps given, then assembled)"""
    m = M.Macroc(argv)
    if steps:
        for ts in steps:
            m.time_step(ts)
    else:
        m.apply_bc_on_u(m.get_displacement(0))
        m.apply_bc_on_u(m.get_displacement(1))
    m.set_strains()
    m.homogenize()
    m.assembly_res()
    m.assembly_jac()
    return m


def grid_argv(g, *more):
    return ["-da_grid_x", g[0], "-da_grid_y", g[1], "-da_grid_z", g[2], "-bc_type", "0", "-ksp_rtol", "1e-8",
            "-ksp_monitor", *more]


def fine_matrix(m):
    petsc, nat = m.owned_dofs()
    assert np.array_equal(petsc, nat)  # one rank: PETSc order is the natural order
    A = csr_of(m.dump_csr(), m.n)
    dmask = np.zeros(m.n, dtype=bool)
    dmask[m.dump_dirichlet()] = True
    return A, dmask


def reference_hierarchy(m, A, dmask):
    """every level's operator and P from the rule alone (scipy), from the fine matrix down"""
    sizes = level_sizes((m.info["NX"], m.info["NY"], m.info["NZ"]))
    ops, Ps, mask = [A], [], dmask
    for l in range(len(sizes) - 1):
        P = prolongation(sizes[l], mask)
        Ac, mask = galerkin(ops[-1], P)
        ops.append(Ac)
        Ps.append(P)
    return sizes, ops, Ps


class Case:
    pass


@pytest.fixture(scope="module", params=list(GRIDS), ids=lambda g: "x".join(map(str, g)))
def case(request):
    k = Case()
    k.grid = request.param
    k.m = assembled(grid_argv(k.grid))
    k.m.set_option("pc_type", 1)
    k.A, k.dmask = fine_matrix(k.m)
    k.sizes, k.ops, k.Ps = reference_hierarchy(k.m, k.A, k.dmask)
    yield k
    k.m.finish()


# ---------------------------------------------------------------- 1. levels
def test_levels(case):
    info = case.m.pc_mg_info()
    want = GRIDS[case.grid][0]
    assert level_sizes(case.grid) == want  # the rule gives what the issue lists
    assert info["levels"] == len(want)
    assert [tuple(r) for r in info["nxyz"].tolist()] == want
    # D^-1 A has a unit diagonal, so its mean eigenvalue is 1 and its largest one at least that; a
    # row has at most 81 entries of size <= 1 after symmetric scaling (Gershgorin)
    assert np.all(info["lmax"][:-1] > 1.0) and np.all(info["lmax"][:-1] < 81.0), info["lmax"]
    assert info["lmax"][-1] == 0.0  # the coarsest level is solved, not smoothed
    assert info["bytes"] > 0


# ---------------------------------------------------------------- 2. Galerkin operators
def check_galerkin(m):
    A, dmask = fine_matrix(m)
    sizes = level_sizes((m.info["NX"], m.info["NY"], m.info["NZ"]))
    P1 = prolongation(sizes[0], dmask)
    ref1, mask1 = galerkin(A, P1)
    got1 = csr_of(m.pc_mg_dump_csr(1), 3 * int(np.prod(sizes[1])))
    e1 = abs(got1 - ref1).max() / abs(ref1).max()
    print("level 1: max |A_c - P^T A P| / max |A_c| =", e1)
    assert e1 <= 1e-12
    if len(sizes) > 2:  # level 2 from the dumped level 1
        P2 = prolongation(sizes[1], mask1)
        ref2, _ = galerkin(got1, P2)
        got2 = csr_of(m.pc_mg_dump_csr(2), 3 * int(np.prod(sizes[2])))
        e2 = abs(got2 - ref2).max() / abs(ref2).max()
        print("level 2: max |A_c - P^T A P| / max |A_c| =", e2)
        assert e2 <= 1e-12
    return got1


def test_galerkin_aij(case):
    got1 = check_galerkin(case.m)
    assert abs(got1 - got1.T).max() <= 1e-12 * abs(got1).max()


@pytest.mark.parametrize("g", list(GRIDS), ids=lambda g: "x".join(map(str, g)))
def test_galerkin_sbaij(g):
    m = assembled(grid_argv(g, "-dm_mat_type", "sbaij"))
    try:
        m.set_option("pc_type", 1)
        check_galerkin(m)
    finally:
        m.finish()


PLASTIC = ["-da_grid_x", 12, "-da_grid_y", 10, "-da_grid_z", 12, "-dt", 0.01, "-ksp_rtol", "1e-12", "-mat_law", "plastic"]


def test_galerkin_plastic_with_exception_nodes():
    """a tangent that differs per Gauss point: the state after time steps 0 and 1 of the non-linear
    tests' load has yielded points, so the value-indexed storage carries exception nodes"""
    m = assembled(PLASTIC, steps=(0, 1))
    try:
        assert m.nonlinear_stats()[0] > 0
        assert m.get_info()["vi_exc_nodes"] > 0
        m.set_option("pc_type", 1)
        check_galerkin(m)
    finally:
        m.finish()


# ---------------------------------------------------------------- 3. the operator M^-1
def test_operator_symmetric_positive(case):
    rng = np.random.default_rng(7)
    u, v = rng.standard_normal(case.m.n), rng.standard_normal(case.m.n)
    Mu, Mv = case.m.pc_apply(u), case.m.pc_apply(v)
    a, b = u @ Mv, v @ Mu
    print("u.Mv =", a, " v.Mu =", b, " rel =", abs(a - b) / abs(a))
    assert abs(a - b) <= 1e-12 * abs(a)
    assert u @ Mu > 0 and v @ Mv > 0
    assert np.array_equal(case.m.pc_apply(u), Mu)  # the same bits again
    # the Dirichlet rows (unit diagonal against a stiffness of 1e7) dominate those products: the
    # same on the free dofs alone, where only the cycle acts
    u[case.dmask] = 0.0
    v[case.dmask] = 0.0
    Mu, Mv = case.m.pc_apply(u), case.m.pc_apply(v)
    a, b = u @ Mv, v @ Mu
    print("free dofs: u.Mv =", a, " v.Mu =", b, " rel =", abs(a - b) / abs(a))
    assert abs(a - b) <= 1e-12 * abs(a)
    assert u @ Mu > 0 and v @ Mv > 0


def test_jacobi_pc_apply_is_the_inverse_diagonal(case):
    """under pc_type 0 the preconditioner is PCJacobi's: z = r * (1 / diag(A)), these bits"""
    m = assembled(grid_argv(case.grid))
    try:
        r = np.random.default_rng(3).standard_normal(m.n)
        assert np.array_equal(m.pc_apply(r), r * (1.0 / case.A.diagonal()))
    finally:
        m.finish()


# ---------------------------------------------------------------- 4. against a reference V-cycle
def chebyshev(A, dinv, lmax, b, x, k):
    """k steps of PETSc's Chebyshev recurrence on D^-1 A over [0.1, 1.1] lmax, from x (None: 0)"""
    emin, emax = 0.1 * lmax, 1.1 * lmax
    scale = 2.0 / (emax + emin)
    alpha = 1.0 - scale * emin
    mu, omegaprod = 1.0 / alpha, 2.0 / alpha
    ckm1, ck = 1.0, mu
    d = None
    for s in range(k):
        r = b if x is None else b - A @ x
        if s == 0:
            d = scale * (dinv * r)
        else:
            ckp1 = 2.0 * mu * ck - ckm1
            omega = omegaprod * ck / ckp1
            d = (omega - 1.0) * d + omega * scale * (dinv * r)
            ckm1, ck = ck, ckp1
        x = d.copy() if x is None else x + d
    return x


def vcycle(ops, Ps, lmax, l, b, k=2):
    if l == len(ops) - 1:
        return np.linalg.solve(ops[l].toarray(), b)
    A = ops[l]
    dinv = 1.0 / A.diagonal()
    x = chebyshev(A, dinv, lmax[l], b, None, k)
    xc = vcycle(ops, Ps, lmax, l + 1, Ps[l].T @ (b - A @ x), k)
    x = x + Ps[l] @ xc
    return chebyshev(A, dinv, lmax[l], b, x, k)


def test_cycle_matches_the_reference(case):
    m = case.m
    info = m.pc_mg_info()
    # the operators the device holds (dumped), the prolongations from the rule
    ops = [case.A] + [csr_of(m.pc_mg_dump_csr(l), 3 * int(np.prod(case.sizes[l]))) for l in range(1, info["levels"])]
    r = np.random.default_rng(11).standard_normal(m.n)
    for k in (2, 3):
        m.set_option("pc_mg_smooth", k)
        z, zref = m.pc_apply(r), vcycle(ops, case.Ps, info["lmax"], 0, r, k)
        err = np.linalg.norm(z - zref) / np.linalg.norm(zref)
        free = ~case.dmask  # without the Dirichlet rows, whose z = r dominates the norms
        err_free = np.linalg.norm((z - zref)[free]) / np.linalg.norm(zref[free])
        print(f"V({k},{k}): |z - z_ref| / |z_ref| =", err, " on the free dofs:", err_free)
        assert err <= 1e-10 and err_free <= 1e-10
    m.set_option("pc_mg_smooth", 2)


# ---------------------------------------------------------------- 5. the solve
def test_solve(case):
    m = case.m
    b = m.b()
    m.set_option("pc_type", 0)
    its_j, _, reason_j = m.solve_Ax()
    du_j = m.du()
    m.set_option("pc_type", 1)
    its, rnorm, reason = m.solve_Ax()
    du, hist = m.du(), m.ksp_history()
    err = np.linalg.norm(du - du_j) / np.linalg.norm(du_j)
    res = np.linalg.norm(b - case.A @ du) / np.linalg.norm(b)
    print(f"{case.grid}: jacobi its {its_j}, mg its {its}, |du_mg - du_j|/|du_j| = {err:.3e}, "
          f"|b - A du|/|b| = {res:.3e}, history {hist[0]:.3e} -> {hist[-1]:.3e}")
    assert reason_j == 2 and reason == 2
    assert err <= 1e-6
    assert res <= 1e-6
    assert len(hist) == its + 1 and hist[-1] == rnorm and hist[-1] < hist[0] * 1e-8
    assert its <= GRIDS[case.grid][1]
    assert its < its_j
    its2, rnorm2, _ = m.solve_Ax()
    assert (its2, rnorm2) == (its, rnorm) and np.array_equal(m.du(), du)


# ---------------------------------------------------------------- 6. Newton
def test_newton_plastic_matches_jacobi():
    """time steps 0 and 1 of the plastic law: every assembly_jac rebuilds the hierarchy"""
    out = []
    for pc in ("jacobi", "mg"):
        with M.Macroc(PLASTIC + ["-pc_type", pc]) as m:
            m.time_step(0)
            r = m.time_step(1)
            out.append((r, m.u()))
    (rj, uj), (rm, um) = out
    print("jacobi:", rj, "\nmg:", rm)
    assert rj["newton_its"] == rm["newton_its"] >= 2
    np.testing.assert_allclose(rm["res"], rj["res"], rtol=1e-6)
    assert max(rm["ksp_its"]) < min(rj["ksp_its"])
    assert np.linalg.norm(um - uj) <= 1e-8 * np.linalg.norm(uj)


# ---------------------------------------------------------------- 7. refusals and memory
def test_two_ranks_refuse():
    g = M.LocalGroup(2)
    got = [None, None]

    def worker(r):
        m = M.Macroc(["-da_grid_x", 9, "-da_grid_y", 9, "-da_grid_z", 9], rank=r, nranks=2, group=g)
        try:
            m.set_option("pc_type", 1)
            got[r] = "accepted"
        except M.MacrocError as e:
            got[r] = str(e)
        finally:
            m.finish()

    ts = [threading.Thread(target=worker, args=(r,), daemon=True) for r in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(120)
    assert not any(t.is_alive() for t in ts)
    g.destroy()
    for e in got:
        assert e is not None and "failed (2)" in e and "one rank only" in e, got


def test_levels_that_do_not_fit_refuse():
    with M.Macroc(["-da_grid_x", 33, "-da_grid_y", 33, "-da_grid_z", 33, "-bc_type", "0"]) as m:
        with pytest.raises(M.MacrocError, match=r"failed \(2\).*14739 dofs.*3072.* 3 levels fit"):
            m.set_option("pc_mg_levels", 2)
        m.set_option("pc_mg_levels", 3)
        for bad in (1, 17, 2.5):
            with pytest.raises(M.MacrocError, match=r"failed \(2\)"):
                m.set_option("pc_mg_levels", bad)
        for bad in (0, 9):
            with pytest.raises(M.MacrocError, match=r"failed \(2\)"):
                m.set_option("pc_mg_smooth", bad)
        with pytest.raises(M.MacrocError, match=r"failed \(2\)"):
            m.set_option("pc_type", 2)
    with pytest.raises(M.MacrocError, match=r"failed \(2\).* 3 levels fit"):
        M.Macroc(["-da_grid_x", 33, "-da_grid_y", 33, "-da_grid_z", 33, "-pc_type", "mg", "-pc_mg_levels", "2"])


def test_device_bytes_count_the_hierarchy():
    m = assembled(grid_argv((17, 17, 17)))
    try:
        before = m.get_info()["device_bytes"]
        assert m.pc_mg_info()["levels"] == 0
        m.set_option("pc_type", 1)
        m.pc_apply(np.ones(m.n))
        info = m.pc_mg_info()
        # level 1 and 2 operators, their five vectors and masks, the fine iterate and mask, the inverse
        n0, n1, n2 = 17 ** 3, 9 ** 3, 5 ** 3
        assert info["bytes"] >= 8 * (243 + 15) * (n1 + n2) + 8 * (3 * n2) ** 2 + 8 * 3 * 19 ** 3 + n0
        assert m.get_info()["device_bytes"] == before + info["bytes"]
        m.set_option("pc_type", 0)
        assert m.get_info()["device_bytes"] == before
        assert m.pc_mg_info()["levels"] == 0
    finally:
        m.finish()


def test_driver_takes_the_flag(tmp_path):
    exe = os.path.join(ROOT, "macroc_amd", "driver", "macroc_amd")
    argv = [exe, "-da_grid_x", "17", "-da_grid_y", "17", "-da_grid_z", "17", "-ts", "2", "-bc_type", "0",
            "-ksp_rtol", "1e-8"]
    its = []
    for more in ([], ["-pc_type", "mg", "-pc_mg_levels", "3", "-mg_levels_ksp_max_it", "2", "-pc_mg_galerkin"]):
        out = subprocess.run(argv + more, cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "not used" not in out.stderr and "Elapsed time" in out.stdout
        its.append([int(v) for v in re.findall(r"Its = (\d+)", out.stdout)])
    assert its[0] and len(its[0]) == len(its[1])
    assert all(a < b for a, b in zip(its[1], its[0])), its
    out = subprocess.run(argv + ["-pc_type", "lu"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "jacobi / mg" in out.stdout + out.stderr
