"""-pc_type mg on decomposed grids (option pc_mg_dist): several contexts over the
in-process transport on one GPU against a one-rank context on the same grid with pc_type 1 — the
level sizes and boxes, the Galerkin operators assembled by box, the eigenvalue estimates, the
V-cycle, the PCG solve, the Newton loop, the early stop, the refusals, one rank, and the memory.

The tolerances are the project's bars for the same quantities (tests/test_gpu_pcmg.py: check_galerkin
1e-12, the cycle 1e-10, the solve 1e-6; tests/test_gpu_multirank.py: iterations +-1).  The hierarchy's
rule is restated here: an axis of N > 2 nodes keeps its even nodes and, when N - 1 is odd, its last
node; the other nodes take 1/2, 1/2 of their neighbours; P is the tensor product times I_3 with zero
rows at Dirichlet dofs."""
import threading

import numpy as np
import pytest
import scipy.sparse as sp

import macroc_amd as M

pytestmark = pytest.mark.gpu

CASES = {"A": ((17, 17, 17), (2, 1, 1)), "B": ((16, 16, 16), (2, 2, 2)), "C": ((24, 9, 13), (3, 1, 2))}
PLASTIC = ["-da_grid_x", 12, "-da_grid_y", 10, "-da_grid_z", 12, "-dt", 0.01, "-ksp_rtol", "1e-12", "-mat_law", "plastic"]


# ---------------------------------------------------------------- the rule, restated
def axis_coarse(N):
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


def prolongation(n, dirichlet):
    Pn = sp.kron(axis_P(n[2]), sp.kron(axis_P(n[1]), axis_P(n[0])))
    return sp.diags(np.where(dirichlet, 0.0, 1.0)) @ sp.kron(Pn, sp.identity(3)).tocsr()


def galerkin(A, P):
    """(P^T A P with a unit diagonal on its empty dofs, the mask of those dofs)"""
    Ac = (P.T @ A @ P).tocsr()
    empty = Ac.diagonal() == 0.0
    return (Ac + sp.diags(np.where(empty, 1.0, 0.0))).tocsr(), empty


def csr_of(t, n):
    rp, ci, v = t
    return sp.csr_matrix((v, ci, rp), shape=(len(rp) - 1, n))


# ---------------------------------------------------------------- contexts
def grid_argv(g, procs=None, *more):
    a = ["-da_grid_x", g[0], "-da_grid_y", g[1], "-da_grid_z", g[2], "-bc_type", "0", "-ksp_rtol", "1e-8", "-ksp_monitor"]
    if procs:
        a += ["-da_processors_x", procs[0], "-da_processors_y", procs[1], "-da_processors_z", procs[2]]
    return a + list(more)


def assemble(m, steps=(), replay=None):
    """replay: instead of running the time steps, the displacement each of them ended with (global,
    natural order): the history a time step commits is a function of its last displacement"""
    if replay is not None:
        nat = m.owned_dofs()[1]
        for u in replay:
            m.set_u(u[nat])
            m.set_strains()
            m.homogenize()
            m.update_vars()
    elif steps:
        for ts in steps:
            m.time_step(ts)
    else:
        m.apply_bc_on_u(m.get_displacement(0))
        m.apply_bc_on_u(m.get_displacement(1))
    m.set_strains()
    m.homogenize()
    m.assembly_res()
    m.assembly_jac()


def run_group(argv, nranks, fn, timeout=300):
    """fn(m) on every rank of an in-process group; ([result per rank], [(rank, error)])"""
    g = M.LocalGroup(nranks)
    results, errors = [None] * nranks, []

    def worker(r):
        try:
            m = M.Macroc(argv, rank=r, nranks=nranks, group=g)
            try:
                results[r] = fn(m)
            finally:
                m.finish()
        except Exception as e:  # surfaced by the caller
            errors.append((r, e))

    ts = [threading.Thread(target=worker, args=(r,), daemon=True) for r in range(nranks)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout)
    assert not any(t.is_alive() for t in ts), f"group hung; errors={errors}"
    g.destroy()
    return results, errors


def measure(m, rvec, steps=(), jacobi=True, fine=False, replay=None):
    """everything the tests compare, of a context (one rank of a group, or the one-rank reference):
    rvec is one global random vector in natural order"""
    o = {}
    assemble(m, steps, replay)
    o["petsc"], o["nat"] = m.owned_dofs()
    r = rvec[o["nat"]]
    if fine:
        o["fine"] = m.dump_csr()
    o["exc"] = m.get_info()["vi_exc_nodes"]
    if jacobi:
        o["its_j"] = m.solve_Ax()[0]
    o["bytes0"] = m.get_info()["device_bytes"]
    m.set_option("pc_mg_dist", 1)
    m.set_option("pc_type", 1)
    o["z"] = {}
    for k in (2, 3):
        m.set_option("pc_mg_smooth", k)
        o["z"][k] = m.pc_apply(r)
        assert np.array_equal(m.pc_apply(r), o["z"][k])  # the same bits again
    m.set_option("pc_mg_smooth", 2)
    o["info"] = m.pc_mg_info()
    o["bytes1"] = m.get_info()["device_bytes"]
    o["boxes"] = [m.pc_mg_box(l) for l in range(o["info"]["levels"])]
    o["ops"] = [m.pc_mg_dump_csr(l) for l in range(1, o["info"]["levels"])]
    o["solve"] = m.solve_Ax()
    o["du"], o["hist"], o["b"] = m.du(), m.ksp_history(), m.b()
    again = m.solve_Ax()
    assert again == o["solve"] and np.array_equal(m.du(), o["du"])  # a second solve: the same bits
    m.set_option("pc_type", 0)
    o["bytes2"] = m.get_info()["device_bytes"]
    o["levels_after"] = m.pc_mg_info()["levels"]
    return o


class Ref:
    """the one-rank context on the same grid with pc_type 1"""

    def __init__(self, grid, more=(), steps=()):
        n = 3 * int(np.prod(grid))
        self.rvec = np.random.default_rng(11).standard_normal(n)
        with M.Macroc(grid_argv(grid, None, *more) if not steps else list(more)) as m:
            self.us = []  # the displacement every time step ended with
            for ts in steps:
                m.time_step(ts)
                self.us.append(m.u())
            assemble(m, replay=[] if steps else None)
            self.A = csr_of(m.dump_csr(), n)
            self.dmask = np.zeros(n, dtype=bool)
            self.dmask[m.dump_dirichlet()] = True
            m.set_option("pc_type", 1)
            self.z = {}
            for k in (2, 3):
                m.set_option("pc_mg_smooth", k)
                self.z[k] = m.pc_apply(self.rvec)
            m.set_option("pc_mg_smooth", 2)
            self.info = m.pc_mg_info()
            self.sizes = [tuple(int(v) for v in s) for s in self.info["nxyz"]]
            self.ops = [csr_of(m.pc_mg_dump_csr(l), 3 * int(np.prod(self.sizes[l]))) for l in range(1, len(self.sizes))]
            self.solve = m.solve_Ax()
            self.du, self.b = m.du(), m.b()


def gathered(outs, key, n):
    v = np.zeros(n)
    for o in outs:
        v[o["nat"]] = o[key] if not isinstance(key, tuple) else o[key[0]][key[1]]
    return v


def assembled_by_box(outs, l, sizes):
    """the ranks' dumps of level l (>= 1), rows placed by their boxes into the level's global matrix"""
    N = sizes[l]
    n = 3 * int(np.prod(N))
    A = sp.csr_matrix((n, n))
    rows_seen = np.zeros(n, dtype=int)
    for o in outs:
        s, c = o["boxes"][l]
        k, j, i = np.meshgrid(np.arange(c[2]), np.arange(c[1]), np.arange(c[0]), indexing="ij")
        node = ((i + s[0]) + N[0] * ((j + s[1]) + N[1] * (k + s[2]))).ravel()
        rows = (3 * node[:, None] + np.arange(3)).ravel()
        rp, ci, v = o["ops"][l - 1]
        assert len(rp) == 3 * int(np.prod(c)) + 1  # 3 * owned + 1
        loc = csr_of((rp, ci, v), n).tocoo()
        A = A + sp.csr_matrix((loc.data, (rows[loc.row], loc.col)), shape=(n, n))
        rows_seen[rows] += 1
    assert np.all(rows_seen == 1)
    return A.tocsr()


class Case:
    pass


@pytest.fixture(scope="module", params=list(CASES))
def case(request):
    k = Case()
    k.grid, k.procs = CASES[request.param]
    k.name = request.param
    k.nr = int(np.prod(k.procs))
    k.n = 3 * int(np.prod(k.grid))
    k.ref = Ref(k.grid)
    k.outs, errors = run_group(grid_argv(k.grid, k.procs), k.nr, lambda m: measure(m, k.ref.rvec))
    assert not errors, errors
    return k


# ---------------------------------------------------------------- 1. levels and boxes
def test_levels_and_boxes(case):
    for r, o in enumerate(case.outs):
        assert o["info"]["levels"] == case.ref.info["levels"]
        assert np.array_equal(o["info"]["nxyz"], case.ref.info["nxyz"])
        start, count = M.pc_mg_plan(grid_argv(case.grid, case.procs), rank=r)
        assert len(start) == o["info"]["levels"]
        for l, (s, c) in enumerate(o["boxes"]):
            assert np.array_equal(s, start[l]) and np.array_equal(c, count[l]), (r, l)
        assert o["levels_after"] == 0


# ---------------------------------------------------------------- 2. operators
def check_operators(outs, ref):
    for l in range(1, len(ref.sizes)):
        got = assembled_by_box(outs, l, ref.sizes)
        e = abs(got - ref.ops[l - 1]).max() / abs(ref.ops[l - 1]).max()
        print(f"level {l}: max |A_c(ranks) - A_c(one rank)| / max |A_c| =", e)
        assert e <= 1e-12
        if l == 1:
            want, _ = galerkin(ref.A, prolongation(ref.sizes[0], ref.dmask))
            e = abs(got - want).max() / abs(want).max()
            print("level 1: max |A_c - P^T A P| / max |A_c| =", e)
            assert e <= 1e-12


def test_operators(case):
    check_operators(case.outs, case.ref)


def test_operators_sbaij():
    grid, procs = CASES["A"]
    ref = Ref(grid, more=("-dm_mat_type", "sbaij"))
    outs, errors = run_group(grid_argv(grid, procs, "-dm_mat_type", "sbaij"), 2,
                             lambda m: measure(m, ref.rvec, jacobi=False))
    assert not errors, errors
    check_operators(outs, ref)


def fine_by_rank(outs, n):
    """the ranks' fine matrix (PETSc numbering per rank) in the natural numbering"""
    nat_of_petsc = np.zeros(n, dtype=np.int64)
    for o in outs:
        nat_of_petsc[o["petsc"]] = o["nat"]
    A = sp.csr_matrix((n, n))
    for o in outs:
        loc = csr_of(o["fine"], n).tocoo()
        A = A + sp.csr_matrix((loc.data, (o["nat"][loc.row], nat_of_petsc[loc.col])), shape=(n, n))
    return A.tocsr()


@pytest.fixture(scope="module")
def plastic():
    """The state after time steps 0 and 1 of the plastic load (tests/test_gpu_pcmg.py's
    test_galerkin_plastic_with_exception_nodes) on one rank and over (2, 1, 2).

    The ranks are brought into that state, not into one of their own: they take the displacement the
    one-rank context ended each time step with and commit the history at it (what mcx_time_step's last
    homogenize and its update_vars do), and owner-computes then gives them the one-rank strains and
    history bit for bit.  Running the time steps on the ranks reaches another state: after a committed
    step every yielded Gauss point sits on its yield surface to rounding (f_trial_max 7.3e-12 here),
    so the tangent assembled again at the same strain takes the elastic or the plastic branch by the
    last bits of u, and the CG's dot products, summed in another order per decomposition, move those
    bits.  Measured that way: |u_ranks - u_1| / |u_1| = 4.8e-15, yet max |A_ranks - A_1| / max |A| =
    3.6e-2 on the fine level (4.6e-3 on level 1); on one rank alone, u perturbed by 1e-16 relative
    changes the fine matrix by 3.1e-2.  test_newton_plastic_matches_jacobi runs the ranks' own time steps."""
    k = Case()
    k.grid = (12, 10, 12)
    k.n = 3 * int(np.prod(k.grid))
    k.ref = Ref(k.grid, more=PLASTIC, steps=(0, 1))
    argv = PLASTIC + ["-da_processors_x", 2, "-da_processors_y", 1, "-da_processors_z", 2]
    k.outs, errors = run_group(argv, 4, lambda m: measure(m, k.ref.rvec, jacobi=False, fine=True, replay=k.ref.us))
    assert not errors, errors
    return k


def test_operators_plastic_with_exception_nodes(plastic):
    """a tangent per Gauss point, exception nodes in the value-indexed storage of some rank: every
    level of the ranks' hierarchy against scipy's P^T A P of the level above it, from the matrix the
    ranks hold"""
    outs, sizes = plastic.outs, plastic.ref.sizes
    assert any(o["exc"] > 0 for o in outs), [o["exc"] for o in outs]
    A, mask = fine_by_rank(outs, plastic.n), plastic.ref.dmask
    for l in range(1, len(sizes)):
        got = assembled_by_box(outs, l, sizes)
        want, mask = galerkin(A, prolongation(sizes[l - 1], mask))
        e = abs(got - want).max() / abs(want).max()
        print(f"level {l}: max |A_c - P^T A P| / max |A_c| =", e)
        assert e <= 1e-12
        A = got


def test_operators_plastic_equal_the_one_rank_dump(plastic):
    """the same state against the one-rank context: the fine matrix the ranks hold is the one-rank
    matrix, and every level of their hierarchy equals the one-rank dump (level 1 also scipy's P^T A P)"""
    assert any(o["exc"] > 0 for o in plastic.outs)
    dA = abs(fine_by_rank(plastic.outs, plastic.n) - plastic.ref.A).max() / abs(plastic.ref.A).max()
    print("fine level: max |A(ranks) - A(one rank)| / max |A| =", dA)
    assert dA == 0.0  # owner-computes: the same state gives the same matrix on any rank grid
    check_operators(plastic.outs, plastic.ref)


# ---------------------------------------------------------------- 3. eigenvalue estimates
def test_eigenvalue_estimates(case):
    l0 = case.outs[0]["info"]["lmax"]
    for o in case.outs:
        assert np.array_equal(o["info"]["lmax"], l0)  # the same bits on every rank
    print("lmax:", l0, " one rank:", case.ref.info["lmax"])
    assert np.all(abs(l0 - case.ref.info["lmax"]) <= 1e-12 * abs(case.ref.info["lmax"]))
    assert l0[-1] == 0.0


# ---------------------------------------------------------------- 4. the cycle
def test_cycle(case):
    free = ~case.ref.dmask
    for k in (2, 3):
        z, zref = gathered(case.outs, ("z", k), case.n), case.ref.z[k]
        err = np.linalg.norm(z - zref) / np.linalg.norm(zref)
        err_free = np.linalg.norm((z - zref)[free]) / np.linalg.norm(zref[free])
        print(f"{case.name} V({k},{k}): |z - z_1| / |z_1| =", err, " on the free dofs:", err_free)
        assert err <= 1e-10 and err_free <= 1e-10


# ---------------------------------------------------------------- 5. the solve
def test_solve(case):
    ref, outs = case.ref, case.outs
    its, rnorm, reason = outs[0]["solve"]
    for o in outs:  # iterations, rnorm and history identical on every rank
        assert o["solve"] == outs[0]["solve"] and np.array_equal(o["hist"], outs[0]["hist"])
    du, b = gathered(outs, "du", case.n), gathered(outs, "b", case.n)
    err = np.linalg.norm(du - ref.du) / np.linalg.norm(ref.du)
    res = np.linalg.norm(b - ref.A @ du) / np.linalg.norm(b)
    print(f"{case.name}: one-rank mg its {ref.solve[0]}, {case.nr}-rank mg its {its}, jacobi its {outs[0]['its_j']}, "
          f"|du - du_1|/|du_1| = {err:.3e}, |b - A du|/|b| = {res:.3e}")
    assert reason == 2 and ref.solve[2] == 2
    assert abs(its - ref.solve[0]) <= 1 and its < outs[0]["its_j"]
    assert err <= 1e-6 and res <= 1e-6
    assert len(outs[0]["hist"]) == its + 1 and outs[0]["hist"][-1] == rnorm


def test_solve_tight():
    """case B at -ksp_rtol 1e-12: the two hierarchies are the same operator"""
    grid, procs = CASES["B"]
    n = 3 * int(np.prod(grid))
    du = []
    for pr in (None, procs):
        argv = grid_argv(grid, pr, "-ksp_rtol", "1e-12")

        def fn(m):
            assemble(m)
            m.set_option("pc_mg_dist", 1)
            m.set_option("pc_type", 1)
            its, _, reason = m.solve_Ax()
            assert reason == 2
            return dict(nat=m.owned_dofs()[1], du=m.du(), its=its)

        if pr is None:
            with M.Macroc(argv) as m:
                outs = [fn(m)]
        else:
            outs, errors = run_group(argv, 8, fn)
            assert not errors, errors
        du.append(gathered(outs, "du", n))
    err = np.linalg.norm(du[1] - du[0]) / np.linalg.norm(du[0])
    print("rtol 1e-12: |du - du_1| / |du_1| =", err)
    assert err <= 1e-10


# ---------------------------------------------------------------- 6. Newton
def test_newton_plastic_matches_jacobi():
    """time steps 0 and 1 of the plastic law over (2, 1, 2): every assembly_jac rebuilds the hierarchy"""
    procs = ["-da_processors_x", 2, "-da_processors_y", 1, "-da_processors_z", 2]
    n = 3 * 12 * 10 * 12
    out = []
    for pc in (["-pc_type", "jacobi"], ["-pc_mg_dist", 1, "-pc_type", "mg"]):
        def fn(m):
            m.time_step(0)
            r = m.time_step(1)
            return dict(r=r, u=m.u(), nat=m.owned_dofs()[1])

        outs, errors = run_group(PLASTIC + procs + pc, 4, fn)
        assert not errors, errors
        assert all(o["r"] == outs[0]["r"] for o in outs)  # every rank saw the same Newton loop
        out.append((outs[0]["r"], gathered(outs, "u", n)))
    (rj, uj), (rm, um) = out
    print("jacobi:", rj, "\nmg:", rm)
    assert rj["newton_its"] == rm["newton_its"] >= 2
    np.testing.assert_allclose(rm["res"], rj["res"], rtol=1e-6)
    assert max(rm["ksp_its"]) < min(rj["ksp_its"])
    assert np.linalg.norm(um - uj) <= 1e-8 * np.linalg.norm(uj)


# ---------------------------------------------------------------- 7. the early stop
def test_early_stop():
    grid = (24, 9, 40)
    n = 3 * int(np.prod(grid))

    def fn(m):
        assemble(m)
        m.set_option("pc_mg_dist", 1)
        m.set_option("pc_type", 1)
        its, _, reason = m.solve_Ax()
        return dict(nat=m.owned_dofs()[1], du=m.du(), reason=reason, sizes=m.pc_mg_info()["nxyz"].tolist())

    with M.Macroc(grid_argv(grid)) as m:
        one = fn(m)
    outs, errors = run_group(grid_argv(grid, (3, 1, 1)), 3, fn)
    assert not errors, errors
    assert len(one["sizes"]) == 5
    for o in outs:
        assert o["sizes"] == [[24, 9, 40], [13, 5, 21], [7, 3, 11], [4, 2, 6]] and o["reason"] == 2
    du, du1 = gathered(outs, "du", n), gathered([one], "du", n)
    err = np.linalg.norm(du - du1) / np.linalg.norm(du1)
    print("4 levels over 3 ranks against 5 levels on one: |du - du_1| / |du_1| =", err)
    assert err <= 1e-6


# ---------------------------------------------------------------- 8. refusals
def refusals(argv, nranks, fn):
    """fn(m) -> a list of error strings (or 'accepted'); no rank may be left alive"""
    outs, errors = run_group(argv, nranks, fn, timeout=120)
    assert not errors, errors
    return outs


def attempt(m, name, value):
    try:
        m.set_option(name, value)
        return "accepted"
    except M.MacrocError as e:
        return str(e)


def test_fixed_levels_reaching_an_empty_rank_refuse():
    argv = grid_argv((12, 9, 9), (4, 1, 1))

    def fn(m):
        got = [attempt(m, "pc_mg_levels", 4)]  # before pc_mg_dist: nothing is known, pc_type 1 refuses it
        got.append(attempt(m, "pc_mg_dist", 1))
        got.append(attempt(m, "pc_type", 1))
        got.append(attempt(m, "pc_mg_levels", 0))
        got.append(attempt(m, "pc_mg_levels", 4))  # under pc_mg_dist: refused at once
        got.append(attempt(m, "pc_type", 1))
        return got

    for got in refusals(argv, 4, fn):
        assert got[0] == got[1] == got[3] == got[5] == "accepted", got
        for e in (got[2], got[4]):
            assert "failed (2)" in e and "level 3" in e and "rank 1" in e and "axis x" in e, got


def test_bad_values_refuse():
    def fn(m):
        got = [attempt(m, "pc_mg_dist", 2), attempt(m, "pc_mg_dist", 0.5), attempt(m, "pc_type", 1)]
        m.set_option("pc_mg_dist", 1)
        m.set_option("pc_type", 1)
        got.append(attempt(m, "pc_mg_dist", 0))
        m.set_option("pc_type", 0)
        got.append(attempt(m, "pc_mg_dist", 0))
        got.append(attempt(m, "pc_type", 1))
        return got

    for got in refusals(grid_argv((9, 9, 9), (2, 1, 1)), 2, fn):
        assert "failed (1)" in got[0] and "failed (1)" in got[1], got
        assert "failed (2)" in got[2] and "one rank only" in got[2] and "pc_mg_dist" in got[2], got
        assert "failed (2)" in got[3], got
        assert got[4] == "accepted" and "one rank only" in got[5], got


# ---------------------------------------------------------------- 9. one rank
def test_one_rank_keeps_its_bits():
    grid = (17, 17, 17)
    ref = Ref(grid)
    with M.Macroc(grid_argv(grid)) as m:
        o = measure(m, ref.rvec)
    assert o["solve"] == ref.solve and np.array_equal(o["du"], ref.du)
    for k in (2, 3):
        assert np.array_equal(o["z"][k], ref.z[k])
    assert np.array_equal(o["info"]["lmax"], ref.info["lmax"])


def test_one_rank_rccl_communicator():
    """a one-rank RCCL communicator: the distributed path (all-reduces through RCCL, no neighbour)"""
    grid = (17, 17, 17)
    ref = Ref(grid)
    with M.Macroc(grid_argv(grid), rank=0, nranks=1, comm_id=M.comm_unique_id()) as m:
        assert "one rank only" in attempt(m, "pc_type", 1)
        o = measure(m, ref.rvec)
    assert o["solve"][2] == 2 and abs(o["solve"][0] - ref.solve[0]) <= 1
    err = np.linalg.norm(o["du"] - ref.du) / np.linalg.norm(ref.du)
    zerr = np.linalg.norm(o["z"][2] - ref.z[2]) / np.linalg.norm(ref.z[2])
    print("one-rank communicator: |du - du_1| / |du_1| =", err, " |z - z_1| / |z_1| =", zerr)
    assert err <= 1e-12 and zerr <= 1e-12


# ---------------------------------------------------------------- 10. memory
def test_device_bytes_count_the_hierarchy(case):
    for o in case.outs:
        n1 = int(np.prod(o["boxes"][1][1]))  # the rank's box of level 1
        assert o["info"]["bytes"] >= 8 * 243 * n1
        assert o["bytes1"] == o["bytes0"] + o["info"]["bytes"]
        assert o["bytes2"] == o["bytes0"]
