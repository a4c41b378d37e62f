"""-mat_law micro: the two-phase micro cell homogenised on the device.

The reference below restates the definition in numpy, independently of the kernel: the unit cube
of n^3 nodes / (n-1)^3 Q1 hexahedra (2x2x2 Gauss, physical B), phases by the integer rule, dense K,
boundary u = E x for the six unit strains, the interior solved directly (np.linalg.solve), the
volume average of the Gauss-point stresses, C_hom = (C + C^T) / 2.  It also returns kappa, the
condition number of the Jacobi-scaled interior stiffness, which sets the bar of the comparison:
    max|C_gpu - C_ref| <= 100 kappa micro_rtol max|C_ref|
(100 covers the step from the preconditioned-residual norm to the error norm and the 10:1
stiffness contrast).  Homogeneous cells (n = 2, the sphere at n = 3, equal materials) keep only
rounding: 1e-13 max|C|.
"""
import functools
import os
import subprocess
import threading

import numpy as np
import pytest

import macroc_amd as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MAT1, MAT2 = (1.0e7, 0.25), (1.0e8, 0.3)
RTOL = 1e-12  # micro_rtol's default
SIZES = (2, 3, 4, 5, 7, 10)
CASES = [(t, n) for t in (0, 1) for n in SIZES]
# phase-1 elements of every case (the issue's table)
COUNTS = {(0, 2): 1, (0, 3): 8, (0, 4): 19, (0, 5): 32, (0, 7): 136, (0, 10): 389,
          (1, 2): 0, (1, 3): 4, (1, 4): 9, (1, 5): 32, (1, 7): 108, (1, 10): 324}
HOMOGENEOUS = {(0, 2), (0, 3), (1, 2)}


def iso_C(E, nu):
    lam = E * nu / ((1. + nu) * (1. - 2. * nu))
    mu = E / (2. * (1. + nu))
    Cm = np.zeros((6, 6))
    Cm[:3, :3] = lam
    Cm[np.arange(3), np.arange(3)] += 2. * mu
    Cm[np.arange(3, 6), np.arange(3, 6)] = mu
    return Cm


def phase_rule(typ, n):
    """[k][j][i] material of element (i, j, k), exact integer arithmetic."""
    ne = n - 1
    k, j, i = np.meshgrid(np.arange(ne), np.arange(ne), np.arange(ne), indexing="ij")
    if typ == 0:
        return ((2 * i + 1 - ne) ** 2 + (2 * j + 1 - ne) ** 2 + (2 * k + 1 - ne) ** 2 < ne * ne).astype(np.uint8)
    return (2 * j + 1 < ne).astype(np.uint8)


def element_B(ne):
    """B[gp][6][24] (Voigt xx, yy, zz, xy, xz, yz; engineering shear) of the cube element of edge
    h = 1 / ne, local node a at offsets (a & 1, a >> 1 & 1, a >> 2), and det J."""
    h = 1.0 / ne
    g = 1.0 / np.sqrt(3.0)
    B = np.zeros((8, 6, 24))
    for gp in range(8):
        xi = [g if (gp >> q) & 1 else -g for q in range(3)]
        for a in range(8):
            sa = [1.0 if (a >> q) & 1 else -1.0 for q in range(3)]
            dN = [0.125 * sa[d] * np.prod([1.0 + sa[q] * xi[q] for q in range(3) if q != d]) * (2.0 / h)
                  for d in range(3)]
            B[gp, 0, 3 * a + 0] = dN[0]
            B[gp, 1, 3 * a + 1] = dN[1]
            B[gp, 2, 3 * a + 2] = dN[2]
            B[gp, 3, 3 * a + 0], B[gp, 3, 3 * a + 1] = dN[1], dN[0]
            B[gp, 4, 3 * a + 0], B[gp, 4, 3 * a + 2] = dN[2], dN[0]
            B[gp, 5, 3 * a + 1], B[gp, 5, 3 * a + 2] = dN[2], dN[1]
    return B, (h / 2.0) ** 3


@functools.lru_cache(maxsize=None)
def reference(typ, n, mat1=MAT1, mat2=MAT2):
    """(C_hom, kappa or None, phase map) by dense assembly and a direct interior solve."""
    ne, nn = n - 1, n ** 3
    ph = phase_rule(typ, n)
    B, detJ = element_B(ne)
    Cs = [iso_C(*mat1), iso_C(*mat2)]
    Ke = [sum(B[gp].T @ Cm @ B[gp] for gp in range(8)) * detJ for Cm in Cs]
    ek, ej, ei = np.meshgrid(np.arange(ne), np.arange(ne), np.arange(ne), indexing="ij")
    ei, ej, ek, phf = ei.ravel(), ej.ravel(), ek.ravel(), ph.ravel()
    conn = np.stack([(ei + (a & 1)) + n * ((ej + (a >> 1 & 1)) + n * (ek + (a >> 2))) for a in range(8)], axis=1)
    edof = (3 * conn[:, :, None] + np.arange(3)[None, None, :]).reshape(-1, 24)
    K = np.zeros((3 * nn, 3 * nn))
    for p in (0, 1):
        ed = edof[phf == p]
        np.add.at(K, (ed[:, :, None], ed[:, None, :]), Ke[p])
    idx = np.arange(nn)
    ci, cj, ck = idx % n, (idx // n) % n, idx // (n * n)
    X = np.stack([ci, cj, ck], axis=1) / ne
    bnd = (ci == 0) | (cj == 0) | (ck == 0) | (ci == ne) | (cj == ne) | (ck == ne)
    bd = np.repeat(bnd, 3)
    U = np.zeros((3 * nn, 6))
    for l in range(6):
        Eb = np.zeros((3, 3))
        if l < 3:
            Eb[l, l] = 1.0
        else:
            p, q = ((0, 1), (0, 2), (1, 2))[l - 3]
            Eb[p, q] = Eb[q, p] = 0.5
        U[:, l] = (X @ Eb.T).ravel()
    U[~bd] = 0.0
    kappa = None
    if (~bd).any():
        Kii = K[np.ix_(~bd, ~bd)]
        U[~bd] = np.linalg.solve(Kii, -K[np.ix_(~bd, bd)] @ U[bd])
        d = np.sqrt(np.diag(Kii))
        w = np.linalg.eigvalsh(Kii / np.outer(d, d))
        kappa = w[-1] / w[0]
    Cm = np.zeros((6, 6))
    ue = U[edof]  # [elements][24][6 load cases]
    for p in (0, 1):
        sel = phf == p
        for gp in range(8):
            Cm += np.einsum("kl,ela->ka", Cs[p] @ B[gp], ue[sel]) * detJ
    return 0.5 * (Cm + Cm.T), kappa, ph


def bar(typ, n):
    Cr, kappa, _ = reference(typ, n)
    if (typ, n) in HOMOGENEOUS:
        return 1e-13 * np.abs(Cr).max()
    return 100.0 * kappa * RTOL * np.abs(Cr).max()


def micro_argv(typ, n, grid=(4, 4, 4), extra=(), mat1=MAT1, mat2=MAT2):
    return ["-da_grid_x", grid[0], "-da_grid_y", grid[1], "-da_grid_z", grid[2], "-mat_law", "micro",
            "-micro_n", n, "-micro_type", typ, "-micro_mat_1", "%r,%r,1e4,1e7" % mat1,
            "-micro_mat_2", "%r,%r,1e4,1e7" % mat2, *extra]


@functools.lru_cache(maxsize=None)
def gpu_ctan(typ, n):
    with M.Macroc(micro_argv(typ, n)) as m:
        Cg, its, rn = m.micro_ctan()
        return Cg, tuple(its), tuple(rn), m.micro_phase()


@pytest.mark.parametrize("typ,n", CASES)
def test_phase_map(typ, n):
    ph = gpu_ctan(typ, n)[3]
    assert ph.shape == (n - 1,) * 3 and np.array_equal(ph, phase_rule(typ, n))
    assert int(ph.sum()) == COUNTS[(typ, n)]


@pytest.mark.parametrize("typ,n", CASES)
def test_chom_against_reference(typ, n):
    Cg, its, rn, _ = gpu_ctan(typ, n)
    Cr, kappa, _ = reference(typ, n)
    err = np.abs(Cg - Cr).max()
    print(f"type {typ} n {n}: kappa {kappa} err/max|C| {err / np.abs(Cr).max():.3e} bar/max|C| "
          f"{bar(typ, n) / np.abs(Cr).max():.3e} its {its} rnorm {max(rn):.3e}")
    assert err <= bar(typ, n)
    assert all(r <= RTOL for r in rn)
    if n == 2:  # no interior unknown: nothing to iterate on
        assert its == (0,) * 6 and rn == (0.0,) * 6
        assert np.abs(Cg - iso_C(*(MAT2 if typ == 0 else MAT1))).max() <= 1e-13 * np.abs(Cr).max()
    if (typ, n) == (0, 3):  # one interior node of a homogeneous cell
        assert max(its) <= 2
        assert np.abs(Cg - iso_C(*MAT2)).max() <= 1e-13 * np.abs(Cr).max()


def test_equal_materials_give_the_isotropic_tangent():
    with M.Macroc(micro_argv(0, 5, mat1=MAT2, mat2=MAT2)) as m:
        Cg, its, rn = m.micro_ctan()
    Ci = iso_C(*MAT2)
    assert np.abs(Cg - Ci).max() <= 1e-13 * np.abs(Ci).max()


@pytest.mark.parametrize("typ,n", CASES)
def test_structure(typ, n):
    Cg = gpu_ctan(typ, n)[0]
    b = bar(typ, n)
    assert np.array_equal(Cg, Cg.T)
    if typ == 0:
        assert abs(Cg[0, 0] - Cg[1, 1]) <= b and abs(Cg[0, 0] - Cg[2, 2]) <= b
        return
    assert abs(Cg[0, 0] - Cg[2, 2]) <= b
    f1 = COUNTS[(typ, n)] / float((n - 1) ** 3)
    C1, C2 = iso_C(*MAT1), iso_C(*MAT2)
    voigt = (1.0 - f1) * C1 + f1 * C2
    reuss = np.linalg.inv((1.0 - f1) * np.linalg.inv(C1) + f1 * np.linalg.inv(C2))
    if 0.0 < f1 < 1.0:
        assert Cg[1, 1] < Cg[0, 0]
    for q in range(6):
        assert reuss[q, q] * (1 - 1e-12) <= Cg[q, q] <= voigt[q, q] * (1 + 1e-12), (q, reuss[q, q], Cg[q, q], voigt[q, q])


def test_refusals_and_dirtiness():
    for flag, val, word in (("-micro_n", 11, "micro_n"), ("-micro_n", 1, "micro_n"), ("-micro_type", 2, "micro_type")):
        argv = micro_argv(0, 4) + [flag, val]  # the later flag wins
        with M.Macroc(argv) as m:
            for call in (m.micro_ctan, m.homogenize, m.assembly_jac):
                with pytest.raises(M.MacrocError, match=word):
                    call()
    with M.Macroc(micro_argv(0, 7)) as m:
        m.set_option("micro_max_it", 1)
        with pytest.raises(M.MacrocError, match="did not converge for load case 0"):
            m.micro_ctan()
        with pytest.raises(M.MacrocError, match="did not converge"):
            m.assembly_jac()
        m.set_option("micro_max_it", 0)
        C0 = m.micro_ctan()[0]
        assert np.abs(C0 - reference(0, 7)[0]).max() <= bar(0, 7)
        m.material_set(1, 2.0e8, 0.3)
        C1 = m.micro_ctan()[0]
        assert C1[0, 0] > 1.05 * C0[0, 0]
        m.set_option("micro_rtol", 1e-3)  # a micro_* option recomputes too: a looser solve, fewer iterations
        C2, its2, _ = m.micro_ctan()
        assert not np.array_equal(C2, C1) and np.abs(C2 - C1).max() <= 1e-2 * np.abs(C1).max()
    with M.Macroc(["-da_grid_x", 4, "-da_grid_y", 4, "-da_grid_z", 4, "-mat_law", "elastic"]) as m:
        m.material_set(1, 1.0e7, 0.25)  # equal: accepted
        with pytest.raises(M.MacrocError, match="two distinct materials need the MicroPP micro-structure"):
            m.material_set(1, 1.0e8, 0.3)
        with pytest.raises(M.MacrocError, match="without -mat_law micro"):
            m.micro_ctan()


def stress_of(eps, Cm):
    """sigma[:, k] = sum_l C[k, l] eps[:, l], l ascending, products and sums rounded one by one."""
    sig = np.zeros_like(eps)
    for k in range(6):
        s = np.zeros(len(eps))
        for l in range(6):
            s = s + Cm[k, l] * eps[:, l]
        sig[:, k] = s
    return sig


def newton_step(m, inject=None):
    for ts in (0, 1):
        m.apply_bc_on_u(m.get_displacement(ts))
    m.set_strains()
    m.homogenize()
    if inject is not None:
        eps = m.gp_strain()
        m.set_gp_stress(stress_of(eps, inject))
        m.set_gp_ctan(np.tile(inject.ravel(), (m.ngp, 1)))
    res = m.assembly_res()
    m.assembly_jac()
    _, _, v = m.dump_csr()
    its, rn, reason = m.solve_Ax()
    return dict(b=m.b(), v=v, du=m.du(), its=its, reason=reason, res=res, info=m.get_info(), force=None)


# The 7x6x5 grid on the reference's default 50 x 1 x 50 box has no node inside the load circle
# (radius 1 about the top face's centre), so its time step 1 is the zero-load step: the matrix is
# compared in full, b and du are zero on both sides.  The same grid on a 6 x 5 x 4 box (dx = 1)
# has four loaded nodes, which makes the b, du and KSP comparisons bite.
@pytest.mark.parametrize("box,loaded", [((), False), (("-lx", 6, "-ly", 5, "-lz", 4), True)], ids=["box50", "box6"])
def test_macro_one_rank_against_injected_tangent(box, loaded):
    """Context A (-mat_law micro, layer n = 4) against context B (-mat_law external fed sigma =
    C_hom eps and C_hom at every Gauss point): the matrix bit for bit (the one-element-matrix path
    keeps the table path's term order), b within 1e-13 |b| row by row (tighter than the row's
    1e-13 sum|C||eps| contributions, which bound |b| from above), du within 1e-10, KSP its +-1;
    then A again in sbaij and in plain AIJ blocks."""
    grid, base = (7, 6, 5), ["-bc_type", 1, "-ksp_rtol", repr(1e-12), *box]
    with M.Macroc(micro_argv(1, 4, grid, base)) as a:
        Ch = a.micro_ctan()[0]
        A = newton_step(a)
        a.update_vars()  # a no-op for the linear micro law
        assert a.nonlinear_stats() == (0, 0.0)
        print("storage micro layer n=4:", A["info"]["storage"], "vi_blocks", A["info"]["vi_blocks"])
    argv_b = ["-da_grid_x", grid[0], "-da_grid_y", grid[1], "-da_grid_z", grid[2], "-mat_law", "external", *base]
    with M.Macroc(argv_b) as b:
        Bx = newton_step(b, inject=Ch)
    assert A["reason"] == Bx["reason"] == (2 if loaded else 3)  # CONVERGED_RTOL; zero load: CONVERGED_ATOL at once
    assert (np.linalg.norm(Bx["b"]) > 0.0) == loaded and (np.linalg.norm(Bx["du"]) > 0.0) == loaded
    assert np.array_equal(A["v"], Bx["v"])
    print("max |b_A - b_B| / |b_B|:", np.max(np.abs(A["b"] - Bx["b"]) / np.maximum(np.abs(Bx["b"]), 1e-300)))
    assert np.all(np.abs(A["b"] - Bx["b"]) <= 1e-13 * np.abs(Bx["b"]))
    assert np.linalg.norm(A["du"] - Bx["du"]) <= 1e-10 * np.linalg.norm(Bx["du"])
    assert abs(A["its"] - Bx["its"]) <= 1
    for extra in (["-dm_mat_type", "sbaij"], ["-mat_aij_vi", 0, "-mat_aij_split", 0]):
        with M.Macroc(micro_argv(1, 4, grid, base + extra)) as a2:
            A2 = newton_step(a2)
        assert A2["reason"] == A["reason"]
        assert np.linalg.norm(A2["du"] - A["du"]) <= 1e-10 * np.linalg.norm(A["du"]), extra


def test_macro_two_ranks():
    grid, base = (10, 8, 8), ["-ksp_rtol", repr(1e-12)]

    def fn(m):
        out = newton_step(m)
        out["C"] = m.micro_ctan()[0]
        out["nat"] = m.owned_dofs()[1]
        out["force"] = m.calc_force()
        return out

    with M.Macroc(micro_argv(0, 5, grid, base)) as m1:
        one = fn(m1)
    assert one["reason"] == 2 and np.linalg.norm(one["du"]) > 0.0  # a loaded step
    g = M.LocalGroup(2)
    res, errors = [None, None], []

    def worker(r):
        try:
            m = M.Macroc(micro_argv(0, 5, grid, base), rank=r, nranks=2, group=g)
            try:
                res[r] = fn(m)
            finally:
                m.finish()
        except Exception as e:  # surfaced below
            errors.append((r, e))

    ts = [threading.Thread(target=worker, args=(r,), daemon=True) for r in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(120)
    assert not any(t.is_alive() for t in ts), f"group hung; errors={errors}"
    assert not errors, errors
    g.destroy()
    assert np.array_equal(res[0]["C"], res[1]["C"]) and np.array_equal(res[0]["C"], one["C"])
    du = np.zeros_like(one["du"])
    for r in res:
        du[r["nat"]] = r["du"]
    ref = np.zeros_like(du)
    ref[one["nat"]] = one["du"]
    assert np.linalg.norm(du - ref) <= 1e-10 * np.linalg.norm(ref)
    for r in res:
        assert abs(r["force"] - one["force"]) <= 1e-10 * abs(one["force"])
    assert one["force"] != 0.0


def test_defaults_are_the_isotropic_first_material(capfd):
    """The reference's defaults (micro_type 1, micro_n 2) are one element of micro_mat_1: the micro
    law is then the elastic law; and it does not print the elastic law's -micro_n warning."""
    grid = ["-da_grid_x", 6, "-da_grid_y", 5, "-da_grid_z", 4, "-ksp_rtol", repr(1e-12)]
    with M.Macroc(grid + ["-mat_law", "micro"]) as a:
        A = newton_step(a)
        Ch = a.micro_ctan()[0]
    with M.Macroc(grid + ["-mat_law", "elastic"]) as e:
        E = newton_step(e)
    assert np.abs(Ch - iso_C(*MAT1)).max() <= 1e-13 * np.abs(Ch).max()
    assert E["reason"] == A["reason"] == 2 and np.linalg.norm(E["du"]) > 0.0  # a loaded step
    assert np.linalg.norm(A["du"] - E["du"]) <= 1e-10 * np.linalg.norm(E["du"])
    capfd.readouterr()
    with M.Macroc(grid + ["-mat_law", "micro", "-micro_n", 4]) as a:
        a.micro_ctan()
    assert "has no effect" not in capfd.readouterr().err


def test_driver_runs_the_micro_law(tmp_path):
    """macroc_amd -mat_law micro needs no MicroPP build: it passes both materials and prints them
    and C_hom before the time loop."""
    exe = os.path.join(ROOT, "macroc_amd", "driver", "macroc_amd")
    out = subprocess.run([exe, "-da_grid_x", "6", "-da_grid_y", "5", "-da_grid_z", "4", "-mat_law", "micro",
                          "-micro_n", "4", "-micro_type", "0", "-micro_mat_2", "1e8,0.3,1e4,1e7"],
                         cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert "id 0 : E = 1.000000e+07\tnu = 2.500000e-01" in lines and "id 1 : E = 1.000000e+08\tnu = 3.000000e-01" in lines
    row = [float(v) for v in lines[lines.index("C_hom : ") + 1].split()]
    Cr = reference(0, 4)[0]
    assert np.abs(np.array(row) - Cr[0]).max() <= 1e-6 * np.abs(Cr).max()  # %e prints 7 digits
    assert "has no effect" not in out.stderr and "Elapsed time" in out.stdout
