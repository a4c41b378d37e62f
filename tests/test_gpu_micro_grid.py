"""Option micro_solver 1 (-micro_solver grid): the six unit-strain solves of -mat_law micro spread
over the device, one workgroup per 8x8x8-node tile of a load case and one launch per CG phase, for
2 <= micro_n <= 128.

The solver sums its dot products in another order than k_micro_rve, so its iterates differ from
the default solver's in the last bits; the project's bar judges (test_gpu_micro.py):
    max|C_gpu - C_ref| <= 100 kappa micro_rtol max|C_ref|
against the dense numpy reference up to n = 12, against the default solver at n = 20, and above
that against what is known in closed form: the homogeneous cell's isotropic tensor, the Reuss and
Voigt bounds, the cubic symmetry of the sphere cell (whose three axes are separate load cases) and
the integer phase rule.  kappa above n = 12 is the dense reference's at n = 12 scaled by
((n - 1) / 11)^2, the growth of the Jacobi-scaled stiffness' condition number with 1 / h^2.

Measured on an MI355X (DESIGN §14 has the table): errors of 2.5e-17 .. 5.0e-13 of max|C| against
bars of 1e-13 (n = 2) and 1e-10 .. 2.2e-7.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import macroc_amd as M
import test_gpu_micro as TM
import test_gpu_micro_nl as TN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REF_CELLS = [(t, n) for t in (0, 1) for n in (2, 3, 4, 5, 7, 8, 9, 10, 11, 12)]
BIG = (21, 33, 64)


@functools.lru_cache(maxsize=None)
def grid_ctan(typ, n, poll=None, mat1=TM.MAT1, mat2=TM.MAT2):
    with M.Macroc(TM.micro_argv(typ, n, mat1=mat1, mat2=mat2)) as m:
        m.set_option("micro_solver", 1)
        if poll is not None:
            m.set_option("micro_grid_poll", poll)
        Cg, its, rn = m.micro_ctan()
        return Cg, tuple(its), tuple(rn), m.micro_phase()


def scaled_kappa(typ, n, mats=(TM.MAT1, TM.MAT2)):
    return TM.reference(typ, 12, *mats)[1] * ((n - 1) / 11.0) ** 2


def check_bounds(Cg, ph, n):
    f1 = float(ph.sum()) / (n - 1) ** 3
    C1, C2 = TM.iso_C(*TM.MAT1), TM.iso_C(*TM.MAT2)
    voigt = (1.0 - f1) * C1 + f1 * C2
    reuss = np.linalg.inv((1.0 - f1) * np.linalg.inv(C1) + f1 * np.linalg.inv(C2))
    for q in range(6):
        assert reuss[q, q] * (1 - 1e-12) <= Cg[q, q] <= voigt[q, q] * (1 + 1e-12), (q, reuss[q, q], Cg[q, q], voigt[q, q])


# ---------------------------------------------------------------- 1. against the dense reference
@pytest.mark.parametrize("typ,n", REF_CELLS)
def test_against_the_dense_reference(typ, n):
    Cg, its, rn, ph = grid_ctan(typ, n)
    Cr, kappa, phr = TM.reference(typ, n)
    cmax = np.abs(Cr).max()
    bar = 1e-13 * cmax if kappa is None else 100.0 * kappa * TM.RTOL * cmax
    err = np.abs(Cg - Cr).max()
    print(f"type {typ} n {n}: kappa {kappa} err/max|C| {err / cmax:.3e} bar/max|C| {bar / cmax:.3e} its {its} "
          f"rnorm {max(rn):.3e}")
    assert err <= bar
    assert all(r <= TM.RTOL for r in rn)
    assert np.array_equal(Cg, Cg.T)
    assert ph.shape == (n - 1,) * 3 and np.array_equal(ph, TM.phase_rule(typ, n)) and np.array_equal(ph, phr)
    if n == 2:
        assert its == (0,) * 6
    else:
        assert min(its) >= 1


# ---------------------------------------------------------------- 2. against the default solver at n = 20
def test_against_the_default_solver_at_its_limit():
    Cg, its_g, rn_g, _ = grid_ctan(0, 20)
    with M.Macroc(TM.micro_argv(0, 20)) as m:
        m.set_option("micro_mem", 1)
        Cd, its_d, rn_d = m.micro_ctan()
    kappa = scaled_kappa(0, 20)
    cmax = np.abs(Cd).max()
    bar = 2 * 100.0 * kappa * TM.RTOL * cmax
    err = np.abs(Cg - Cd).max()
    print(f"n 20 sphere: its grid {its_g} / default {tuple(its_d)}, kappa {kappa:.1f} |C_grid - C_dev|/max|C| "
          f"{err / cmax:.3e} bar {bar / cmax:.3e}")
    assert err <= bar
    assert all(r <= TM.RTOL for r in rn_g) and all(r <= TM.RTOL for r in rn_d)
    assert np.array_equal(Cg, Cg.T)


# ---------------------------------------------------------------- 3. above n = 20
@pytest.mark.parametrize("n", BIG)
def test_homogeneous_cell_is_isotropic(n):
    kappa = scaled_kappa(0, n, (TM.MAT2, TM.MAT2))
    Cg, its, rn, _ = grid_ctan(0, n, None, TM.MAT2, TM.MAT2)
    Ci = TM.iso_C(*TM.MAT2)
    err = np.abs(Cg - Ci).max() / np.abs(Ci).max()
    print(f"n {n} homogeneous: its {its} rnorm {max(rn):.3e} kappa {kappa:.1f} err/max|C| {err:.3e} bar "
          f"{100 * kappa * TM.RTOL:.3e}")
    assert err <= 100.0 * kappa * TM.RTOL
    assert all(r <= TM.RTOL for r in rn) and min(its) >= 1
    assert np.array_equal(Cg, Cg.T)


@pytest.mark.parametrize("n", BIG)
def test_sphere_cell_structure(n):
    Cg, its, rn, ph = grid_ctan(0, n)
    kappa = scaled_kappa(0, n)
    bar = 100.0 * kappa * TM.RTOL * np.abs(Cg).max()
    groups = ((Cg[0, 0], Cg[1, 1], Cg[2, 2]), (Cg[0, 1], Cg[0, 2], Cg[1, 2]), (Cg[3, 3], Cg[4, 4], Cg[5, 5]))
    spread = max(max(g) - min(g) for g in groups)
    print(f"n {n} sphere: its {its} rnorm {max(rn):.3e} kappa {kappa:.1f} C00 {Cg[0, 0]:.9e} C01 {Cg[0, 1]:.9e} C33 "
          f"{Cg[3, 3]:.9e} cubic spread/max|C| {spread / np.abs(Cg).max():.3e} bar {100 * kappa * TM.RTOL:.3e}")
    assert all(r <= TM.RTOL for r in rn) and min(its) >= 1
    assert np.array_equal(Cg, Cg.T)
    assert ph.shape == (n - 1,) * 3 and np.array_equal(ph, TM.phase_rule(0, n))
    check_bounds(Cg, ph, n)
    assert spread <= bar  # C00 = C11 = C22, C01 = C02 = C12, C33 = C44 = C55: no axis is mixed up in the tiling


def test_layer_cell_structure():
    n = 24
    Cg, its, rn, ph = grid_ctan(1, n)
    bar = 100.0 * scaled_kappa(1, n) * TM.RTOL * np.abs(Cg).max()
    print(f"n {n} layer: its {its} rnorm {max(rn):.3e} C00 {Cg[0, 0]:.9e} C11 {Cg[1, 1]:.9e} C22 {Cg[2, 2]:.9e}")
    assert all(r <= TM.RTOL for r in rn)
    assert np.array_equal(Cg, Cg.T)
    assert np.array_equal(ph, TM.phase_rule(1, n))
    check_bounds(Cg, ph, n)
    assert abs(Cg[0, 0] - Cg[2, 2]) <= bar
    assert Cg[0, 0] - Cg[1, 1] > 1e3 * bar  # the layers are stacked in y


# ---------------------------------------------------------------- 4. determinism and gating
def test_bits_do_not_depend_on_the_poll_interval():
    base = grid_ctan(0, 12)
    assert max(base[1]) > 16  # the default interval is passed more than once
    for poll in (1, 7, None):  # None: the default again, a second run of what base is
        Cg, its, rn, _ = grid_ctan.__wrapped__(0, 12, poll)
        assert np.array_equal(Cg, base[0])
        assert its == base[1]
        assert np.array_equal(np.array(rn), np.array(base[2]))


def test_max_it_stops_on_the_device_at_any_poll_interval():
    fresh = grid_ctan(0, 12)
    for poll in (7, 1):
        with M.Macroc(TM.micro_argv(0, 12)) as m:
            m.set_option("micro_solver", 1)
            m.set_option("micro_grid_poll", poll)
            m.set_option("micro_max_it", 3)
            with pytest.raises(M.MacrocError, match=r"did not converge for load case 0.*: 3 iterations"):
                m.micro_ctan()
            m.set_option("micro_max_it", 0)  # the option's default: 10 x the interior dofs
            Cg, its, rn = m.micro_ctan()
            assert np.array_equal(Cg, fresh[0]) and tuple(its) == fresh[1]
            assert np.array_equal(rn, np.array(fresh[2]))


# ---------------------------------------------------------------- 5. through the macro path
def test_through_the_macro_path():
    grid = (3, 3, 3)
    u = TN.field(grid, 11, 2e-5)
    with M.Macroc(TN.nl_argv(0, 12, grid, law="micro", extra=("-micro_solver", "grid"))) as m:
        Ch = m.micro_ctan()[0]
        b, v = TN.assemble(m, u)
        eps, sig = m.strain(), m.stress()
    assert np.array_equal(Ch, grid_ctan(0, 12, None, TN.MAT1[:2], TN.MAT2[:2])[0])  # the flag is the option
    assert np.abs(sig).max() > 0 and np.linalg.norm(b) > 0
    assert np.abs(sig - eps @ Ch.T).max() <= 1e-13 * np.abs(sig).max()
    argv = ["-da_grid_x", grid[0], "-da_grid_y", grid[1], "-da_grid_z", grid[2], "-lx", grid[0] - 1, "-ly", grid[1] - 1,
            "-lz", grid[2] - 1, "-mat_law", "external"]
    with M.Macroc(argv) as x:
        bx, vx = TN.assemble(x, u, inject=(sig, np.tile(Ch.ravel(), (sig.shape[0], 1))))
    assert np.array_equal(v, vx)
    assert np.array_equal(b, bx)


# ---------------------------------------------------------------- 6. memory
def test_workspace_is_counted_and_released():
    n = 33
    with M.Macroc(TM.micro_argv(0, n, mat1=TM.MAT2, mat2=TM.MAT2)) as m:
        m.set_option("micro_solver", 1)
        before = m.get_info()["device_bytes"]
        assert np.array_equal(m.micro_ctan()[0], grid_ctan(0, n, None, TM.MAT2, TM.MAT2)[0])
        assert m.get_info()["device_bytes"] - before >= 6 * 5 * 3 * n ** 3 * 8
    with M.Macroc(TM.micro_argv(0, 10)) as m:
        before = m.get_info()["device_bytes"]
        m.set_option("micro_solver", 1)
        Cg = m.micro_ctan()[0]
        assert m.get_info()["device_bytes"] - before >= 6 * 5 * 3 * 10 ** 3 * 8
        m.set_option("micro_solver", 0)
        assert m.get_info()["device_bytes"] == before
        Cd = m.micro_ctan()[0]  # dirty: the default solver's bits again
        assert np.array_equal(Cd, TM.gpu_ctan(0, 10)[0])
        assert m.get_info()["device_bytes"] == before
        assert np.abs(Cg - Cd).max() <= 2 * TM.bar(0, 10)


# ---------------------------------------------------------------- 7. refusals
def test_refusals():
    with M.Macroc(TM.micro_argv(0, 4)) as m:
        for bad in (2, -1, 0.5):
            with pytest.raises(M.MacrocError, match="micro_solver"):
                m.set_option("micro_solver", bad)
        for bad in (0, 5000):
            with pytest.raises(M.MacrocError, match="micro_grid_poll"):
                m.set_option("micro_grid_poll", bad)
        assert np.array_equal(m.micro_ctan()[0], TM.gpu_ctan(0, 4)[0])  # the refused values changed nothing
    with M.Macroc(TM.micro_argv(0, 129)) as m:
        m.set_option("micro_solver", 1)
        for call in (m.micro_ctan, m.homogenize, m.micro_phase):
            with pytest.raises(M.MacrocError, match=r"micro_n 129.*micro_solver"):
                call()
    with M.Macroc(TM.micro_argv(0, 21, mat1=TM.MAT2, mat2=TM.MAT2)) as m:
        with pytest.raises(M.MacrocError, match="micro_n 21"):
            m.micro_ctan()
        m.set_option("micro_solver", 1)  # the same context goes on once the solver fits the cell
        assert np.array_equal(m.micro_ctan()[0], grid_ctan(0, 21, None, TM.MAT2, TM.MAT2)[0])
    with pytest.raises(M.MacrocError, match="cell or grid, got hbm"):
        M.Macroc(TM.micro_argv(0, 4, extra=("-micro_solver", "hbm")))
    u1 = TN.field((2, 2, 2), 5, 4e-3)
    with M.Macroc(TN.nl_argv(0, 4)) as ref:
        sig_ref = TN.evaluate(ref, u1)[1]
    with M.Macroc(TN.nl_argv(0, 4)) as m:
        with pytest.raises(M.MacrocError, match="micro_nl"):
            m.set_option("micro_solver", 1)
        m.set_option("micro_solver", 0)  # no change: accepted
        assert np.array_equal(TN.evaluate(m, u1)[1], sig_ref)  # and the context homogenises, the same bits
    with M.Macroc(["-da_grid_x", 4, "-da_grid_y", 4, "-da_grid_z", 4]) as m:  # accepted, without effect
        m.set_option("micro_solver", 1)


# ---------------------------------------------------------------- 8. driver
def test_driver_takes_the_flag(tmp_path):
    exe = os.path.join(ROOT, "macroc_amd", "driver", "macroc_amd")
    argv = [exe, "-da_grid_x", "4", "-da_grid_y", "4", "-da_grid_z", "4", "-ts", "2", "-mat_law", "micro",
            "-micro_type", "0", "-micro_mat_1", "1e7,0.25,1e4,1e7", "-micro_mat_2", "1e8,0.3,1e4,1e7"]
    out = subprocess.run(argv + ["-micro_n", "24", "-micro_solver", "grid"], cwd=tmp_path, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert "Micro cell : type = 0 (sphere)\tn = 24\tmem = lds\tsolver = grid" in lines
    assert "not used" not in out.stderr and "Elapsed time" in out.stdout
    out = subprocess.run(argv + ["-micro_n", "12", "-micro_mem", "device"], cwd=tmp_path, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "Micro cell : type = 0 (sphere)\tn = 12\tmem = device" in out.stdout.splitlines()
