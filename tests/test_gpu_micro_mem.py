"""Option micro_mem 1 (-micro_mem device): the micro cell solvers with their nodal vectors in device
memory, which lifts micro_n from 10 to 20.

The main check is identity: for n <= 10 the device-memory instantiations of k_micro_rve and
k_mnl_solve run the statements of the LDS ones (same loops, same gather order, same reduction
trees, no contraction), so every result has the same bits.  Above n = 10 the dense numpy references
of test_gpu_micro.py and test_gpu_micro_nl.py judge, with their bars (100 kappa rtol); at n = 20,
where a dense reference is out of reach, the homogeneous cell has a closed form, the two-phase one
its bounds, and the non-linear law its linear limit.
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

LINEAR_CELLS = [(1, 2), (0, 3), (0, 4), (1, 5), (0, 10)]
NL_CELLS = [(0, 4), (1, 5), (1, 2)]
BIG_CELLS = [(0, 11), (1, 11), (0, 12), (1, 12)]
NL_STAGES = (1.0, 1.5, 0.5)


def ctan_of(typ, n, mem, **kw):
    with M.Macroc(TM.micro_argv(typ, n, **kw)) as m:
        m.set_option("micro_mem", mem)
        Cg, its, rn = m.micro_ctan()
        return Cg, tuple(its), tuple(rn), m.micro_phase()


# ---------------------------------------------------------------- 1. identity, linear law
@pytest.mark.parametrize("typ,n", LINEAR_CELLS)
def test_linear_law_same_bits_as_lds(typ, n):
    C0, its0, rn0, _ = ctan_of(typ, n, 0)
    C1, its1, rn1, _ = ctan_of(typ, n, 1)
    print(f"cell ({typ},{n}): its {its0} / {its1}, max rnorm {max(rn0):.3e} / {max(rn1):.3e}")
    assert np.array_equal(C0, C1)
    assert its0 == its1
    assert np.array_equal(np.array(rn0), np.array(rn1))
    assert np.abs(C1).max() > 0


# ---------------------------------------------------------------- 2. identity, non-linear law
@functools.lru_cache(maxsize=None)
def nl_run(typ, n, mem):
    """2x2x2 nodes, u -> 1.5 u -> 0.5 u with a commit between: per stage (sigma, C, info)."""
    u1 = TN.field((2, 2, 2), 5, 4e-3)
    out = []
    with M.Macroc(TN.nl_argv(typ, n)) as m:
        m.set_option("micro_mem", mem)
        for fac in NL_STAGES:
            _, sig, Cg, info = TN.evaluate(m, fac * u1)
            out.append((sig, Cg, info))
            m.update_vars()
    return out


def same_info(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("path", "newton_its", "cg_its", "rnorm"))


@pytest.mark.parametrize("typ,n", NL_CELLS)
def test_nonlinear_law_same_bits_as_lds(typ, n):
    lds, dev = nl_run(typ, n, 0), nl_run(typ, n, 1)
    for stage, ((s0, c0, i0), (s1, c1, i1)) in enumerate(zip(lds, dev)):
        print(f"cell ({typ},{n}) stage {stage}: newton {i0['newton_its']} / {i1['newton_its']} cg {i0['cg_its']} / "
              f"{i1['cg_its']}")
        assert np.array_equal(s0, s1) and np.array_equal(c0, c1)
        assert same_info(i0, i1)
        assert i0["slots_used"] == i1["slots_used"] >= 1
        assert np.abs(s1).max() > 0


# ---------------------------------------------------------------- 3. C_hom above the LDS limit
@pytest.mark.parametrize("typ,n", BIG_CELLS)
def test_chom_above_the_lds_limit(typ, n):
    with M.Macroc(TM.micro_argv(typ, n, extra=("-micro_mem", "device"))) as m:  # the flag, through mcx_apply_args
        Cg, its, rn = m.micro_ctan()
        ph = m.micro_phase()
    Cr, kappa, phr = TM.reference(typ, n)
    cmax = np.abs(Cr).max()
    bar = 100.0 * kappa * TM.RTOL * cmax
    err = np.abs(Cg - Cr).max()
    print(f"type {typ} n {n}: kappa {kappa:.1f} err/max|C| {err / cmax:.3e} bar/max|C| {bar / cmax:.3e} its {its} "
          f"rnorm {max(rn):.3e}")
    assert err <= bar
    assert all(r <= TM.RTOL for r in rn)
    assert np.array_equal(Cg, Cg.T)
    assert ph.shape == (n - 1,) * 3 and np.array_equal(ph, TM.phase_rule(typ, n)) and np.array_equal(ph, phr)
    f1 = float(ph.sum()) / (n - 1) ** 3
    C1, C2 = TM.iso_C(*TM.MAT1), TM.iso_C(*TM.MAT2)
    voigt = (1.0 - f1) * C1 + f1 * C2
    reuss = np.linalg.inv((1.0 - f1) * np.linalg.inv(C1) + f1 * np.linalg.inv(C2))
    for q in range(6):
        assert reuss[q, q] * (1 - 1e-12) <= Cg[q, q] <= voigt[q, q] * (1 + 1e-12), (q, reuss[q, q], Cg[q, q], voigt[q, q])


# ---------------------------------------------------------------- 4. the non-linear cell at n = 11
def test_nonlinear_cell_above_the_lds_limit():
    """Cell (0, 11), eight Gauss points that share one strain up to rounding (no wobble); the dense
    reference is solved for point 0's reported strain only.  Reference on the CPU: 5 and 6 Newton
    iterations, min|f|/Sy 4.2e-2 and 3.3e-1, linear-test margin 0.36, kappa 67.9."""
    ref = TN.cell(0, 11)
    u1 = TN.field((2, 2, 2), 5, 4e-3, wobble=0.0)
    hold = None
    with M.Macroc(TN.nl_argv(0, 11)) as m:
        m.set_option("micro_mem", 1)
        for stage, fac in enumerate((1.0, 1.5)):
            eps, sig, Cg, info = TN.evaluate(m, fac * u1)
            r = ref.point(eps[0], hold)
            TN.check_conditions(r)
            bar = 100 * r["kappa"] * TN.NL_RTOL
            smax, cmax = np.abs(r["sig"]).max(), np.abs(r["C"]).max()
            es, ec = np.abs(sig[0] - r["sig"]).max() / smax, np.abs(Cg[0] - r["C"]).max() / cmax
            ds = max(np.abs(sig[q] - sig[0]).max() for q in range(1, 8)) / smax
            dc = max(np.abs(Cg[q] - Cg[0]).max() for q in range(1, 8)) / cmax
            print(f"stage {stage}: kappa {r['kappa']:.1f} ref newton {r['its']} margin {r['margin']:.2e} mlin "
                  f"{r['mlin']:.2e} gpu newton {info['newton_its']} cg {info['cg_its']} err sigma {es:.2e} C {ec:.2e} "
                  f"spread sigma {ds:.2e} C {dc:.2e} bar {bar:.2e} rnorm {info['rnorm'].max():.1e}")
            assert r["path"] == 1 and (info["path"] == 1).all()
            assert es <= bar and ec <= bar
            assert ds <= bar and dc <= bar
            assert (info["rnorm"] <= TN.NL_RTOL).all()
            for q in range(8):
                assert np.array_equal(Cg[q], Cg[q].T)
            hold = r["h"]
            m.update_vars()
        assert info["slots_used"] == 8 and info["bytes_per_slot"] == 224 * 8 * 10 ** 3


# ---------------------------------------------------------------- 5. n = 20
def test_n20_homogeneous_cell_is_isotropic():
    """Equal phases at n = 20: the exact C_hom is the phase's isotropic tensor.  The bar's kappa is
    the dense reference's at n = 12 (the same homogeneous cell) scaled by (19/11)^2, the growth of
    the Jacobi-scaled stiffness' condition number with 1/h^2."""
    kappa12 = TM.reference(0, 12, TM.MAT2, TM.MAT2)[1]
    kappa = kappa12 * (19.0 / 11.0) ** 2
    Cg, its, rn, _ = ctan_of(0, 20, 1, mat1=TM.MAT2, mat2=TM.MAT2)
    Ci = TM.iso_C(*TM.MAT2)
    err = np.abs(Cg - Ci).max() / np.abs(Ci).max()
    kappa_est = (max(its) / np.log(2.0 / TM.RTOL) * 2.0) ** 2  # CG: its ~ sqrt(kappa) / 2 ln(2 / rtol); printout only
    print(f"n 20 homogeneous: its {its} rnorm {max(rn):.3e} err/max|C| {err:.3e} bar {100 * kappa * TM.RTOL:.3e} "
          f"kappa(n=12) {kappa12:.1f} scaled {kappa:.1f} estimated from the iterations {kappa_est:.1f}")
    assert err <= 100.0 * kappa * TM.RTOL
    assert all(r <= TM.RTOL for r in rn) and min(its) >= 1
    assert np.array_equal(Cg, Cg.T)


def test_n20_sphere_structure():
    Cg, its, rn, ph = ctan_of(0, 20, 1)
    print(f"n 20 sphere: its {its} rnorm {max(rn):.3e} C00 {Cg[0, 0]:.6e} C33 {Cg[3, 3]:.6e}")
    assert ph.shape == (19,) * 3 and np.array_equal(ph, TM.phase_rule(0, 20))
    assert all(r <= TM.RTOL for r in rn)
    assert np.array_equal(Cg, Cg.T)
    f1 = float(ph.sum()) / 19 ** 3
    C1, C2 = TM.iso_C(*TM.MAT1), TM.iso_C(*TM.MAT2)
    voigt = (1.0 - f1) * C1 + f1 * C2
    reuss = np.linalg.inv((1.0 - f1) * np.linalg.inv(C1) + f1 * np.linalg.inv(C2))
    for q in range(6):
        assert reuss[q, q] * (1 - 1e-12) <= Cg[q, q] <= voigt[q, q] * (1 + 1e-12), (q, reuss[q, q], Cg[q, q], voigt[q, q])


def test_n20_nonlinear_converges_and_unloads_to_chom():
    u1 = TN.field((2, 2, 2), 5, 4e-3, wobble=0.0)
    with M.Macroc(TN.nl_argv(0, 20, law="micro")) as lin:
        lin.set_option("micro_mem", 1)
        Ch = lin.micro_ctan()[0]
    with M.Macroc(TN.nl_argv(0, 20)) as m:
        m.set_option("micro_mem", 1)
        _, sig, Cg, info = TN.evaluate(m, u1)
        print(f"n 20: newton {info['newton_its']} cg {info['cg_its']} rnorm {info['rnorm'].max():.1e} bytes per slot "
              f"{info['bytes_per_slot']}")
        assert info["path"].all() and (info["rnorm"] <= TN.NL_RTOL).all() and (info["newton_its"] >= 1).all()
        assert info["slots_used"] == 8 and info["slots"] == 8
        assert info["bytes_per_slot"] == 224 * 8 * 19 ** 3
        for q in range(8):
            assert np.array_equal(Cg[q], Cg[q].T) and np.isfinite(sig[q]).all()
            assert np.linalg.eigvalsh(Cg[q]).min() > 0
    with M.Macroc(TN.nl_argv(0, 20)) as m:  # a fresh context below yield: the linear law's C_hom, bit for bit
        m.set_option("micro_mem", 1)
        _, sig, Cg, info = TN.evaluate(m, 0.01 * u1)
        assert not info["path"].any() and info["slots"] == 0
        for q in range(8):
            assert np.array_equal(Cg[q], Ch)


# ---------------------------------------------------------------- 6. the walk
def test_walk_order_does_not_matter():
    """3x3x3 nodes, 64 yielding Gauss points; element 0 carries the 2x2x2 run's displacements, so
    its eight points must give that run's bits, whether 64 blocks take one point each or 5 blocks
    (option micro_mem_blocks) walk the list in 13 uneven rounds."""
    grid = (3, 3, 3)
    u1 = TN.field((2, 2, 2), 5, 4e-3).reshape(2, 2, 2, 3)
    u = TN.field(grid, 5, 4e-3).reshape(3, 3, 3, 3)
    u[:2, :2, :2] = u1  # [k][j][i][component]: the nodes of element 0
    sig_ref, C_ref, info_ref = nl_run(0, 4, 1)[0]
    res = []
    for blocks in (0, 5):
        with M.Macroc(TN.nl_argv(0, 4, grid)) as m:
            m.set_option("micro_mem", 1)
            m.set_option("micro_mem_blocks", blocks)
            eps, sig, Cg, info = TN.evaluate(m, u.ravel())
            assert info["path"].all() and info["slots_used"] == 64
            res.append((sig, Cg, info))
    for sig, Cg, info in res:
        assert np.array_equal(sig[:8], sig_ref) and np.array_equal(Cg[:8], C_ref)
        for k in ("newton_its", "cg_its", "rnorm"):
            assert np.array_equal(info[k][:8], info_ref[k])
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1]) and same_info(res[0][2], res[1][2])


# ---------------------------------------------------------------- 7. refusals
def test_refusals():
    u1 = TN.field((2, 2, 2), 5, 4e-3)
    with M.Macroc(TM.micro_argv(0, 4)) as m:
        for bad in (2, -1, 0.5):
            with pytest.raises(M.MacrocError, match="micro_mem"):
                m.set_option("micro_mem", bad)
        C0 = m.micro_ctan()[0]
        m.set_option("micro_mem", 1)  # marks the cell dirty: recomputed, the same bits
        assert np.array_equal(m.micro_ctan()[0], C0)
    with M.Macroc(TM.micro_argv(0, 21)) as m:
        m.set_option("micro_mem", 1)
        for call in (m.micro_ctan, m.homogenize, m.micro_phase):
            with pytest.raises(M.MacrocError, match="micro_n 21"):
                call()
    with M.Macroc(TM.micro_argv(0, 11)) as m:
        with pytest.raises(M.MacrocError, match=r"micro_n 11.*micro_mem"):
            m.micro_ctan()
        m.set_option("micro_mem", 1)  # the same context goes on once the mode fits the cell
        Cr, kappa, _ = TM.reference(0, 11)
        assert np.abs(m.micro_ctan()[0] - Cr).max() <= 100.0 * kappa * TM.RTOL * np.abs(Cr).max()
    with pytest.raises(M.MacrocError, match="lds or device"):
        M.Macroc(TM.micro_argv(0, 4, extra=("-micro_mem", "hbm")))
    with M.Macroc(TN.nl_argv(0, 4)) as m:
        sig = TN.evaluate(m, u1)[1]
        assert m.micro_nl_info()["slots_used"] >= 1
        with pytest.raises(M.MacrocError, match="micro_mem.*slots are in use"):
            m.set_option("micro_mem", 1)
        m.set_option("micro_mem", 0)  # no change: accepted
        m.homogenize()  # and the context still homogenises
        assert np.array_equal(m.stress().reshape(-1, 6), sig)
        assert np.array_equal(sig, nl_run(0, 4, 0)[0][0])
    with M.Macroc(TN.nl_argv(0, 11, extra=("-micro_mem", "device", "-micro_nl_slots", 1))) as m:
        m.set_u(u1)
        m.set_strains()
        with pytest.raises(M.MacrocError, match=r"micro_nl_slots 1, 0 slots in use and 8 more.*%d bytes per slot"
                                                % (224 * 8 * 10 ** 3)):
            m.homogenize()
        assert m.micro_nl_info()["slots"] == 0


# ---------------------------------------------------------------- 8. driver
def test_driver_takes_the_flag(tmp_path):
    exe = os.path.join(ROOT, "macroc_amd", "driver", "macroc_amd")
    argv = [exe, "-da_grid_x", "4", "-da_grid_y", "4", "-da_grid_z", "4", "-ts", "2", "-mat_law", "micro",
            "-micro_n", "12", "-micro_type", "0", "-micro_mat_1", "1e7,0.25,1e4,1e7", "-micro_mat_2", "1e8,0.3,1e4,1e7"]
    out = subprocess.run(argv + ["-micro_mem", "device"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert "Micro cell : type = 0 (sphere)\tn = 12\tmem = device" in lines
    row = [float(v) for v in lines[lines.index("C_hom : ") + 1].split()]
    Cr = TM.reference(0, 12)[0]
    assert np.abs(np.array(row) - Cr[0]).max() <= 1e-6 * np.abs(Cr).max()  # %e prints 7 digits
    assert "not used" not in out.stderr and "Elapsed time" in out.stdout
    out = subprocess.run(argv, cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert out.returncode != 0
    assert "micro_n" in out.stdout + out.stderr
