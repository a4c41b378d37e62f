"""Option micro_nl_solver 1 (-micro_nl_solver grid): the cells of -mat_law micro_nl solved by launches
over the whole device, one workgroup per 8x8x8 tile and one launch per phase, for 2 <= micro_n <= 64
(DESIGN §18).  The definition is §12's; only the order of the dot-product sums differs from solver
0, so the two agree to the Newton / CG tolerances and not bit for bit.  The project's bar judges
(test_gpu_micro_nl.py):
    max|x_gpu - x_ref| <= 100 kappa micro_nl_rtol max|x_ref|      (x = sigma, C)
against the dense numpy reference (kappa from the reference) up to n = 9, against solver 0 up to
n = 17 (the sum of the two bars), and above n = 20, in this file, against what is known in closed
form: a cell of equal phases is solved by the affine field, so it must give the law of -mat_law
plastic.  Heterogeneous cells at n = 21 and 26 are judged against a sparse CPU reference's recorded
results in test_gpu_micro_cells_resolved.py.  kappa above n = 12 is, here, the dense linear
reference's at n = 12 scaled by ((n - 1) / 11)^2.

Every test sets micro_nl_solver 1.  Measured on an MI355X: DESIGN §18 has the tables.
"""
import functools
import os
import subprocess
import threading

import numpy as np
import pytest

import macroc_amd as M
import test_gpu_micro as TM
import test_gpu_micro_nl as TN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NL_RTOL = TN.NL_RTOL
# n = 9: the reference was run alone on the CPU first, for TN.LOADS and the neighbours (5, 2e-3), (7, 1e-3),
# (7, 4e-3).  (5, 4e-3) is kept for both cells: on the sphere the reference takes 5 Newton iterations to
# 1e-13 with min |f| / Sy = 5.5e-4, on the layer 6 with 3.0e-1 (TN.check_conditions allows 10; on the layer
# (7, 2e-3), (5, 2e-3) and (7, 1e-3) take 39 iterations and (7, 4e-3) takes 7, so none was closer to 5)
REF_CASES = [(t, n, s, a) for (t, n) in TN.CELLS for (s, a) in TN.LOADS] + [(0, 9, 5, 4e-3), (1, 9, 5, 4e-3)]
# equal phases: J2 with a yield the load crosses.  The hardening modulus is the project's default (1e7, of the
# order of E): with TN.MAT1's 1e6 the law's plain Newton from a zero interior gives up after 20 iterations on
# the unload stage at every n >= 12, under solver 0 and solver 1 alike ("What plain Newton cannot do")
EQ = (1.0e7, 0.25, 1.0e4, 1.0e7)
EQ_FLAGS = ("-micro_mat_1", "%r,%r,%r,%r" % EQ, "-micro_mat_2", "%r,%r,%r,%r" % EQ)


def grid_ctx(argv, **opts):
    m = M.Macroc(argv)
    m.set_option("micro_nl_solver", 1)
    for k, v in opts.items():
        m.set_option(k, v)
    return m


def scaled_kappa(n, mats=(TM.MAT1, TM.MAT2)):
    return TM.reference(0, 12, *mats)[1] * ((n - 1) / 11.0) ** 2


def stages_of(m, u1, stages, nl=True):
    out = []
    for fac in stages:
        m.set_u(fac * u1)
        m.set_strains()
        m.homogenize()
        out.append(dict(eps=m.gp_strain(), sig=m.stress().reshape(-1, 6), C=m.gp_ctan(),
                        info=m.micro_nl_info() if nl else None, stats=m.nonlinear_stats()))
        m.update_vars()
    return out


# ---------------------------------------------------------------- 1. against the dense reference
@pytest.mark.parametrize("typ,n,seed,amp", REF_CASES)
def test_against_reference(typ, n, seed, amp):
    """TN.test_against_reference under solver 1: 8 Gauss points with their own strains through
    u -> 1.5 u -> 0.5 u with commits.  n = 3 has one interior node, n <= 5 is one partial tile, n = 9
    has two tiles per axis, the second one node wide."""
    ref = TN.cell(typ, n)
    u1 = TN.field((2, 2, 2), seed, amp)
    hold = [None] * 8
    with grid_ctx(TN.nl_argv(typ, n)) as m:
        for stage, fac in enumerate(TN.STAGES):
            eps, sig, Cg, info = TN.evaluate(m, fac * u1)
            for q in range(8):
                r = ref.point(eps[q], hold[q])
                TN.check_conditions(r)
                assert info["path"][q] == r["path"]
                bar = 100 * r["kappa"] * NL_RTOL
                es = np.abs(sig[q] - r["sig"]).max() / np.abs(r["sig"]).max()
                ec = np.abs(Cg[q] - r["C"]).max() / np.abs(r["C"]).max()
                print(f"cell ({typ},{n}) load ({seed},{amp}) stage {stage} gp {q}: path {r['path']} kappa "
                      f"{r['kappa']:.1f} err sigma {es:.2e} C {ec:.2e} bar {bar:.2e} newton gpu "
                      f"{info['newton_its'][q]} ref {r['its']} margin {r['margin']:.1e} cg {info['cg_its'][q]} "
                      f"rnorm {info['rnorm'][q]:.1e}")
                assert es <= bar and ec <= bar
                assert info["rnorm"][q] <= NL_RTOL
                assert np.array_equal(Cg[q], Cg[q].T)
                if r["path"]:
                    hold[q] = r["h"]
            m.update_vars()
        assert info["slots_used"] == sum(h is not None for h in hold) and info["slots"] >= info["slots_used"]
        assert any(h is not None for h in hold)  # the load yields


# ---------------------------------------------------------------- 2. against solver 0
@pytest.mark.parametrize("n,mem", [(10, 0), (12, 1), (17, 1)])
def test_against_solver_0(n, mem):
    """one yielding load, two stages with a commit: sigma, C and f_trial within the sum of the two
    bars (kappa = the n = 12 reference's x ((n - 1) / 11)^2), equal paths, Newton counts within 1.
    n = 17 has two full tiles plus one node.  f_trial's error is the trial stress's, which is no
    smaller than sqrt(2/3) Sy where f > 0: that is its scale.  (Load (5, 4e-3): at n = 17 both
    solvers' Newton gives up on (5, 2e-3) x 1.5 with the same counts)"""
    u1 = TN.field((2, 2, 2), 5, 4e-3)
    with M.Macroc(TN.nl_argv(0, n)) as m:
        m.set_option("micro_mem", mem)
        a = stages_of(m, u1, (1.0, 1.5))
    with grid_ctx(TN.nl_argv(0, n)) as m:
        b = stages_of(m, u1, (1.0, 1.5))
    bar = 2 * 100 * scaled_kappa(n) * NL_RTOL
    for st, (x, y) in enumerate(zip(a, b)):
        es = np.abs(x["sig"] - y["sig"]).max() / np.abs(x["sig"]).max()
        ec = np.abs(x["C"] - y["C"]).max() / np.abs(x["C"]).max()
        ef = abs(x["stats"][1] - y["stats"][1]) / (x["stats"][1] + np.sqrt(2 / 3) * TN.MAT1[2])
        print(f"n {n} stage {st}: |d sigma| {es:.2e} |d C| {ec:.2e} |d f| {ef:.2e} bar {bar:.2e} newton "
              f"{x['info']['newton_its']} / {y['info']['newton_its']} cg {x['info']['cg_its'].max()} / "
              f"{y['info']['cg_its'].max()}")
        assert x["info"]["path"].all() and x["stats"][1] > 0  # the load yields
        assert np.array_equal(x["info"]["path"], y["info"]["path"]) and x["stats"][0] == y["stats"][0]
        assert es <= bar and ec <= bar and ef <= bar
        assert np.abs(x["info"]["newton_its"] - y["info"]["newton_its"]).max() <= 1
        assert (y["info"]["rnorm"] <= NL_RTOL).all()


# ---------------------------------------------------------------- 3. above n = 20
@pytest.mark.parametrize("n", [21, 33])
def test_equal_phases_are_the_plastic_law(n):
    """the affine field solves a cell of equal phases, so sigma, the tangent and f_trial are those of
    -mat_law plastic at the same macro strains, also after a commit and a partial unload.  Newton
    starts from a zero interior, so it has real work to do."""
    u1 = TN.field((2, 2, 2), 5, 4e-3)
    with M.Macroc(TN.nl_argv(0, 2, law="plastic", extra=EQ_FLAGS)) as m:
        a = stages_of(m, u1, (1.0, 0.5), nl=False)
    with grid_ctx(TN.nl_argv(0, n, extra=EQ_FLAGS)) as m:
        b = stages_of(m, u1, (1.0, 0.5))
        assert m.micro_nl_info()["bytes_per_slot"] == 224 * 8 * (n - 1) ** 3
    bar = 100 * scaled_kappa(n, (EQ[:2], EQ[:2])) * NL_RTOL
    assert a[0]["stats"][0] == 8  # every point yields in stage 1
    for st, (x, y) in enumerate(zip(a, b)):
        smax = np.abs(x["sig"]).max()
        es = np.abs(x["sig"] - y["sig"]).max() / smax
        ec = np.abs(x["C"] - y["C"]).max() / np.abs(x["C"]).max()
        ef = abs(x["stats"][1] - y["stats"][1]) / smax  # the trial stress is of the stresses' size
        print(f"equal phases n {n} stage {st}: err sigma {es:.2e} C {ec:.2e} f {ef:.2e} bar {bar:.2e} newton "
              f"{y['info']['newton_its']} cg {y['info']['cg_its']} rnorm {y['info']['rnorm'].max():.1e}")
        assert np.array_equal(x["eps"], y["eps"])
        assert es <= bar and ec <= bar and ef <= bar
        assert x["stats"][0] == y["stats"][0]
        assert y["info"]["path"].all() and (y["info"]["rnorm"] <= NL_RTOL).all()
        assert (y["info"]["newton_its"] >= 2).all()


def test_sphere_cell_n21():
    """(0, 21): at the first, linear call C = C_hom has cubic symmetry to the bar and its diagonal
    lies between the Reuss and Voigt bounds; then one yielding stage converges at every point."""
    n, u1 = 21, TN.field((2, 2, 2), 5, 4e-3)
    bar = 100 * scaled_kappa(n) * TM.RTOL
    with grid_ctx(TN.nl_argv(0, n)) as m:
        eps, sig, Cg, info = TN.evaluate(m, 0.01 * u1)
        assert not info["path"].any() and info["slots"] == 0
        Ch, ph = Cg[0], m.micro_phase()
        groups = ((Ch[0, 0], Ch[1, 1], Ch[2, 2]), (Ch[0, 1], Ch[0, 2], Ch[1, 2]), (Ch[3, 3], Ch[4, 4], Ch[5, 5]))
        spread = max(max(g) - min(g) for g in groups) / np.abs(Ch).max()
        f1 = float(ph.sum()) / (n - 1) ** 3
        C1, C2 = TM.iso_C(*TN.MAT1[:2]), TM.iso_C(*TN.MAT2[:2])
        voigt = (1.0 - f1) * C1 + f1 * C2
        reuss = np.linalg.inv((1.0 - f1) * np.linalg.inv(C1) + f1 * np.linalg.inv(C2))
        print(f"sphere n {n}: cubic spread {spread:.2e} bar {bar:.2e} C00 {Ch[0, 0]:.6e}")
        assert spread <= bar and np.array_equal(Ch, Ch.T)
        for q in range(6):
            assert reuss[q, q] * (1 - 1e-12) <= Ch[q, q] <= voigt[q, q] * (1 + 1e-12)
        eps, sig, Cg, info = TN.evaluate(m, u1)
        print(f"sphere n {n}: newton {info['newton_its']} cg {info['cg_its']} rnorm {info['rnorm'].max():.1e}")
        assert info["path"].all() and (info["rnorm"] <= NL_RTOL).all() and info["slots_used"] == 8
        for q in range(8):
            assert np.array_equal(Cg[q], Cg[q].T) and np.linalg.eigvalsh(Cg[q]).min() > 0


# ---------------------------------------------------------------- 4. below yield
def test_below_yield_is_the_linear_grid_solver_bit_for_bit():
    grid = (5, 4, 3)
    u = TN.field(grid, 11, 2e-5)
    with grid_ctx(TN.nl_argv(1, 9, grid)) as a:
        ba, va = TN.assemble(a, u)
        eps, sa, info = a.strain(), a.stress(), a.micro_nl_info()
        Ch = a.micro_ctan()[0]
        assert not info["path"].any() and info["slots"] == 0 and info["slots_used"] == 0
        assert np.abs(sa - eps @ Ch.T).max() <= 1e-13 * np.abs(sa).max()
    with M.Macroc(TN.nl_argv(1, 9, grid, law="micro", extra=("-micro_solver", "grid"))) as b:
        bb, vb = TN.assemble(b, u)
        sb = b.stress()
    assert np.linalg.norm(bb) > 0
    assert np.array_equal(sa, sb) and np.array_equal(ba, bb) and np.array_equal(va, vb)


# ---------------------------------------------------------------- 5. determinism and independence
def run_stages(typ, n, u1, grid=(2, 2, 2), **opts):
    with grid_ctx(TN.nl_argv(typ, n, grid), **opts) as m:
        return [(s["eps"], s["sig"], s["C"], s["info"]["newton_its"], s["info"]["cg_its"], s["info"]["rnorm"])
                for s in stages_of(m, u1, TN.STAGES)]  # the histories show in the later stages


@functools.lru_cache(maxsize=None)
def base_run():
    return run_stages(0, 9, TN.field((2, 2, 2), 5, 4e-3))


def test_two_runs_are_bitwise_equal():
    again = run_stages(0, 9, TN.field((2, 2, 2), 5, 4e-3))
    for a, b in zip(base_run(), again):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)


@pytest.mark.parametrize("blocks", [0, 3])
def test_results_do_not_depend_on_slot_grid_or_batch(blocks):
    """the 2x2x2 grid's element again as the second element of a 3x2x2 grid whose first element is
    solved too: other slots, other places in the batch; with micro_mem_blocks 3 the sixteen points
    go in batches of three, so the element's points share launches with other points."""
    u1 = TN.field((2, 2, 2), 5, 4e-3).reshape(2, 2, 2, 3)  # [k][j][i]
    big = np.zeros((2, 2, 3, 3))
    big[:, :, 1:, :] = u1
    big[:, :, 0, :] = TN.field((2, 2, 2), 9, 4e-3).reshape(2, 2, 2, 3)[:, :, 0, :]
    out = run_stages(0, 9, big.ravel(), (3, 2, 2), micro_mem_blocks=blocks)
    for a, b in zip(base_run(), out):
        assert b[3][:8].all()  # the first element is solved too
        for x, y in zip(a, b):
            assert np.array_equal(x, y[8:])


@pytest.mark.parametrize("poll", [1, 7])
def test_bits_do_not_depend_on_the_poll_interval(poll):
    assert max(s[4].max() for s in base_run()) > 16 * 7  # CGs longer than the default interval
    out = run_stages(0, 9, TN.field((2, 2, 2), 5, 4e-3), micro_grid_poll=poll)
    for a, b in zip(base_run(), out):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)


# ---------------------------------------------------------------- 6. plumbing
@functools.lru_cache(maxsize=None)
def mixed_state():
    with grid_ctx(TN.nl_argv(*TN.MIXED_CELL, TN.MIXED_GRID)) as m:
        b, v = TN.assemble(m, TN.mixed_u())
        return dict(b=b, v=v, eps=m.gp_strain(), sig=m.stress().reshape(-1, 6), C=m.gp_ctan(), info=m.micro_nl_info(),
                    dirichlet=m.dump_dirichlet())


def test_mixed_grid_plumbing():
    S, ref = mixed_state(), TN.cell(*TN.MIXED_CELL)
    path = np.array([ref.point(e)["path"] for e in S["eps"]])
    assert 0 < path.sum() < len(path) and np.array_equal(S["info"]["path"], path)
    b, v = TN.external(TN.mixed_u(), S["sig"], S["C"])
    assert np.array_equal(b, S["b"]) and np.array_equal(v, S["v"])


def test_tangent_consistency_at_the_macro_level():
    """TN's central-difference check under solver 1: within 10 x the reference's own figure."""
    S, ref, u = mixed_state(), TN.cell(*TN.MIXED_CELL), TN.mixed_u()
    v = np.random.default_rng(3).uniform(-1, 1, len(u))
    v[S["dirichlet"]] = 0.0
    h = 1e-7 * TN.MIXED_AMP
    free = np.ones(len(u), bool)
    free[S["dirichlet"]] = False

    def mismatch(bp, bm, Av):
        return np.abs((bp - bm)[free] / (2 * h) + Av[free]).max() / np.abs(Av[free]).max()

    with grid_ctx(TN.nl_argv(*TN.MIXED_CELL, TN.MIXED_GRID)) as m:
        TN.assemble(m, u)
        Av = m.spmv(v)
        bp, _ = TN.assemble(m, u + h * v)
        ep = m.gp_strain()
        bm, _ = TN.assemble(m, u - h * v)
        em = m.gp_strain()
    gpu = mismatch(bp, bm, Av)
    G = TN.MIXED_GRID
    argv = ["-da_grid_x", G[0], "-da_grid_y", G[1], "-da_grid_z", G[2], "-lx", G[0] - 1, "-ly", G[1] - 1,
            "-lz", G[2] - 1, "-mat_law", "external"]
    pts = [ref.point(e) for e in S["eps"]]
    Cref = np.array([r["C"] for r in pts])
    with M.Macroc(argv) as x:
        TN.assemble(x, u, inject=(np.array([r["sig"] for r in pts]), Cref))
        Avr = x.spmv(v)
        rbp, _ = TN.assemble(x, u + h * v, inject=(np.array([ref.point(e)["sig"] for e in ep]), Cref))
        rbm, _ = TN.assemble(x, u - h * v, inject=(np.array([ref.point(e)["sig"] for e in em]), Cref))
    refm = mismatch(rbp, rbm, Avr)
    print(f"central-difference mismatch: reference {refm:.3e}, gpu {gpu:.3e}")
    assert gpu <= 10 * refm


# ---------------------------------------------------------------- 7. limits and refusals
def test_option_values_words_and_slots_in_use():
    u1 = TN.field((2, 2, 2), 5, 4e-3)
    with M.Macroc(TN.nl_argv(0, 4)) as m:
        for bad in (2, -1, 0.5):
            with pytest.raises(M.MacrocError, match=r"micro_nl_solver: 0 \(.*micro_n <= 10 / 20.*\) or 1 \(.*micro_n <= 64\)"):
                m.set_option("micro_nl_solver", bad)
        sig0 = TN.evaluate(m, u1)[1]  # the refused values changed nothing: solver 0 still
        with pytest.raises(M.MacrocError, match="micro_nl_solver: 8 history slots are in use"):
            m.set_option("micro_nl_solver", 1)
        m.set_option("micro_nl_solver", 0)  # no change: accepted
        assert np.array_equal(TN.evaluate(m, u1)[1], sig0)
    with M.Macroc(TN.nl_argv(0, 4)) as m:
        assert np.array_equal(TN.evaluate(m, u1)[1], sig0)
    with grid_ctx(TN.nl_argv(0, 4)) as m:
        sig1 = TN.evaluate(m, u1)[1]
        with pytest.raises(M.MacrocError, match="micro_nl_solver: 8 history slots are in use"):
            m.set_option("micro_nl_solver", 0)
        assert np.array_equal(TN.evaluate(m, u1)[1], sig1)
    for where in (M.parse_args, M.Macroc):
        with pytest.raises(M.MacrocError, match="-micro_nl_solver: cell or grid, got hbm"):
            where(TN.nl_argv(0, 4, extra=("-micro_nl_solver", "hbm")))
    with M.Macroc(TN.nl_argv(0, 4, extra=("-micro_nl_solver", "grid"))) as m:  # the flag is the option
        assert np.array_equal(TN.evaluate(m, u1)[1], sig1)
    for law in ("micro", "elastic"):  # accepted, no effect
        with M.Macroc(TN.nl_argv(0, 4, law=law)) as m:
            before = m.get_info()["device_bytes"]
            m.set_option("micro_nl_solver", 1)
            m.set_u(u1)
            m.set_strains()
            m.homogenize()
            s = m.stress()
            m.set_option("micro_nl_solver", 0)
        with M.Macroc(TN.nl_argv(0, 4, law=law)) as m:
            m.set_u(u1)
            m.set_strains()
            m.homogenize()
            assert np.array_equal(m.stress(), s)


def test_micro_n_limits():
    u1 = TN.field((2, 2, 2), 5, 4e-3)
    for n in (65, 1):
        with grid_ctx(TN.nl_argv(0, n)) as m:
            m.set_u(u1)
            m.set_strains()
            for call in (m.homogenize, m.micro_ctan):
                with pytest.raises(M.MacrocError, match=r"micro_n %d outside .*<= 64 \(option micro_nl_solver 1" % n):
                    call()
    with M.Macroc(TN.nl_argv(0, 21, extra=EQ_FLAGS)) as m:
        m.set_u(u1)
        m.set_strains()
        with pytest.raises(M.MacrocError, match=r"micro_n 21 outside .*<= 10 \(option micro_mem 0"):
            m.homogenize()
        m.set_option("micro_nl_solver", 1)  # the same context goes on once the solver fits the cell
        m.homogenize()
        info = m.micro_nl_info()
        assert info["path"].all() and (info["rnorm"] <= NL_RTOL).all()


def test_newton_limit_and_pool_messages_are_todays():
    u1 = TN.field((2, 2, 2), 5, 4e-3)
    with grid_ctx(TN.nl_argv(0, 4)) as m:
        m.set_option("micro_nl_max_it", 1)
        m.set_u(u1)
        m.set_strains()
        with pytest.raises(M.MacrocError, match=r"\d+ of 8 micro cells did not converge; worst: Gauss point \d+ "
                                                r"\(Newton gave up\): 1 Newton iterations \(micro_nl_max_it 1\)"):
            m.homogenize()
        m.set_option("micro_nl_max_it", 20)
        m.homogenize()
        sig, Cg = m.stress().reshape(-1, 6), m.gp_ctan()
    with grid_ctx(TN.nl_argv(0, 4)) as m:
        _, s2, c2, _ = TN.evaluate(m, u1)
        assert np.array_equal(s2, sig) and np.array_equal(c2, Cg)
    with grid_ctx(TN.nl_argv(0, 4), micro_nl_slots=1) as m:
        m.set_u(u1)
        m.set_strains()
        with pytest.raises(M.MacrocError, match=r"micro_nl_slots 1, 0 slots in use and 8 more"):
            m.homogenize()
        assert m.micro_nl_info()["slots"] == 0
        m.set_option("micro_nl_slots", 8)
        m.homogenize()
        assert np.array_equal(m.stress().reshape(-1, 6), sig)


def test_workspace_is_counted_and_released():
    n, u1 = 12, TN.field((2, 2, 2), 5, 4e-6)  # below yield: no slot, the option stays free
    with M.Macroc(TN.nl_argv(0, n)) as m:
        m.set_option("micro_mem", 1)
        before = m.get_info()["device_bytes"]
        m.set_option("micro_nl_solver", 1)
        _, _, _, info = TN.evaluate(m, u1)
        assert not info["path"].any() and info["slots"] == 0
        grown = m.get_info()["device_bytes"] - before
        fields = (6 * 3 * n ** 3 + 38 * 8 * (n - 1) ** 3) * 8  # the unit-strain fields and concentration tensors stay
        assert grown - fields >= 8 * 6 * 3 * n ** 3 * 8  # eight solves' six vectors
        m.set_option("micro_nl_solver", 0)
        assert m.get_info()["device_bytes"] == before + fields


# ---------------------------------------------------------------- 8. two in-process ranks
def test_two_ranks_match_one():
    grid = (10, 8, 8)
    probe = ["-da_grid_x", grid[0], "-da_grid_y", grid[1], "-da_grid_z", grid[2], "-mat_law", "elastic"]
    with M.Macroc(probe) as m:  # the load of time step 1; Sy of phase 1 is set so that part of the grid yields
        for ts in (0, 1):
            m.apply_bc_on_u(m.get_displacement(ts))
        m.set_strains()
        eps = m.gp_strain()
    tr = eps[:, :3].sum(1)
    dev = np.concatenate([eps[:, :3] - tr[:, None] / 3, eps[:, 3:] / 2], axis=1)
    dn = np.sqrt((dev[:, :3] ** 2).sum(1) + 2 * (dev[:, 3:] ** 2).sum(1))
    Sy = float("%.3e" % (np.sqrt(1.5) * 2 * TN.MAT1[0] / (2 * (1 + TN.MAT1[1])) * np.quantile(dn[dn > 0], 0.8)))
    argv = ["-da_grid_x", grid[0], "-da_grid_y", grid[1], "-da_grid_z", grid[2], "-mat_law", "micro_nl", "-micro_n", 4,
            "-micro_type", 0, "-micro_mat_1", "%r,%r,%r,%r" % (TN.MAT1[0], TN.MAT1[1], Sy, TN.MAT1[3]),
            "-micro_mat_2", "%r,%r,%r,%r" % TN.MAT2, "-ksp_rtol", repr(1e-12), "-micro_nl_solver", "grid"]

    def fn(m):
        for ts in (0, 1):
            m.apply_bc_on_u(m.get_displacement(ts))
        m.set_strains()
        m.homogenize()
        m.assembly_res()
        m.assembly_jac()
        its, rn, reason = m.solve_Ax()
        return dict(du=m.du(), reason=reason, nat=m.owned_dofs()[1], force=m.calc_force(), nl=m.reduce_nonlinear())

    with M.Macroc(argv) as m1:
        one = fn(m1)
    assert one["reason"] > 0 and np.linalg.norm(one["du"]) > 0.0
    assert 0 < one["nl"][1] < 8 * 9 * 7 * 7
    g = M.LocalGroup(2)
    res, errors = [None, None], []

    def worker(r):
        try:
            m = M.Macroc(argv, rank=r, nranks=2, group=g)
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
    du, ref = np.zeros_like(one["du"]), np.zeros_like(one["du"])
    for r in res:
        du[r["nat"]] = r["du"]
        assert r["nl"][1:] == one["nl"][1:]  # the count and the largest trial f, bit for bit
        assert abs(r["force"] - one["force"]) <= 1e-10 * abs(one["force"])
    ref[one["nat"]] = one["du"]
    assert np.linalg.norm(du - ref) <= 1e-10 * np.linalg.norm(ref)  # the macro CG sums in another order
    assert res[0]["nl"][0] + res[1]["nl"][0] == one["nl"][1]


# ---------------------------------------------------------------- 9. driver
def test_driver_takes_the_flag(tmp_path):
    grid = ("-da_grid_x", "4", "-da_grid_y", "4", "-da_grid_z", "4")
    with M.Macroc(list(grid) + ["-mat_law", "elastic"]) as m:  # Sy from the load of time step 1: a few points yield
        for ts in (0, 1):
            m.apply_bc_on_u(m.get_displacement(ts))
        m.set_strains()
        eps = m.gp_strain()
    tr = eps[:, :3].sum(1)
    dev = np.concatenate([eps[:, :3] - tr[:, None] / 3, eps[:, 3:] / 2], axis=1)
    dn = np.sqrt((dev[:, :3] ** 2).sum(1) + 2 * (dev[:, 3:] ** 2).sum(1))
    Sy = np.sqrt(1.5) * 2 * 1e7 / (2 * 1.25) * np.quantile(dn[dn > 0], 0.9)
    # hardening 1e8: with 1e6 the cells' plain Newton gives up on this load under either solver
    exe = os.path.join(ROOT, "macroc_amd", "driver", "macroc_amd")
    out = subprocess.run([exe, *grid, "-ts", "2", "-mat_law", "micro_nl", "-micro_n", "24", "-micro_type", "0",
                          "-micro_mat_1", "1e7,0.25,%.3e,1e8" % Sy, "-micro_mat_2", "1e8,0.3,1e9,1e7",
                          "-micro_nl_solver", "grid"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert "Micro cell : type = 0 (sphere)\tn = 24\tmem = lds\tnl_solver = grid" in lines
    counts = [int(l.split(":")[1].split()[0]) for l in lines if l.startswith("Non-Linear Gauss points : ")]
    assert counts and max(counts) > 0, out.stdout
    assert "has no effect" not in out.stderr and "Elapsed time" in out.stdout
