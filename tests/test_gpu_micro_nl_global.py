"""Options micro_nl_start / micro_nl_ls: the globalised Newton loop of -mat_law micro_nl.

micro_nl_start 1: after the first state pass at the zero interior (D and the first norm as under 0)
the interior takes the elastic predictor sum_l eps_l w_l and the state is evaluated there.
micro_nl_ls K: after a step's CG the lengths 2^-j, j = 0 .. K, are tried in turn; trial j is accepted
when |D^-1 R| is smaller than at the last accepted iterate, trial K regardless.

The reference (solve_global) extends test_gpu_micro_nl.CellRef.solve by exactly these two rules,
with dense direct solves and a stop at 1e-13.  The bars are the project's:
    max|x_gpu - x_ref| <= 100 kappa micro_nl_rtol max|x_ref|      (x = sigma, C)
and, for a cell of equal phases (the J2 law itself), test_gpu_micro_nl_grid's against -mat_law plastic.

The soft matrix (1e7, 0.25, 1e4, 1e6) (hardening E / 10) is the one plain Newton from a zero interior
gives up on; the first test pins that and fails without the options.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import macroc_amd as M
import test_gpu_micro_nl as TN
import test_gpu_micro_nl_grid as TG

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NL_RTOL, MAX_IT = TN.NL_RTOL, 20  # the defaults of micro_nl_rtol and micro_nl_max_it
SOFT = (1.0e7, 0.25, 1.0e4, 1.0e6)
SOFT_FLAGS = ("-micro_mat_1", "%r,%r,%r,%r" % SOFT, "-micro_mat_2", "%r,%r,%r,%r" % SOFT)
MODES = {"ls": dict(micro_nl_ls=5), "start": dict(micro_nl_start=1), "both": dict(micro_nl_start=1, micro_nl_ls=5)}
SOLVERS = {"lds": dict(micro_nl_solver=0, micro_mem=0), "mem": dict(micro_nl_solver=0, micro_mem=1),
           "grid": dict(micro_nl_solver=1)}
GIVE_UP = r"micro cells did not converge; worst: Gauss point \d+ \(Newton gave up\): 20 Newton iterations"


def ctx(argv, solver, **opts):
    m = M.Macroc(argv)
    for k, v in {**SOLVERS[solver], **opts}.items():
        m.set_option(k, v)
    return m


def stages_of(m, u1, stages):
    out = []
    for fac in stages:
        m.set_u(fac * u1)
        m.set_strains()
        m.homogenize()
        out.append(dict(eps=m.gp_strain(), sig=m.stress().reshape(-1, 6), C=m.gp_ctan(), info=m.micro_nl_info(),
                        steps=m.micro_nl_steps(), stats=m.nonlinear_stats()))
        m.update_vars()
    return out


# ---------------------------------------------------------------- the extended reference
def unit_fields(ref):
    """the six elastic unit-strain fields w_l [ndof][6] (what the law keeps for its linear test)"""
    if not hasattr(ref, "W"):
        Ct = ref.j2(np.zeros((ref.nel, 8, 6)), ref.zero_hist)[4]
        ref.W = ref.tangent(Ct)[1]
    return ref.W


def solve_global(ref, eps, hold, start, ls, rtol=1e-13, max_it=40, kappa=True):
    """CellRef.solve with the two rules.  its = the linear solves, passes = the state evaluations,
    rejects / min_step as mcx_micro_nl_get_steps reports them; status 1 = gave up after max_it."""
    fr = ~ref.bd
    u = ref.boundary_field(eps)
    passes = 0

    def state(u):
        s, hn, f, sn, Ct = ref.j2(ref.strains(u), hold)
        R = np.zeros(len(u))
        np.add.at(R, ref.edof, np.einsum("gki,egk->ei", ref.B, s) * ref.detJ)
        return s, hn, f, sn, Ct, R

    s, hn, f, sn, Ct, R = state(u)
    passes += 1
    D = np.diag(ref.stiffness(Ct)[np.ix_(fr, fr)]).copy()
    n0 = np.linalg.norm(R[fr] / D)
    if start and n0 != 0.0:
        W = unit_fields(ref)
        pred = np.zeros(len(u))
        for l in range(6):  # ascending l
            pred += eps[l] * W[:, l]
        u[fr] = pred[fr]
        s, hn, f, sn, Ct, R = state(u)
        passes += 1
    its, rejects, min_step, status = 0, 0, 1.0, 0
    while True:
        nacc = np.linalg.norm(R[fr] / D)
        if n0 == 0.0 or nacc <= rtol * n0:
            break
        if its >= max_it:
            status = 1
            break
        dx = np.linalg.solve(ref.stiffness(Ct)[np.ix_(fr, fr)], -R[fr])
        its += 1
        lam = 1.0
        u[fr] += dx
        for j in range(ls + 1):
            s, hn, f, sn, Ct, R = state(u)
            passes += 1
            if ls == 0 or np.linalg.norm(R[fr] / D) < nacc or j == ls:
                break
            rejects += 1
            lam *= 0.5
            u[fr] -= lam * dx
        if ls > 0:
            min_step = min(min_step, lam)
    out = dict(sig=s.sum((0, 1)) * ref.detJ, h=hn, its=its, passes=passes, rejects=rejects, min_step=min_step,
               status=status, fmax=f.max(), margin=(np.abs(f) / ref.Sy).min(), strial=sn.max(), mlin=np.inf,
               rel=nacc / n0 if n0 else 0.0)
    if status == 0:
        Cm, _, Kii = ref.tangent(Ct)
        out["C"] = Cm
        if kappa:
            d = np.sqrt(np.diag(Kii))
            w = np.linalg.eigvalsh(Kii / np.outer(d, d))
            out["kappa"] = w[-1] / w[0]
    return out


def plastic_bar(n):
    return 100 * TG.scaled_kappa(n, (SOFT[:2], SOFT[:2])) * NL_RTOL  # test_equal_phases_are_the_plastic_law's


# ---------------------------------------------------------------- 1. fails without the feature
@functools.lru_cache(maxsize=None)
def plastic_law():
    u1 = TN.field((2, 2, 2), 5, 4e-3, wobble=0)
    with M.Macroc(TN.nl_argv(1, 2, law="plastic", extra=SOFT_FLAGS)) as m:
        return TG.stages_of(m, u1, (1.0, 0.5), nl=False)


@pytest.mark.parametrize("solver", list(SOLVERS))
def test_soft_equal_phases_need_the_options(solver):
    """layer cell n = 6 of equal soft phases, all eight points at e0 of load (5, 4e-3), a commit, then
    0.5 e0: plain Newton gives up on the unload with today's message; under ls 5, start 1 and both
    it converges to the J2 law (sigma, C, f_trial of -mat_law plastic at the same strains)."""
    n, u1 = 6, TN.field((2, 2, 2), 5, 4e-3, wobble=0)
    a, bar = plastic_law(), plastic_bar(6)
    with ctx(TN.nl_argv(1, n, extra=SOFT_FLAGS), solver) as m:
        first = stages_of(m, u1, (1.0,))[0]
        assert first["info"]["path"].all() and (first["steps"]["ls_rejects"] == 0).all()
        assert (first["steps"]["min_step"] == 1.0).all()  # solved, never backtracked
        m.set_u(0.5 * u1)
        m.set_strains()
        with pytest.raises(M.MacrocError, match=GIVE_UP) as err:
            m.homogenize()
        assert "micro_nl_start" not in str(err.value) and "micro_nl_ls" not in str(err.value)
    for mode, opts in MODES.items():
        with ctx(TN.nl_argv(1, n, extra=SOFT_FLAGS), solver, **opts) as m:
            b = stages_of(m, u1, (1.0, 0.5))
        backtracked = False
        for st, (x, y) in enumerate(zip(a, b)):
            smax = np.abs(x["sig"]).max()
            es = np.abs(x["sig"] - y["sig"]).max() / smax
            ec = np.abs(x["C"] - y["C"]).max() / np.abs(x["C"]).max()
            ef = abs(x["stats"][1] - y["stats"][1]) / smax
            print(f"soft equal phases n {n} {solver} {mode} stage {st}: err sigma {es:.2e} C {ec:.2e} f {ef:.2e} bar "
                  f"{bar:.2e} newton {y['info']['newton_its']} cg {y['info']['cg_its']} rejects "
                  f"{y['steps']['ls_rejects']} min step {y['steps']['min_step']} rnorm {y['info']['rnorm'].max():.1e}")
            assert np.array_equal(x["eps"], y["eps"])
            assert es <= bar and ec <= bar and ef <= bar
            assert x["stats"][0] == y["stats"][0]
            assert y["info"]["path"].all() and (y["info"]["rnorm"] <= NL_RTOL).all()
            assert (y["info"]["newton_its"] <= MAX_IT).all()
            if "micro_nl_start" in opts:  # the affine field solves a cell of equal phases
                assert not y["info"]["newton_its"].any()
                assert (y["steps"]["ls_rejects"] == 0).all() and (y["steps"]["min_step"] == 1.0).all()
            backtracked = backtracked or ((y["steps"]["ls_rejects"] > 0) & (y["steps"]["min_step"] < 1.0)).any()
        if mode == "ls":
            assert backtracked


def test_unconverged_message_names_the_options():
    n, u1 = 6, TN.field((2, 2, 2), 5, 4e-3, wobble=0)
    with ctx(TN.nl_argv(1, n, extra=SOFT_FLAGS), "lds", micro_nl_ls=5, micro_nl_max_it=1) as m:
        m.set_u(u1)
        m.set_strains()
        with pytest.raises(M.MacrocError, match=r"1 Newton iterations \(micro_nl_max_it 1\).*"
                                                r"\(micro_nl_start 0, micro_nl_ls 5: \d+ rejected trials"):
            m.homogenize()


# ---------------------------------------------------------------- 2. a heterogeneous cell
SPHERE_N = 12


@functools.lru_cache(maxsize=None)
def sphere_reference():
    """the one strain of the 2x2x2 grid (wobble 0) through e0 -> commit -> 1.25 e0: stage 1 once (both
    rules), stage 2 from its history under each mode; kappa once per stage."""
    ref = TN.cell(0, SPHERE_N)
    rng = np.random.default_rng(5)
    e0 = 4e-3 * rng.uniform(-1, 1, 6)
    r1 = solve_global(ref, e0, ref.zero_hist, 1, 5)
    r1["mlin"] = ref.linear_f(e0)[1]
    r2 = {mode: solve_global(ref, 1.25 * e0, r1["h"], o.get("micro_nl_start", 0), o.get("micro_nl_ls", 0),
                             kappa=mode == "both") for mode, o in MODES.items()}
    for r in r2.values():
        r["kappa"] = r2["both"]["kappa"]
    return e0, r1, r2


@pytest.mark.slow
@pytest.mark.parametrize("solver", ["mem", "grid"])
def test_sphere_cell_against_the_extended_reference(solver):
    n, u1 = SPHERE_N, TN.field((2, 2, 2), 5, 4e-3, wobble=0)
    e0, r1, r2 = sphere_reference()
    with ctx(TN.nl_argv(0, n), solver) as m:
        stages_of(m, u1, (1.0,))
        m.set_u(1.25 * u1)
        m.set_strains()
        with pytest.raises(M.MacrocError, match=GIVE_UP):
            m.homogenize()
    its = {}
    for mode, opts in MODES.items():
        with ctx(TN.nl_argv(0, n), solver, **opts) as m:
            b = stages_of(m, u1, (1.0, 1.25))
        for st, (y, r) in enumerate(zip(b, (r1, r2[mode]))):
            TN.check_conditions(r)
            assert r["status"] == 0
            bar = 100 * r["kappa"] * NL_RTOL
            assert np.abs(y["eps"] - (1.0, 1.25)[st] * e0).max() <= 1e-15
            es = np.abs(y["sig"] - r["sig"]).max() / np.abs(r["sig"]).max()
            ec = np.abs(y["C"] - r["C"]).max() / np.abs(r["C"]).max()
            print(f"sphere n {n} {solver} {mode} stage {st}: kappa {r['kappa']:.1f} err sigma {es:.2e} C {ec:.2e} bar "
                  f"{bar:.2e} newton gpu {y['info']['newton_its']} ref {r['its']} rejects gpu {y['steps']['ls_rejects']} "
                  f"ref {r['rejects']} cg {y['info']['cg_its']} rnorm {y['info']['rnorm'].max():.1e}")
            assert es <= bar and ec <= bar
            assert y["info"]["path"].all() and (y["info"]["rnorm"] <= NL_RTOL).all()
            assert (y["info"]["newton_its"] <= MAX_IT).all()
        its[mode] = b[1]["info"]["newton_its"]
    assert (its["start"] <= its["ls"]).all()  # the predictor needs no more CG-solved steps than ls alone


# ---------------------------------------------------------------- 3. where plain Newton converges
@pytest.mark.parametrize("solver", ["lds", "grid"])
@pytest.mark.parametrize("typ,n", [(0, 5), (1, 4)])
def test_options_change_only_the_path(typ, n, solver):
    ref = TN.cell(typ, n)
    u1 = TN.field((2, 2, 2), 5, 4e-3)
    with ctx(TN.nl_argv(typ, n), solver) as m:
        base = stages_of(m, u1, TN.STAGES)
    pts, hold = [], [None] * 8
    for st in base:
        rs = [ref.point(st["eps"][q], hold[q]) for q in range(8)]
        for q, r in enumerate(rs):
            TN.check_conditions(r)
            if r["path"]:
                hold[q] = r["h"]
        pts.append(rs)
    for mode, opts in MODES.items():
        with ctx(TN.nl_argv(typ, n), solver, **opts) as m:
            b = stages_of(m, u1, TN.STAGES)
        same_path = mode == "ls"
        for st, (x, y, rs) in enumerate(zip(base, b, pts)):
            assert np.array_equal(x["eps"], y["eps"])
            for q, r in enumerate(rs):
                bar = 100 * r["kappa"] * NL_RTOL
                assert y["info"]["path"][q] == r["path"]
                assert np.abs(y["sig"][q] - r["sig"]).max() <= bar * np.abs(r["sig"]).max()
                assert np.abs(y["C"][q] - r["C"]).max() <= bar * np.abs(r["C"]).max()
            assert (y["info"]["rnorm"] <= NL_RTOL).all() and (y["info"]["newton_its"] <= MAX_IT).all()
            print(f"cell ({typ},{n}) {solver} {mode} stage {st}: newton {y['info']['newton_its']} (defaults "
                  f"{x['info']['newton_its']}) rejects {y['steps']['ls_rejects']}")
            # ls alone: the first trial is the full step, so without a reject the path is the defaults'
            same_path = same_path and not y["steps"]["ls_rejects"].any()
            if same_path:
                for k in ("sig", "C"):
                    assert np.array_equal(x[k], y[k])
                for k in ("newton_its", "cg_its", "rnorm"):
                    assert np.array_equal(x["info"][k], y["info"][k])


# ---------------------------------------------------------------- 4. determinism
DET_CASES = {"soft-ls": (1, 6, SOFT_FLAGS, 0.0, (1.0, 0.5), MODES["ls"]),
             "sphere-both": (0, 5, (), 0.15, TN.STAGES, MODES["both"])}


def det_run(case, solver, **more):
    typ, n, flags, wobble, stages, opts = DET_CASES[case]
    with ctx(TN.nl_argv(typ, n, extra=flags), solver, **opts, **more) as m:
        return [(s["eps"], s["sig"], s["C"], s["info"]["newton_its"], s["info"]["cg_its"], s["info"]["rnorm"],
                 s["steps"]["ls_rejects"], s["steps"]["min_step"])
                for s in stages_of(m, TN.field((2, 2, 2), 5, 4e-3, wobble=wobble), stages)]


@functools.lru_cache(maxsize=None)
def det_base(case, solver):
    return det_run(case, solver)


def same_bits(a, b):
    for x, y in zip(a, b):
        for p, q in zip(x, y):
            assert np.array_equal(p, q)


@pytest.mark.parametrize("solver", list(SOLVERS))
@pytest.mark.parametrize("case", list(DET_CASES))
def test_two_runs_are_bitwise_equal(case, solver):
    same_bits(det_base(case, solver), det_run(case, solver))


@pytest.mark.parametrize("more", [dict(micro_grid_poll=1), dict(micro_grid_poll=7), dict(micro_grid_poll=16),
                                  dict(micro_mem_blocks=64), dict(micro_mem_blocks=3)],
                         ids=["poll1", "poll7", "poll16", "batch64", "batch3"])
@pytest.mark.parametrize("case", list(DET_CASES))
def test_grid_bits_do_not_depend_on_poll_or_batch(case, more):
    same_bits(det_base(case, "grid"), det_run(case, "grid", **more))


@pytest.mark.parametrize("case", list(DET_CASES))
def test_solvers_agree(case):
    typ, n, flags = DET_CASES[case][:3]
    kappa = TG.scaled_kappa(n, (SOFT[:2], SOFT[:2])) if flags else TG.scaled_kappa(n)
    bar = 2 * 100 * kappa * NL_RTOL  # the sum of the two solvers' bars, as test_against_solver_0 takes them
    for x, y in zip(det_base(case, "lds"), det_base(case, "grid")):
        assert np.array_equal(x[0], y[0])
        assert np.abs(x[1] - y[1]).max() <= bar * np.abs(x[1]).max()
        assert np.abs(x[2] - y[2]).max() <= bar * np.abs(x[2]).max()
        assert np.array_equal(x[3], y[3]) and np.array_equal(x[6], y[6])  # newton_its, ls_rejects
        assert np.array_equal(x[7], y[7])


# ---------------------------------------------------------------- 5. below yield
@pytest.mark.parametrize("solver", ["lds", "grid"])
def test_below_yield_is_the_linear_law_bit_for_bit(solver):
    grid = (5, 4, 3)
    u = TN.field(grid, 11, 2e-5)
    with ctx(TN.nl_argv(1, 4, grid), solver, **MODES["both"]) as a:
        ba, va = TN.assemble(a, u)
        sa, info, steps = a.stress(), a.micro_nl_info(), a.micro_nl_steps()
        assert not info["path"].any() and info["slots"] == 0 and info["slots_used"] == 0  # no pool
        assert not steps["ls_rejects"].any() and not steps["min_step"].any()  # linear shortcut: (0, 0.0)
    extra = ("-micro_solver", "grid") if solver == "grid" else ()
    with M.Macroc(TN.nl_argv(1, 4, grid, law="micro", extra=extra)) as b:
        bb, vb = TN.assemble(b, u)
        sb = b.stress()
    assert np.linalg.norm(bb) > 0
    assert np.array_equal(sa, sb) and np.array_equal(ba, bb) and np.array_equal(va, vb)


# ---------------------------------------------------------------- 6. the options' values
def test_option_values_are_checked_and_other_laws_accept_them():
    with M.Macroc(TN.nl_argv(1, 4)) as m:
        for name, bad in (("micro_nl_start", 2), ("micro_nl_start", -1), ("micro_nl_start", 0.5), ("micro_nl_ls", 17),
                          ("micro_nl_ls", -1), ("micro_nl_ls", 2.5)):
            with pytest.raises(M.MacrocError, match=name + ": "):
                m.set_option(name, bad)
        u1 = TN.field((2, 2, 2), 5, 4e-3)
        _, sig, Cg, _ = TN.evaluate(m, u1)  # (no commit: the second evaluation starts from the same history)
        m.set_option("micro_nl_ls", 16)  # both may change at any time, slots in use or not
        m.set_option("micro_nl_start", 1)
        m.set_option("micro_nl_ls", 0)
        m.set_option("micro_nl_start", 0)
        _, sig2, Cg2, _ = TN.evaluate(m, u1)  # the refused values and the round trip left the defaults
        assert np.array_equal(sig, sig2) and np.array_equal(Cg, Cg2)
    with M.Macroc(TN.nl_argv(1, 2, extra=("-micro_nl_start", "elastic", "-micro_nl_ls", 5))) as m:  # n = 2: no interior
        a = stages_of(m, TN.field((2, 2, 2), 5, 4e-3), (1.0,))[0]
    with M.Macroc(TN.nl_argv(1, 2)) as m:
        b = stages_of(m, TN.field((2, 2, 2), 5, 4e-3), (1.0,))[0]
    assert np.array_equal(a["sig"], b["sig"]) and np.array_equal(a["C"], b["C"]) and not a["info"]["newton_its"].any()
    for law in ("micro", "plastic", "elastic"):
        with M.Macroc(TN.nl_argv(1, 4, law=law, extra=("-micro_nl_start", "elastic", "-micro_nl_ls", 5))) as m:
            m.set_option("micro_nl_start", 1)
            m.set_option("micro_nl_ls", 5)
            with pytest.raises(M.MacrocError, match="without -mat_law micro_nl"):
                m.micro_nl_steps()


# ---------------------------------------------------------------- 7. the driver
def driver_argv():
    """4^3 nodes, micro_n 6, the soft matrix (hardening 1e6) with Sy from the load of time step 1 so that a
    few points yield (test_gpu_micro_nl_grid's driver test takes hardening 1e8 for plain Newton's sake)"""
    grid = ("-da_grid_x", "4", "-da_grid_y", "4", "-da_grid_z", "4")
    with M.Macroc(list(grid) + ["-mat_law", "elastic"]) as m:
        for ts in (0, 1):
            m.apply_bc_on_u(m.get_displacement(ts))
        m.set_strains()
        eps = m.gp_strain()
    tr = eps[:, :3].sum(1)
    dev = np.concatenate([eps[:, :3] - tr[:, None] / 3, eps[:, 3:] / 2], axis=1)
    dn = np.sqrt((dev[:, :3] ** 2).sum(1) + 2 * (dev[:, 3:] ** 2).sum(1))
    Sy = np.sqrt(1.5) * 2 * 1e7 / (2 * 1.25) * np.quantile(dn[dn > 0], 0.9)
    return [os.path.join(ROOT, "macroc_amd", "driver", "macroc_amd"), *grid, "-ts", "2", "-mat_law", "micro_nl",
            "-micro_n", "6", "-micro_type", "0", "-micro_mat_1", "1e7,0.25,%.3e,1e6" % Sy,
            "-micro_mat_2", "1e8,0.3,1e9,1e7"]


def test_driver_takes_the_flags(tmp_path):
    """the driver's time loop runs to its end with both flags (DESIGN §19 records the same command
    without them)."""
    out = subprocess.run(driver_argv() + ["-micro_nl_start", "elastic", "-micro_nl_ls", "5"], cwd=tmp_path,
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "options you set that were not used" not in out.stderr
    counts = [int(l.split(":")[1].split()[0]) for l in out.stdout.splitlines() if l.startswith("Non-Linear Gauss points : ")]
    assert counts and max(counts) > 0, out.stdout
    assert "Elapsed time" in out.stdout
