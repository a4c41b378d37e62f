"""The CG's stop reasons: a table of inputs that end KSPSolve_CG for every reason the Jacobi path can
reach, and a numpy restatement of KSPSolve_CG + KSPConvergedDefault that also reports p.Ap and z.r.

A plain helper module (no fixtures): tests/test_ksp_stops_cpu.py proves every row against the CPU
oracle and the restatement, tests/test_gpu_ksp_stops.py runs the rows on the device CG's paths.

Every case is time step 0 then 1 at -ksp_rtol 1e-12, E = 1e7.  The rows:
  indef   DIVERGED_INDEFINITE_MAT (-10): a Poisson ratio outside (-1, 0.5); p.Ap changes sign at
          iteration i = its - 1.  The (grid, nu) -> its table below is literal.
  dtol    DIVERGED_DTOL (-4): -bc_type 0, nu = 0.4999, whose preconditioned residual norm rises for
          several iterations; -ksp_divtol = sqrt(r[k-1] r[k]) of the oracle's own history (r = h / h[0])
          stops at its = k.  dtol0: -ksp_divtol 1.0 / 0.5 on the default problem stop at iteration 0.
  atol    CONVERGED_ATOL (3): the default problem, -ksp_atol = sqrt(h[k-1] h[k]) stops at its = k;
          with -ksp_max_it k, k + 1 (converged at the last allowed iteration wins) and k - 1 (-3).
  nan     DIVERGED_NANORINF (-9): one interior dof of u overwritten before set_strains.
The margins (GAP, PAP_MARGIN) are what let a solver that sums its dot products in another order be
held to the exact iteration count.
"""
import functools
from collections import namedtuple

import numpy as np
import scipy.sparse as sp

from oracle import oracle as O

RTOL = 1e-12
E = 1e7
GAP = 1.05          # neighbouring history entries around an -ksp_atol / -ksp_divtol threshold differ by >= 5 %
PAP_MARGIN = 1e-3   # |p.Ap| >= PAP_MARGIN * sum |p_j| |(Ap)_j| at the stopping iteration and the one before
REASONS = {"rtol": 2, "atol": 3, "its": -3, "dtol": -4, "pc": -8, "nan": -9, "indef": -10}

GRIDS = {"g8": (8, 8, 8), "g20": (20, 12, 10), "g70": (70, 20, 12), "g12": (12, 10, 14)}

# DIVERGED_INDEFINITE_MAT: nu -> its (i = its - 1 covers 0..3 mod 4 below and above 4 on every grid)
INDEF = {
    "g8": {0.75: 2, 1.5: 3, 2.0: 4, 3.0: 5, -2.0: 7, -1.5: 8, -1.2: 13},
    "g20": {0.75: 2, 1.5: 3, 2.0: 4, 3.0: 6, -2.0: 11, -1.5: 13, -1.2: 24},
    "g70": {0.75: 2, 1.5: 4, 2.0: 5, 3.0: 8, -2.0: 13, -1.5: 16, -1.2: 39},
}
INDEF_NUS = (0.75, 1.5, 2.0, 3.0, -2.0, -1.5, -1.2)
DTOL_NU = 0.4999
DTOL_K = {"g8": range(1, 8), "g20": range(1, 7), "g70": range(1, 6), "g12": (2, 5)}
ATOL_K = {"g8": range(1, 7), "g20": range(1, 7), "g70": range(1, 7), "g12": (3,)}
POISON = {"nan": float("nan"), "inf": float("inf"), "big": 1e300}

# kind: the row's family; kw: O.Problem's keywords beyond the grid; poison: None or a POISON key;
# its / reason: what the oracle gives; k: the history index the threshold sits below (atol, dtol)
Case = namedtuple("Case", "id grid kind kw poison its reason k")


def norms_computed(its, reason):
    """Residual norms one solve computes = the length of its history: entry 0 and one per completed
    iteration; an INDEFINITE_MAT stop leaves its last iteration before the norm."""
    return its if reason == REASONS["indef"] else its + 1


def poison_dof(grid):
    """An interior dof (natural numbering): x component of the centre node."""
    NX, NY, NZ = GRIDS[grid]
    return 3 * (NX // 2 + NX * (NY // 2 + NY * (NZ // 2)))


def problem(grid, **kw):
    NX, NY, NZ = GRIDS[grid]
    return O.Problem(NX, NY, NZ, rtol=RTOL, E=E, **kw)


def prepare(P, poison=None, grid=None):
    """Time step 0 then 1 up to the assembled system (src/main.c:49-70)."""
    for ts in (0, 1):
        P.apply_bc_u(P.get_displacement(ts))
    if poison is not None:
        u = P.u()
        u[poison_dof(grid)] = POISON[poison]
        P.set_u(u)
    P.set_strains()
    P.homogenize()
    P.assembly_res()
    P.assembly_jac()
    return P


@functools.lru_cache(maxsize=None)
def base_history(grid, bc_type, nu):
    """The first 11 norms of the problem without -ksp_atol / -ksp_divtol (-ksp_max_it 10)."""
    P = prepare(problem(grid, bc_type=bc_type, nu=nu, maxits=10))
    h = P.solve(history=True)["history"]
    P.close()
    assert len(h) == 11
    return h


def dtol_threshold(grid, k):
    h = base_history(grid, O.BC_BENDING, DTOL_NU)
    r = h / h[0]
    return float(np.sqrt(r[k - 1] * r[k]))


def atol_threshold(grid, k):
    h = base_history(grid, O.BC_CIRCLE, 0.25)
    return float(np.sqrt(h[k - 1] * h[k]))


@functools.lru_cache(maxsize=None)
def derived_indef(grid, nu):
    """its of (grid, nu) for a grid without a literal INDEF row, by the rule of the literal ones: the
    oracle's count where it stops for INDEFINITE_MAT and the restatement's p.Ap margin holds, else None."""
    P = prepare(problem(grid, nu=nu))
    o = P.solve()
    c = restated(P)
    P.close()
    i = o["its"] - 1
    if (o["reason"] == REASONS["indef"] and (c["its"], c["reason"]) == (o["its"], o["reason"])
            and min(c["pap_margin"][i - 1:i + 1]) >= PAP_MARGIN):
        return o["its"]
    return None


def indef_its(grid, nu):
    return INDEF[grid][nu] if grid in INDEF else derived_indef(grid, nu)


def indef_case(grid, nu):
    its = indef_its(grid, nu)
    return Case(f"indef-{grid}-nu{nu}", grid, "indef", dict(nu=nu), None, its, REASONS["indef"], None)


def dtol_case(grid, k):
    kw = dict(nu=DTOL_NU, bc_type=O.BC_BENDING, dtol=dtol_threshold(grid, k))
    return Case(f"dtol-{grid}-k{k}", grid, "dtol", kw, None, k, REASONS["dtol"], k)


def dtol0_case(grid, dtol):
    return Case(f"dtol0-{grid}-{dtol}", grid, "dtol0", dict(dtol=dtol), None, 0, REASONS["dtol"], None)


def atol_case(grid, k, dmax=None):
    """dmax: -ksp_max_it = k + dmax."""
    kw = dict(abstol=atol_threshold(grid, k))
    if dmax is None:
        return Case(f"atol-{grid}-k{k}", grid, "atol", kw, None, k, REASONS["atol"], k)
    kw["maxits"] = k + dmax
    its, reason = (k, REASONS["atol"]) if dmax >= 0 else (k - 1, REASONS["its"])
    return Case(f"atol-{grid}-k{k}-max{k + dmax}", grid, "atol_max", kw, None, its, reason, k)


def nan_case(grid, poison):
    return Case(f"nan-{grid}-{poison}", grid, "nan", {}, poison, 0, REASONS["nan"], None)


def cases_for(grid):
    """Every row of a literal grid."""
    out = [indef_case(grid, nu) for nu in INDEF[grid]]
    out += [dtol_case(grid, k) for k in DTOL_K[grid]]
    out += [atol_case(grid, k) for k in ATOL_K[grid]]
    if grid == "g8":
        out += [dtol0_case(grid, d) for d in (1.0, 0.5)]
        out += [atol_case(grid, k, d) for k in (3, 4) for d in (0, 1, -1)]
        out += [nan_case(grid, p) for p in POISON]
    return out


def decomposed_cases(grid):
    """The rows of the decomposed runs: two INDEFINITE_MAT rows whose i differ mod 4, DTOL at k = 2 and
    5, ATOL at k = 3, the NaN row."""
    first = next(nu for nu in INDEF_NUS if indef_its(grid, nu) is not None)  # the earliest stop
    # and the latest one with another residue: beyond one turn of the four p buffers
    second = next(nu for nu in reversed(INDEF_NUS) if indef_its(grid, nu) is not None
                  and indef_its(grid, nu) > 4 and (indef_its(grid, nu) - indef_its(grid, first)) % 4)
    return ([indef_case(grid, first), indef_case(grid, second), dtol_case(grid, 2), dtol_case(grid, 5),
             atol_case(grid, 3), nan_case(grid, "nan")])


ALL_GRIDS_CASES = [c for g in ("g8", "g20", "g70") for c in cases_for(g)]


def oracle_case(case):
    """(P, out): the oracle's prepared problem of a row and its solve (history included)."""
    P = prepare(problem(case.grid, **case.kw), case.poison, case.grid)
    out = P.solve(history=True)
    out["history"] = out["history"][:norms_computed(out["its"], out["reason"])]
    return P, out


def matrix(P):
    rp, ci = P.csr()
    return sp.csr_matrix((P.A_values(), ci, rp), shape=(P.ndofs, P.ndofs))


def converged_default(rn, ttol, abstol, dtol, rn0):
    """KSPConvergedDefault."""
    if np.isnan(rn) or np.isinf(rn):
        return REASONS["nan"]
    if rn <= ttol:
        return REASONS["atol"] if rn < abstol else REASONS["rtol"]
    if rn >= dtol * rn0:
        return REASONS["dtol"]
    return 0


def cg_petsc(A, b, **kw):
    """_cg_petsc with floating-point warnings off: the NaN / Inf rows overflow on purpose."""
    with np.errstate(over="ignore", invalid="ignore"):
        return _cg_petsc(A, b, **kw)


def _cg_petsc(A, b, rtol=1e-5, abstol=1e-50, dtol=1e4, maxits=10000, pc=None, norm="preconditioned"):
    """KSPSolve_CG, zero initial guess (numpy restatement; tests/golden/make_golden.py:cg_petsc with
    every reason and the scalars of each iteration).  pc: z = pc(r), default PCJacobi of A.
    norm "preconditioned": |z| (KSP_NORM_PRECONDITIONED); "natural": sqrt(r.z).
    Returns x, its, reason, rnorm, history, pap [p.Ap per iteration], pap_margin
    [|p.Ap| / sum |p_j| |(Ap)_j|], zr [z.r: entry 0 and one per completed iteration]."""
    if pc is None:
        d = A.diagonal()
        dinv = np.where(d != 0, 1.0 / np.where(d != 0, d, 1.0), 1.0)
        pc = lambda r: r * dinv  # noqa: E731
    natural = norm == "natural"
    x = np.zeros_like(b)
    r = b.copy()
    z = pc(r)
    out = dict(history=[], pap=[], pap_margin=[], zr=[])

    def done(its, reason, rn):
        out.update(x=x, its=its, reason=reason, rnorm=rn, history=np.array(out["history"]))
        return out

    beta = float(z @ r)
    out["zr"].append(beta)
    if natural and beta < 0:
        return done(0, REASONS["pc"], float("nan"))
    dp = float(np.sqrt(beta)) if natural else float(np.linalg.norm(z))
    out["history"].append(dp)
    ttol, rn0 = max(rtol * dp, abstol), dp
    reason = converged_default(dp, ttol, abstol, dtol, rn0)
    if reason:
        return done(0, reason, dp)
    i, its, p, dpi, betaold = 0, 0, None, 0.0, 0.0
    while True:
        its = i + 1
        if beta == 0.0:
            return done(its, REASONS["atol"], dp)
        if i > 0 and beta * betaold < 0.0:
            return done(its, REASONS["pc"], dp)
        p = z.copy() if i == 0 else z + (beta / betaold) * p
        dpiold = dpi
        w = A @ p
        dpi = float(p @ w)
        out["pap"].append(dpi)
        s = float(np.abs(p) @ np.abs(w))
        out["pap_margin"].append(abs(dpi) / s if s > 0 else 0.0)
        betaold = beta
        if dpi == 0.0 or (i > 0 and dpi * dpiold <= 0.0):
            return done(its, REASONS["indef"], dp)
        a = beta / dpi
        x = x + a * p
        r = r - a * w
        z = pc(r)
        beta = float(z @ r)
        out["zr"].append(beta)
        if natural and beta < 0:
            return done(its, REASONS["pc"], dp)
        dp = float(np.sqrt(beta)) if natural else float(np.linalg.norm(z))
        out["history"].append(dp)
        reason = converged_default(dp, ttol, abstol, dtol, rn0)
        if reason:
            return done(its, reason, dp)
        i += 1
        if i >= maxits:
            return done(its, REASONS["its"], dp)


def restated(P):
    """cg_petsc on the oracle's assembled system with the oracle's tolerances."""
    o = P.opts
    return cg_petsc(matrix(P), P.b(), rtol=o.rtol, abstol=o.abstol, dtol=o.dtol, maxits=o.maxits)


def same_rnorm(a, b, rel=1e-9):
    """rnorm agreement: NaN / Inf by kind, else to `rel` relative."""
    if np.isnan(b):
        return bool(np.isnan(a))
    if np.isinf(b):
        return bool(np.isinf(a)) and (a > 0) == (b > 0)
    return abs(a - b) <= rel * abs(b)
