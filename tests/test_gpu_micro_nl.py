"""-mat_law micro_nl: the two-phase micro cell with J2-plastic phases, solved per macro Gauss point
(DESIGN §12).

The reference (CellRef) restates the definition in numpy, independently of the kernels: the unit
cube of n^3 nodes / (n-1)^3 Q1 hexahedra (2x2x2 Gauss, physical B), phases by the integer rule, the
small-strain J2 law with linear isotropic hardening at every micro Gauss point, a dense K_T, plain
Newton with np.linalg.solve to 1e-13, the consistent tangent by the six frozen-K_T solves.  It is
fed the strains the GPU reports.  Its kappa, the condition number of the Jacobi-scaled converged
K_T,ii, sets the bar of every comparison:
    max|x_gpu - x_ref| <= 100 kappa micro_nl_rtol max|x_ref|      (x = sigma, C)
Every use of the reference asserts the conditions under which it is a fair judge: every micro
point's |f| >= 1e-6 Sy at the converged state, the linear test's f_max that far from 0, Newton in
at most 10 iterations.

The micro histories have no getter; their determinism is checked through the next load stage,
whose results depend on them.
"""
import functools
import os
import subprocess
import threading
import time

import numpy as np
import pytest

import macroc_amd as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MAT1, MAT2 = (1.0e7, 0.25, 1.0e4, 1.0e6), (1.0e8, 0.3, 1.0e9, 1.0e7)
NL_RTOL = 1e-10  # micro_nl_rtol's default
CELLS = [(1, 3), (0, 4), (1, 4), (0, 5), (1, 5)]
LOADS = [(5, 4e-3), (7, 2e-3)]
STAGES = (1.0, 1.5, 0.5)
MARGIN = 1e-6  # |f| >= MARGIN * Sy


def phase_rule(typ, n):
    """[k][j][i] material of element (i, j, k), exact integer arithmetic."""
    ne = n - 1
    k, j, i = np.meshgrid(np.arange(ne), np.arange(ne), np.arange(ne), indexing="ij")
    if typ == 0:
        return ((2 * i + 1 - ne) ** 2 + (2 * j + 1 - ne) ** 2 + (2 * k + 1 - ne) ** 2 < ne * ne).astype(np.uint8)
    return (2 * j + 1 < ne).astype(np.uint8)


def element_B(h):
    """B[gp][6][24] (Voigt xx, yy, zz, xy, xz, yz; engineering shear) of the brick element of edges
    h = (hx, hy, hz), local node a at offsets (a & 1, a >> 1 & 1, a >> 2), and det J."""
    g = 1.0 / np.sqrt(3.0)
    B = np.zeros((8, 6, 24))
    for gp in range(8):
        xi = [g if (gp >> q) & 1 else -g for q in range(3)]
        for a in range(8):
            sa = [1.0 if (a >> q) & 1 else -1.0 for q in range(3)]
            dN = [0.125 * sa[d] * np.prod([1.0 + sa[q] * xi[q] for q in range(3) if q != d]) * (2.0 / h[d])
                  for d in range(3)]
            B[gp, 0, 3 * a + 0] = dN[0]
            B[gp, 1, 3 * a + 1] = dN[1]
            B[gp, 2, 3 * a + 2] = dN[2]
            B[gp, 3, 3 * a + 0], B[gp, 3, 3 * a + 1] = dN[1], dN[0]
            B[gp, 4, 3 * a + 0], B[gp, 4, 3 * a + 2] = dN[2], dN[0]
            B[gp, 5, 3 * a + 1], B[gp, 5, 3 * a + 2] = dN[2], dN[1]
    return B, h[0] * h[1] * h[2] / 8.0


def strain_tensor(e):
    return np.array([[e[0], e[3] / 2, e[4] / 2], [e[3] / 2, e[1], e[5] / 2], [e[4] / 2, e[5] / 2, e[2]]])


class CellRef:
    def __init__(self, typ, n, mat1=MAT1, mat2=MAT2):
        self.n, ne, nn = n, n - 1, n ** 3
        self.B, self.detJ = element_B((1.0 / ne,) * 3)
        ek, ej, ei = np.meshgrid(np.arange(ne), np.arange(ne), np.arange(ne), indexing="ij")
        ei, ej, ek = ei.ravel(), ej.ravel(), ek.ravel()
        self.ph = phase_rule(typ, n).ravel()
        conn = np.stack([(ei + (a & 1)) + n * ((ej + (a >> 1 & 1)) + n * (ek + (a >> 2))) for a in range(8)], axis=1)
        self.edof = (3 * conn[:, :, None] + np.arange(3)[None, None, :]).reshape(-1, 24)
        self.nel = len(self.edof)
        idx = np.arange(nn)
        ci, cj, ck = idx % n, (idx // n) % n, idx // (n * n)
        self.X = np.stack([ci, cj, ck], axis=1) / ne
        bnd = (ci == 0) | (cj == 0) | (ck == 0) | (ci == ne) | (cj == ne) | (ck == ne)
        self.bd = np.repeat(bnd, 3)
        mats = np.array([mat1, mat2])[self.ph]  # [nel][4]
        E, nu = mats[:, 0], mats[:, 1]
        self.G = (E / (2 * (1 + nu)))[:, None]
        self.K = (E / (3 * (1 - 2 * nu)))[:, None]
        self.Sy, self.Ka = mats[:, 2][:, None], mats[:, 3][:, None]
        self.zero_hist = np.zeros((self.nel, 8, 7))
        # elastic unit-strain fields -> C_hom and the strain concentration of the linear test
        Ct = self.j2(np.zeros((self.nel, 8, 6)), self.zero_hist)[4]
        self.Chom, W, _ = self.tangent(Ct)
        self.A = np.stack([self.strains(W[:, l]) for l in range(6)], axis=-1)  # [nel][8][6][6]

    def boundary_field(self, eps):
        u = (self.X @ strain_tensor(eps).T).ravel()
        u[~self.bd] = 0.0
        return u

    def strains(self, u):
        return np.einsum("gkd,ed->egk", self.B, u[self.edof])

    def j2(self, eps, h):
        """(sigma, h_new, f, trial-stress norm, C) at every micro Gauss point [nel][8]."""
        G, K = self.G, self.K
        tr = eps[..., :3].sum(-1)
        dev = eps.copy()
        dev[..., :3] -= tr[..., None] / 3
        dev[..., 3:] /= 2
        st = 2 * G[..., None] * (dev - h[..., :6])
        sn = np.sqrt((st[..., :3] ** 2).sum(-1) + 2 * (st[..., 3:] ** 2).sum(-1))
        f = sn - np.sqrt(2 / 3) * (self.Sy + self.Ka * h[..., 6])
        pl = f > 0
        dg = np.where(pl, f / (2 * G + 2 / 3 * self.Ka), 0.0)
        nv = np.where(pl[..., None], st / np.where(sn > 0, sn, 1.0)[..., None], 0.0)
        s = st - 2 * G[..., None] * dg[..., None] * nv
        s[..., :3] += (K * tr)[..., None]
        hn = h.copy()
        hn[..., :6] += dg[..., None] * nv
        hn[..., 6] += np.sqrt(2 / 3) * dg
        th = np.where(pl, 1 - 2 * G * dg / np.where(sn > 0, sn, 1.0), 1.0)
        thb = np.where(pl, 1 / (1 + self.Ka / (3 * G)) - (1 - th), 0.0)
        Id = np.zeros((6, 6))
        Id[:3, :3] = -1 / 3
        Id[np.arange(3), np.arange(3)] += 1
        Id[np.arange(3, 6), np.arange(3, 6)] = 0.5
        m = np.zeros((6, 6))
        m[:3, :3] = 1
        C = (K[..., None, None] * m + (2 * G * th)[..., None, None] * Id
             - (2 * G * thb)[..., None, None] * nv[..., :, None] * nv[..., None, :])
        return s, hn, f, sn, C

    def stiffness(self, Ct):
        Ke = np.einsum("gki,egkl,glj->eij", self.B, Ct, self.B) * self.detJ
        Kt = np.zeros((3 * self.n ** 3,) * 2)
        np.add.at(Kt, (self.edof[:, :, None], self.edof[:, None, :]), Ke)
        return Kt

    def tangent(self, Ct):
        """(C symmetrised, the six fields, K_T,ii or None) with the tangents Ct frozen."""
        Kt, fr = self.stiffness(Ct), ~self.bd
        Kii = Kt[np.ix_(fr, fr)] if fr.any() else None
        W = np.zeros((len(self.bd), 6))
        Cm = np.zeros((6, 6))
        for l in range(6):
            e = np.zeros(6)
            e[l] = 1.0
            W[:, l] = self.boundary_field(e)
            if fr.any():
                W[fr, l] = np.linalg.solve(Kii, -Kt[np.ix_(fr, ~fr)] @ W[~fr, l])
            Cm[:, l] = np.einsum("egkl,egl->k", Ct, self.strains(W[:, l])) * self.detJ
        return 0.5 * (Cm + Cm.T), W, Kii

    def linear_f(self, eps):
        """largest trial f of the superposed elastic field, and its margin min|f| / Sy."""
        f = self.j2(self.A @ eps, self.zero_hist)[2]
        return f.max(), (np.abs(f) / self.Sy).min()

    def solve(self, eps, hold):
        u, fr = self.boundary_field(eps), ~self.bd
        n0 = 0.0
        for it in range(40):
            s, hn, f, sn, Ct = self.j2(self.strains(u), hold)
            R = np.zeros(len(u))
            np.add.at(R, self.edof, np.einsum("gki,egk->ei", self.B, s) * self.detJ)
            if not fr.any():
                break
            Kii = self.stiffness(Ct)[np.ix_(fr, fr)]
            if it == 0:
                D = np.diag(Kii).copy()
                n0 = np.linalg.norm(R[fr] / D)
            if n0 == 0.0 or np.linalg.norm(R[fr] / D) <= 1e-13 * n0:
                break
            u[fr] += np.linalg.solve(Kii, -R[fr])
        Cm, _, Kii = self.tangent(Ct)
        kappa = 1.0
        if Kii is not None:
            d = np.sqrt(np.diag(Kii))
            w = np.linalg.eigvalsh(Kii / np.outer(d, d))
            kappa = w[-1] / w[0]
        return dict(sig=s.sum((0, 1)) * self.detJ, C=Cm, h=hn, its=it, fmax=f.max(),
                    margin=(np.abs(f) / self.Sy).min(), kappa=kappa, strial=sn.max())

    def point(self, eps, hold=None):
        """what the law must give one macro point: linear shortcut (never solved before, no yield
        on the elastic field) or the solve; path, linear-test f and margin included."""
        flin, mlin = self.linear_f(eps)
        if hold is None and flin <= 0:
            return dict(path=0, sig=self.Chom @ eps, C=self.Chom, h=None, its=0, fmax=flin, margin=mlin,
                        kappa=1.0, flin=flin, mlin=mlin, strial=0.0)
        r = self.solve(eps, self.zero_hist if hold is None else hold)
        r.update(path=1, flin=flin, mlin=mlin if hold is None else np.inf)  # the linear test judges fresh points only
        return r


@functools.lru_cache(maxsize=None)
def cell(typ, n):
    return CellRef(typ, n)


def nl_argv(typ, n, grid=(2, 2, 2), extra=(), law="micro_nl", box=None):
    box = box or tuple(g - 1 for g in grid)  # unit elements
    return ["-da_grid_x", grid[0], "-da_grid_y", grid[1], "-da_grid_z", grid[2], "-lx", box[0], "-ly", box[1],
            "-lz", box[2], "-mat_law", law, "-micro_n", n, "-micro_type", typ,
            "-micro_mat_1", "%r,%r,%r,%r" % MAT1, "-micro_mat_2", "%r,%r,%r,%r" % MAT2, *extra]


def node_coords(grid, box=None):
    box = box or tuple(g - 1 for g in grid)
    k, j, i = np.meshgrid(*(np.arange(g) for g in grid[::-1]), indexing="ij")
    return np.stack([i.ravel() * box[0] / (grid[0] - 1), j.ravel() * box[1] / (grid[1] - 1),
                     k.ravel() * box[2] / (grid[2] - 1)], axis=1)


def field(grid, seed, amp, wobble=0.15, ramp=None):
    """u = E0 x (E0 from amp * uniform(-1, 1, 6)) plus a nodal wobble, so every Gauss point gets its
    own strain; ramp scales the whole field linearly in x from ramp[0] to ramp[1]."""
    rng = np.random.default_rng(seed)
    e0 = amp * rng.uniform(-1, 1, 6)
    X = node_coords(grid)
    u = X @ strain_tensor(e0).T + wobble * amp * rng.uniform(-1, 1, X.shape)
    if ramp is not None:
        u *= (ramp[0] + (ramp[1] - ramp[0]) * X[:, 0] / X[:, 0].max())[:, None]
    return u.ravel()


def evaluate(m, u):
    m.set_u(u)
    m.set_strains()
    m.homogenize()
    return m.gp_strain(), m.stress().reshape(-1, 6), m.gp_ctan(), m.micro_nl_info()


def check_conditions(r):
    assert r["its"] <= 10, r["its"]
    assert r["margin"] >= MARGIN and r["mlin"] >= MARGIN, (r["margin"], r["mlin"])


# ---------------------------------------------------------------- 1. against the reference
@pytest.mark.parametrize("seed,amp", LOADS)
@pytest.mark.parametrize("typ,n", CELLS)
def test_against_reference(typ, n, seed, amp):
    """sigma and C of 8 Gauss points with their own strains against the reference through the load
    path u -> 1.5 u -> 0.5 u with a commit between the stages; paths, final residuals, symmetry,
    and the committed history showing in stage 3.  Measured on an MI355X: errors <= 9.9e-13
    (sigma) and 2.4e-13 (C) of the largest entry against bars of 1e-8 .. 6.5e-8, 3 to 5 Newton
    iterations (DESIGN §12 has the table)."""
    ref = cell(typ, n)
    u1 = field((2, 2, 2), seed, amp)
    hold = [None] * 8
    with M.Macroc(nl_argv(typ, n)) as m:
        for stage, fac in enumerate(STAGES):
            eps, sig, Cg, info = evaluate(m, fac * u1)
            worst = [0.0, 0.0, 0.0]
            for q in range(8):
                r = ref.point(eps[q], hold[q])
                check_conditions(r)
                assert info["path"][q] == r["path"]
                bar = 100 * r["kappa"] * NL_RTOL
                es = np.abs(sig[q] - r["sig"]).max() / np.abs(r["sig"]).max()
                ec = np.abs(Cg[q] - r["C"]).max() / np.abs(r["C"]).max()
                worst = [max(worst[0], es / bar), max(worst[1], ec / bar), max(worst[2], r["kappa"])]
                print(f"cell ({typ},{n}) load ({seed},{amp}) stage {stage} gp {q}: path {r['path']} kappa "
                      f"{r['kappa']:.1f} err sigma {es:.2e} C {ec:.2e} bar {bar:.2e} newton gpu "
                      f"{info['newton_its'][q]} ref {r['its']} cg {info['cg_its'][q]} rnorm {info['rnorm'][q]:.1e}")
                assert es <= bar and ec <= bar
                assert info["rnorm"][q] <= NL_RTOL
                assert np.array_equal(Cg[q], Cg[q].T)
                if stage == 2:  # the committed history shows: a fresh solve of 0.5 eps is far away
                    fresh = ref.point(eps[q])
                    assert np.abs(fresh["sig"] - r["sig"]).max() > 1e3 * bar * np.abs(r["sig"]).max()
                    assert np.abs(sig[q] - fresh["sig"]).max() > 1e3 * bar * np.abs(r["sig"]).max()
                if r["path"]:
                    hold[q] = r["h"]
            m.update_vars()
        assert info["slots_used"] == sum(h is not None for h in hold) and info["slots"] >= info["slots_used"]
        assert any(h is not None for h in hold)  # the load yields


# ---------------------------------------------------------------- 2. n = 2 against the device J2 law
def test_n2_is_the_plastic_law():
    u1 = field((2, 2, 2), 5, 4e-3)
    out = {}
    for law in ("micro_nl", "plastic"):
        with M.Macroc(nl_argv(1, 2, law=law)) as m:
            res = []
            for fac in (1.0, 1.5):
                m.set_u(fac * u1)
                m.set_strains()
                m.homogenize()
                res.append((m.stress().reshape(-1, 6), m.gp_ctan(), m.nonlinear_stats()))
                if law == "micro_nl":
                    info = m.micro_nl_info()
                    assert info["path"].all()  # the load yields at every point
                    assert not info["newton_its"].any() and not info["cg_its"].any()
                m.update_vars()
            out[law] = res
    for (sa, ca, na), (sb, cb, nb) in zip(out["micro_nl"], out["plastic"]):
        assert np.abs(sa - sb).max() <= 1e-12 * np.abs(sb).max()
        assert np.abs(ca - cb).max() <= 1e-12 * np.abs(cb).max()
        assert na[0] == nb[0] == 8 and abs(na[1] - nb[1]) <= 1e-12 * np.abs(sb).max()


# ---------------------------------------------------------------- 3. below yield: the linear law
def assemble(m, u, inject=None):
    m.set_u(u)
    m.set_strains()
    m.homogenize()
    if inject is not None:
        m.set_gp_stress(inject[0])
        m.set_gp_ctan(inject[1].reshape(-1, 36))
    m.assembly_res()
    m.assembly_jac()
    return m.b(), m.dump_csr()[2]


def test_below_yield_is_the_linear_law_bit_for_bit():
    grid, ref = (7, 6, 5), cell(1, 4)
    u = field(grid, 11, 2e-5)
    with M.Macroc(nl_argv(1, 4, grid)) as a:
        ba, va = assemble(a, u)
        eps, sa, info = a.gp_strain(), a.stress(), a.micro_nl_info()
        fl = [ref.linear_f(e) for e in eps]
        assert max(f for f, _ in fl) < 0 and min(mg for _, mg in fl) >= MARGIN
        assert not info["path"].any() and info["slots"] == 0 and info["slots_used"] == 0
        assert a.nonlinear_stats()[0] == 0
        a.update_vars()
    with M.Macroc(nl_argv(1, 4, grid, law="micro")) as b:
        bb, vb = assemble(b, u)
        sb = b.stress()
    assert np.linalg.norm(bb) > 0
    assert np.array_equal(sa, sb) and np.array_equal(ba, bb) and np.array_equal(va, vb)


# ---------------------------------------------------------------- 4. / 5. mixed grid
MIXED_GRID, MIXED_CELL, MIXED_AMP = (4, 3, 3), (1, 4), 1e-3


def mixed_u():
    return field(MIXED_GRID, 22, MIXED_AMP, ramp=(0.05, 1.0))


@functools.lru_cache(maxsize=None)
def mixed_state():
    """the law's own results on the mixed grid, and the reference's for the same strains."""
    ref = cell(*MIXED_CELL)
    with M.Macroc(nl_argv(*MIXED_CELL, MIXED_GRID, ["-ksp_rtol", repr(1e-12)])) as m:
        b, v = assemble(m, mixed_u())
        eps, sig, Cg, info = m.gp_strain(), m.stress().reshape(-1, 6), m.gp_ctan(), m.micro_nl_info()
        stats = m.nonlinear_stats()
        its, rn, reason = m.solve_Ax()
        du, dirichlet = m.du(), m.dump_dirichlet()
    pts = [ref.point(e) for e in eps]
    for r in pts:
        check_conditions(r)
    return dict(b=b, v=v, eps=eps, sig=sig, C=Cg, info=info, stats=stats, du=du, reason=reason, pts=pts,
                dirichlet=dirichlet)


def external(u, sig, Cg, extra=()):
    argv = ["-da_grid_x", MIXED_GRID[0], "-da_grid_y", MIXED_GRID[1], "-da_grid_z", MIXED_GRID[2],
            "-lx", MIXED_GRID[0] - 1, "-ly", MIXED_GRID[1] - 1, "-lz", MIXED_GRID[2] - 1, "-mat_law", "external", *extra]
    with M.Macroc(argv) as m:
        return assemble(m, u, inject=(sig, Cg))


def test_mixed_grid_paths_and_values():
    S = mixed_state()
    pts, info = S["pts"], S["info"]
    path = np.array([r["path"] for r in pts])
    assert 0 < path.sum() < len(path)  # some over yield, some under
    assert np.array_equal(info["path"], path)
    bar = 100 * max(r["kappa"] for r in pts) * NL_RTOL
    for q, r in enumerate(pts):
        assert np.abs(S["sig"][q] - r["sig"]).max() <= bar * np.abs(r["sig"]).max()
        assert np.abs(S["C"][q] - r["C"]).max() <= bar * np.abs(r["C"]).max()
        if not r["path"]:
            assert np.array_equal(S["C"][q], S["C"][np.argmin(path)])  # one C_hom, the same bits
    n, fmax = S["stats"]
    fref = max(r["fmax"] for r in pts)
    assert n == path.sum()
    assert abs(fmax - fref) <= bar * max(r["strial"] for r in pts)  # f's error is the trial stress's (2G d eps)
    assert info["slots_used"] == path.sum()


def test_mixed_grid_plumbing_and_reference_residual():
    S = mixed_state()
    b, v = external(mixed_u(), S["sig"], S["C"])
    assert np.array_equal(b, S["b"]) and np.array_equal(v, S["v"])
    sref = np.array([r["sig"] for r in S["pts"]])
    bref, _ = external(mixed_u(), sref, S["C"])
    # |b_row(sigma) - b_row(sigma_ref)| <= max|d sigma| sum |B| wg over the row's Gauss points
    Bm, detJ = element_B((1.0, 1.0, 1.0))
    NX, NY, NZ = MIXED_GRID
    rows = np.zeros(3 * NX * NY * NZ)
    w = np.abs(Bm).sum((0, 1)) * detJ  # [24]
    for ez in range(NZ - 1):
        for ey in range(NY - 1):
            for ex in range(NX - 1):
                for a in range(8):
                    nd = (ex + (a & 1)) + NX * ((ey + (a >> 1 & 1)) + NY * (ez + (a >> 2)))
                    rows[3 * nd:3 * nd + 3] += w[3 * a:3 * a + 3]
    bar = 100 * max(r["kappa"] for r in S["pts"]) * NL_RTOL * np.abs(sref).max()
    assert np.linalg.norm(bref) > 0
    assert np.all(np.abs(S["b"] - bref) <= bar * rows)


@pytest.mark.parametrize("extra", [["-dm_mat_type", "sbaij"], ["-mat_aij_vi", 0]], ids=["sbaij", "aij_vi0"])
def test_mixed_grid_storages(extra):
    S = mixed_state()
    assert S["reason"] > 0 and np.linalg.norm(S["du"]) > 0
    with M.Macroc(nl_argv(*MIXED_CELL, MIXED_GRID, ["-ksp_rtol", repr(1e-12), *extra])) as m:
        assemble(m, mixed_u())
        its, rn, reason = m.solve_Ax()
        du = m.du()
    assert reason > 0
    assert np.linalg.norm(du - S["du"]) <= 1e-10 * np.linalg.norm(S["du"])


def test_tangent_consistency_at_the_macro_level():
    """(b(u + h v) - b(u - h v)) / 2h against -A v on the non-Dirichlet rows.  The same mismatch is
    measured first with the reference's (sigma, C) injected into the external law; the GPU law gets
    10 x that (its inner CG adds iterative error the dense reference has not)."""
    S, ref, u = mixed_state(), cell(*MIXED_CELL), mixed_u()
    rng = np.random.default_rng(3)
    v = rng.uniform(-1, 1, len(u))
    v[S["dirichlet"]] = 0.0
    h = 1e-7 * MIXED_AMP
    free = np.ones(len(u), bool)
    free[S["dirichlet"]] = False

    def mismatch(bp, bm, Av):
        return np.abs((bp - bm)[free] / (2 * h) + Av[free]).max() / np.abs(Av[free]).max()

    with M.Macroc(nl_argv(*MIXED_CELL, MIXED_GRID)) as m:
        assemble(m, u)
        Av = m.spmv(v)
        bp, _ = assemble(m, u + h * v)
        ep = m.gp_strain()
        bm, _ = assemble(m, u - h * v)
        em = m.gp_strain()
    gpu = mismatch(bp, bm, Av)
    argv = ["-da_grid_x", MIXED_GRID[0], "-da_grid_y", MIXED_GRID[1], "-da_grid_z", MIXED_GRID[2],
            "-lx", MIXED_GRID[0] - 1, "-ly", MIXED_GRID[1] - 1, "-lz", MIXED_GRID[2] - 1, "-mat_law", "external"]
    Cref = np.array([r["C"] for r in S["pts"]])
    with M.Macroc(argv) as x:
        assemble(x, u, inject=(np.array([r["sig"] for r in S["pts"]]), Cref))
        Avr = x.spmv(v)
        # a point's path is decided at u (the law keeps a solved point on the non-linear path)
        rbp, _ = assemble(x, u + h * v, inject=(np.array([ref.point(e)["sig"] for e in ep]), Cref))
        rbm, _ = assemble(x, u - h * v, inject=(np.array([ref.point(e)["sig"] for e in em]), Cref))
    refm = mismatch(rbp, rbm, Avr)
    print(f"central-difference mismatch: reference {refm:.3e}, gpu {gpu:.3e}")
    assert gpu <= 10 * refm


# ---------------------------------------------------------------- 6. determinism and independence
def test_two_runs_are_bitwise_equal():
    u1 = field((2, 2, 2), 5, 4e-3)
    runs = []
    for _ in range(2):
        with M.Macroc(nl_argv(0, 5)) as m:
            out = []
            for fac in STAGES:  # the histories are compared through the later stages
                _, sig, Cg, info = evaluate(m, fac * u1)
                out.append((sig, Cg, info["newton_its"], info["cg_its"], info["rnorm"]))
                m.update_vars()
            runs.append(out)
    for a, b in zip(*runs):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)


def test_results_do_not_depend_on_slot_or_grid():
    """the 2x2x2 grid's element again as the second element of a 3x2x2 grid whose first element
    is solved too: other slots, other workgroups, other launch size, the same bits."""
    u1 = field((2, 2, 2), 5, 4e-3).reshape(2, 2, 2, 3)  # [k][j][i]
    big = np.zeros((2, 2, 3, 3))
    big[:, :, 1:, :] = u1
    big[:, :, 0, :] = field((2, 2, 2), 9, 4e-3).reshape(2, 2, 2, 3)[:, :, 0, :]
    with M.Macroc(nl_argv(0, 4)) as a, M.Macroc(nl_argv(0, 4, (3, 2, 2))) as b:
        for fac in STAGES:
            ea, sa, ca, ia = evaluate(a, fac * u1.ravel())
            eb, sb, cb, ib = evaluate(b, fac * big.ravel())
            assert np.array_equal(ea, eb[8:])  # the same strains, bit for bit
            assert ib["path"][:8].any()  # the first element takes slots too
            assert np.array_equal(sa, sb[8:]) and np.array_equal(ca, cb[8:])
            a.update_vars()
            b.update_vars()


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
    Sy = float("%.3e" % (np.sqrt(1.5) * 2 * MAT1[0] / (2 * (1 + MAT1[1])) * np.quantile(dn[dn > 0], 0.8)))
    argv = ["-da_grid_x", grid[0], "-da_grid_y", grid[1], "-da_grid_z", grid[2], "-mat_law", "micro_nl", "-micro_n", 4,
            "-micro_type", 0, "-micro_mat_1", "%r,%r,%r,%r" % (MAT1[0], MAT1[1], Sy, MAT1[3]),
            "-micro_mat_2", "%r,%r,%r,%r" % MAT2, "-ksp_rtol", repr(1e-12)]

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
    du = np.zeros_like(one["du"])
    for r in res:
        du[r["nat"]] = r["du"]
    ref = np.zeros_like(du)
    ref[one["nat"]] = one["du"]
    assert np.linalg.norm(du - ref) <= 1e-10 * np.linalg.norm(ref)
    for r in res:
        assert abs(r["force"] - one["force"]) <= 1e-10 * abs(one["force"])
        assert r["nl"][1] == one["nl"][1]
    assert res[0]["nl"][0] + res[1]["nl"][0] == one["nl"][1]


# ---------------------------------------------------------------- 7. refusals
def test_refusals_leave_a_usable_context():
    u1 = field((2, 2, 2), 5, 4e-3)
    for flag, val, word in (("-micro_n", 11, "micro_n"), ("-micro_n", 1, "micro_n"), ("-micro_type", 2, "micro_type")):
        with M.Macroc(nl_argv(0, 4) + [flag, val]) as m:  # the later flag wins
            m.set_u(u1)
            m.set_strains()
            for call in (m.homogenize, m.assembly_jac):
                with pytest.raises(M.MacrocError, match=word):
                    call()
    with M.Macroc(nl_argv(*MIXED_CELL, MIXED_GRID)) as m:
        m.set_option("micro_nl_slots", 1)
        m.set_u(mixed_u())
        m.set_strains()
        need = int(mixed_state()["info"]["slots_used"])
        with pytest.raises(M.MacrocError, match=r"micro_nl_slots 1, 0 slots in use and %d more" % need):
            m.homogenize()
        assert m.micro_nl_info()["slots"] == 0
        m.set_option("micro_nl_slots", need)
        m.homogenize()
        assert np.array_equal(m.stress().reshape(-1, 6), mixed_state()["sig"])
        assert m.micro_nl_info()["slots"] == need == m.micro_nl_info()["slots_used"]
    with M.Macroc(nl_argv(0, 4)) as m:
        m.set_option("micro_nl_max_it", 1)
        m.set_u(u1)
        m.set_strains()
        with pytest.raises(M.MacrocError, match=r"\d+ of \d+ micro cells did not converge; worst: Gauss point \d+ "
                                                r".*1 Newton iterations \(micro_nl_max_it 1\)"):
            m.homogenize()
        m.set_option("micro_nl_max_it", 20)
        m.homogenize()
        sig = m.stress().reshape(-1, 6)
    with M.Macroc(nl_argv(0, 4)) as m:
        assert np.array_equal(evaluate(m, u1)[1], sig)
    with M.Macroc(nl_argv(0, 4, law="micro")) as m:
        with pytest.raises(M.MacrocError, match="without -mat_law micro_nl"):
            m.micro_nl_info()
        with pytest.raises(M.MacrocError, match="no tangent per Gauss point"):
            m.gp_ctan()
        m.set_option("micro_nl_slots", 4)  # accepted, unused
        m.micro_ctan()


# ---------------------------------------------------------------- 8. n = 10
def test_n10_converges_and_unloads_to_chom():
    """GPU only, no dense reference.  A solved point stays on the non-linear path for good, so the
    load below yield goes to a fresh context: it must return the linear law's C_hom, bit for bit."""
    u1 = field((2, 2, 2), 5, 4e-3)
    with M.Macroc(nl_argv(0, 10, law="micro")) as lin:
        Ch = lin.micro_ctan()[0]
    with M.Macroc(nl_argv(0, 10)) as m:
        m.set_u(u1)
        m.set_strains()
        m.synchronize()
        t0 = time.perf_counter()
        m.homogenize()
        m.synchronize()
        dt = time.perf_counter() - t0
        sig, Cg, info = m.stress().reshape(-1, 6), m.gp_ctan(), m.micro_nl_info()
        assert info["path"].all() and (info["rnorm"] <= NL_RTOL).all() and (info["newton_its"] >= 1).all()
        print(f"n = 10: {dt / 8 * 1e3:.2f} ms per solved point (8 points in one launch, {dt * 1e3:.2f} ms), newton "
              f"{info['newton_its']}, cg {info['cg_its']}, bytes per slot {info['bytes_per_slot']}")
        assert info["bytes_per_slot"] == 28 * 8 * 8 * 729 and info["slots"] == 8
        for q in range(8):
            assert np.array_equal(Cg[q], Cg[q].T)
            assert np.linalg.eigvalsh(Cg[q]).min() > 0
            assert np.isfinite(sig[q]).all()
    with M.Macroc(nl_argv(0, 10)) as m:  # a fresh context at a load below yield: C_hom, bit for bit
        eps, sig, Cg, info = evaluate(m, 0.01 * u1)
        assert not info["path"].any() and info["slots"] == 0
        for q in range(8):
            assert np.array_equal(Cg[q], Ch)


def test_driver_runs_the_law(tmp_path):
    exe = os.path.join(ROOT, "macroc_amd", "driver", "macroc_amd")
    out = subprocess.run([exe, "-da_grid_x", "6", "-da_grid_y", "5", "-da_grid_z", "4", "-mat_law", "micro_nl",
                          "-micro_n", "4", "-micro_type", "0", "-micro_mat_1", "1e7,0.25,1e4,1e6",
                          "-micro_mat_2", "1e8,0.3,1e9,1e7"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert "id 0 : E = 1.000000e+07\tnu = 2.500000e-01\tSy = 1.000000e+04\tKa = 1.000000e+06" in lines
    assert "id 1 : E = 1.000000e+08\tnu = 3.000000e-01\tSy = 1.000000e+09\tKa = 1.000000e+07" in lines
    assert any(l.startswith("Non-Linear Gauss points : ") for l in lines)
    assert "has no effect" not in out.stderr and "Elapsed time" in out.stdout
