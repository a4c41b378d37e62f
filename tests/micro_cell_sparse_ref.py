"""A sparse restatement of test_gpu_micro_nl.CellRef for cells a dense K_T cannot reach (n = 21, 26).

SparseCellRef keeps CellRef's definition, Newton stop (1e-13 of the first Jacobi-scaled norm, D from the
first iterate) and returned keys, and replaces its linear algebra: K_T is assembled by scipy.sparse, the
Newton steps and the six tangent columns go through one splu factorisation of K_T,ii each, and kappa of the
Jacobi-scaled K_T,ii comes from eigsh (the largest eigenvalue directly, the smallest through the
factorisation).  solve() adds one key, nplastic: the number of micro Gauss points with f > 0 at the
converged state.

It is far too slow for a GPU test (minutes per load stage at n = 26), so tests/golden/make_micro_cells.py
runs it once and commits the results; tests/test_micro_cell_sparse_cpu.py checks it against the dense
CellRef at the sizes both can do.  scipy is imported here only.
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import test_gpu_micro_nl as TN

EIG_TOL = 1e-10  # eigsh's relative accuracy of the two extreme eigenvalues


class SparseCellRef(TN.CellRef):
    def __init__(self, typ, n, mat1=TN.MAT1, mat2=TN.MAT2, flip=()):
        """flip: elements (i, j, k) whose phase is inverted after the integer rule (the generator's
        sensitivity run); every derived quantity is rebuilt for the changed map."""
        self._fact = None
        super().__init__(typ, n, mat1, mat2)
        if len(flip):
            ne = n - 1
            for i, j, k in flip:
                self.ph[i + ne * (j + ne * k)] ^= 1
            mats = np.array([mat1, mat2])[self.ph]
            E, nu = mats[:, 0], mats[:, 1]
            self.G = (E / (2 * (1 + nu)))[:, None]
            self.K = (E / (3 * (1 - 2 * nu)))[:, None]
            self.Sy, self.Ka = mats[:, 2][:, None], mats[:, 3][:, None]
            Ct = self.j2(np.zeros((self.nel, 8, 6)), self.zero_hist)[4]
            self.Chom, W, _ = self.tangent(Ct)
            self.A = np.stack([self.strains(W[:, l]) for l in range(6)], axis=-1)
        # the elastic K_ii is the last matrix factorised above: its kappa judges C_hom
        self.kappa_lin = self.kappa(*self._fact) if self._fact is not None else 1.0
        self._fact = None

    def stiffness(self, Ct):
        """K_T as a CSR matrix of all 3 n^3 dofs."""
        T = np.matmul(Ct, self.B[None])  # [nel][8][6][24]
        B2 = self.B.reshape(48, 24)
        Ke = np.matmul(B2.T[None], T.reshape(self.nel, 48, 24)) * self.detJ  # [nel][24][24]
        rows = np.broadcast_to(self.edof[:, :, None], Ke.shape).ravel()
        cols = np.broadcast_to(self.edof[:, None, :], Ke.shape).ravel()
        nd = 3 * self.n ** 3
        return sp.csr_matrix((Ke.ravel(), (rows, cols)), shape=(nd, nd))

    def interior(self, Kt):
        fr = np.flatnonzero(~self.bd)
        return Kt[fr][:, fr].tocsc()

    @staticmethod
    def factor(Kii):
        # K_T,ii is symmetric positive definite: no pivoting, the ordering of the symmetric pattern
        return spla.splu(Kii, permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))

    @staticmethod
    def kappa(Kii, lu):
        """condition number of D^-1/2 K_ii D^-1/2, D = diag K_ii"""
        d = np.sqrt(Kii.diagonal())
        n = len(d)
        if n <= 2:
            w = np.linalg.eigvalsh(Kii.toarray() / np.outer(d, d))
            return w[-1] / w[0]
        S = sp.diags(1.0 / d) @ Kii @ sp.diags(1.0 / d)
        v0 = np.random.default_rng(0).uniform(-1, 1, n)
        top = spla.eigsh(S, k=1, which="LA", tol=EIG_TOL, v0=v0, return_eigenvectors=False)[0]
        inv = spla.LinearOperator((n, n), matvec=lambda x: d * lu.solve(d * np.asarray(x).ravel()), dtype=float)
        low = 1.0 / spla.eigsh(inv, k=1, which="LA", tol=EIG_TOL, v0=v0, return_eigenvectors=False)[0]
        return top / low

    def tangent(self, Ct):
        """(C symmetrised, the six fields, K_T,ii sparse or None) with the tangents Ct frozen."""
        fr = ~self.bd
        Kt = self.stiffness(Ct)
        Kii = lu = None
        if fr.any():
            Kii = self.interior(Kt)
            lu = self.factor(Kii)
            self._fact = (Kii, lu)
        W = np.zeros((len(self.bd), 6))
        Cm = np.zeros((6, 6))
        for l in range(6):
            e = np.zeros(6)
            e[l] = 1.0
            W[:, l] = self.boundary_field(e)  # interior zero: Kt @ W is the boundary columns' product
            if fr.any():
                W[fr, l] = lu.solve(-(Kt @ W[:, l])[fr])
            Cm[:, l] = np.einsum("egkl,egl->k", Ct, self.strains(W[:, l])) * self.detJ
        return 0.5 * (Cm + Cm.T), W, Kii

    def solve(self, eps, hold):
        u, fr = self.boundary_field(eps), ~self.bd
        n0 = 0.0
        for it in range(40):
            s, hn, f, sn, Ct = self.j2(self.strains(u), hold)
            R = np.zeros(len(u))
            np.add.at(R, self.edof, np.einsum("gki,egk->ei", self.B, s) * self.detJ)
            if not fr.any():
                break
            Kii = self.interior(self.stiffness(Ct))
            if it == 0:
                D = Kii.diagonal().copy()
                n0 = np.linalg.norm(R[fr] / D)
            if n0 == 0.0 or np.linalg.norm(R[fr] / D) <= 1e-13 * n0:
                break
            u[fr] += self.factor(Kii).solve(-R[fr])
        Cm, _, Kii = self.tangent(Ct)
        kappa = self.kappa(*self._fact) if Kii is not None else 1.0
        self._fact = None
        return dict(sig=s.sum((0, 1)) * self.detJ, C=Cm, h=hn, its=it, fmax=f.max(),
                    margin=(np.abs(f) / self.Sy).min(), kappa=kappa, strial=sn.max(), nplastic=int((f > 0).sum()))

    def matrix_points(self):
        """micro Gauss points of phase 0, the matrix"""
        return 8 * int((self.ph == 0).sum())
