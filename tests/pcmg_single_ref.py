"""-pc_mg_precision single in numpy / scipy: the hierarchy's rule, the Galerkin products,
the eigenvalue estimates, the V-cycle and a PCG around it, in double or with the levels >= 1 stored
in float.  tests/test_pcmg_single_cpu.py runs it on the oracle's matrix, tests/test_gpu_pcmg_single.py
holds the device against it.

The rule is restated from tests/test_gpu_pcmg.py: an axis of N > 2 nodes keeps its even nodes and, when
N - 1 is odd, its last node; the other nodes take 1/2, 1/2 of their two neighbours; P is the tensor
product times I_3 with zero rows at Dirichlet dofs.

What "single" rounds, np.float32 at exactly these stores (every expression around them is double):
the operators of the levels >= 1 (level 1: the double product rounded; deeper: the stored A_l P e,
then the restricted result), 1 / a of the stored diagonal, and on such a level every stored vector:
r = b - A x, the Chebyshev increment d and the iterate x, the restricted right-hand side (also the
one level 0 hands to level 1), the coarsest solve's result and the iterate after P's correction."""
import numpy as np
import scipy.sparse as sp

GRIDS = [(17, 17, 17), (16, 16, 16), (24, 9, 13), (40, 3, 40), (5, 17, 17)]

# The relative asymmetry |u.M^-1 v - v.M^-1 u| / |u.M^-1 v| of the single-precision reference cycle
# V(2,2), free dofs only: the largest of asymmetry()'s four pairs, as tests/test_pcmg_single_cpu.py
# measured it on the oracle's matrix.  The value is rounding noise (the pairs spread over a factor 30,
# and another numpy or BLAS build moves it), so both tests hold what they measure on the same four
# pairs, the reference on the CPU and the device, to the same bar: 10 x this.
REF_ASYM = {(17, 17, 17): 4.416e-08, (16, 16, 16): 2.506e-08, (24, 9, 13): 1.002e-07, (40, 3, 40): 1.149e-07,
            (5, 17, 17): 2.104e-08}


def f32(a):
    """round to float, keep as double"""
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def ident(a):
    return a


def f32_csr(A):
    A = A.tocsr().copy()
    A.data = f32(A.data)
    return A


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
    Pn = sp.kron(axis_P(n[2]), sp.kron(axis_P(n[1]), axis_P(n[0])))
    P = sp.kron(Pn, sp.identity(3)).tocsr()
    return (sp.diags(np.where(dirichlet, 0.0, 1.0)) @ P).tocsr()


def unit_on_empty(Ac):
    empty = Ac.diagonal() == 0.0
    return (Ac + sp.diags(np.where(empty, 1.0, 0.0))).tocsr(), empty


def hierarchy(A, dmask, grid, single):
    """(sizes, ops, Ps): every level's operator from the fine matrix down, by the probing's two steps:
    T = A_l P (what the level's product stores), A_{l+1} = P^T T (what the restriction stores)"""
    sizes = level_sizes(grid)
    ops, Ps, mask = [A.tocsr()], [], dmask
    for l in range(len(sizes) - 1):
        P = prolongation(sizes[l], mask)
        T = (ops[-1] @ P).tocsr()
        if single and l >= 1:
            T = f32_csr(T)  # level l's product lands in its float r
        Ac = (P.T @ T).tocsr()
        if single:
            Ac = f32_csr(Ac)  # the restricted result lands in level l + 1's float b
        Ac, mask = unit_on_empty(Ac)
        ops.append(Ac)
        Ps.append(P)
    return sizes, ops, Ps


def seed(n):
    """the power iteration's start vector (k_pcmg_seed), dof q = 3 * node + d"""
    h = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(2246822519)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(13)
    return (h & np.uint64(0xFFFFFF)).astype(np.float64) * (1.0 / 16777216.0) - 0.5 + 1.0 / 33554432.0


def dinv_of(A, rnd):
    return rnd(1.0 / A.diagonal())


def estimates(ops, single):
    """lmax per level: ten power iterations on D^-1 A from the seed, the norm in double; 0 on the coarsest"""
    out = []
    for l, A in enumerate(ops[:-1]):
        rnd = f32 if single and l >= 1 else ident
        dinv, x, nrm = dinv_of(A, rnd), rnd(seed(A.shape[0])), 0.0
        for _ in range(10):
            v = dinv * rnd(A @ x)
            nrm = np.sqrt(np.sum(v * v))
            x = rnd((1.0 / nrm) * rnd(v))
        out.append(nrm)
    return np.array(out + [0.0])


def chebyshev(A, dinv, lmax, b, x, k, rnd=ident):
    """k steps of PETSc's Chebyshev recurrence on D^-1 A over [0.1, 1.1] lmax, from x (None: 0)"""
    emin, emax = 0.1 * lmax, 1.1 * lmax
    scale = 2.0 / (emax + emin)
    alpha = 1.0 - scale * emin
    mu, omegaprod = 1.0 / alpha, 2.0 / alpha
    ckm1, ck = 1.0, mu
    d = None
    for s in range(k):
        r = b if x is None else rnd(b - A @ x)
        if s == 0:
            dn = scale * (dinv * r)
        else:
            ckp1 = 2.0 * mu * ck - ckm1
            omega = omegaprod * ck / ckp1
            dn = (omega - 1.0) * d + omega * scale * (dinv * r)
            ckm1, ck = ck, ckp1
        d = rnd(dn)
        x = rnd(dn) if x is None else rnd(x + dn)
    return x


def vcycle(ops, Ps, lmax, l, b, k=2, single=False):
    """single: the levels >= 1 store float (ops are then the float operators, widened)"""
    rnd = f32 if single and l >= 1 else ident
    rnd_c = f32 if single else ident  # the next coarser level's stores
    if l == len(ops) - 1:
        A = ops[l].toarray()
        return rnd(np.linalg.solve(0.5 * (A + A.T), b))
    A = ops[l]
    dinv = dinv_of(A, rnd)
    x = chebyshev(A, dinv, lmax[l], b, None, k, rnd)
    bc = rnd_c(Ps[l].T @ rnd(b - A @ x))
    xc = vcycle(ops, Ps, lmax, l + 1, bc, k, single)
    x = rnd(x + Ps[l] @ xc)
    return chebyshev(A, dinv, lmax[l], b, x, k, rnd)


def pcg(A, b, Minv, rtol, maxit=200):
    """KSPCG with the norm sqrt(r . z): (iterations, x, the norms' history)"""
    x = np.zeros_like(b)
    r = b.copy()
    z = Minv(r)
    beta = r @ z
    hist = [np.sqrt(beta)]
    ttol = rtol * hist[0]
    p, its = None, 0
    while hist[-1] > ttol and its < maxit:
        p = z.copy() if p is None else z + (beta / betaold) * p
        w = A @ p
        a = beta / (p @ w)
        x = x + a * p
        r = r - a * w
        z = Minv(r)
        betaold, beta = beta, r @ z
        hist.append(np.sqrt(beta))
        its += 1
    return its, x, hist


def asymmetry(Minv, free, n, pairs=4):
    """[|u.Mv - v.Mu| / |u.Mv|] for `pairs` pairs u, v of default_rng(7), zero on the Dirichlet dofs
    (the first pair is tests/test_gpu_pcmg.py's), and min(u.Mu, v.Mv)"""
    rng = np.random.default_rng(7)
    out, pos = [], np.inf
    for _ in range(pairs):
        u, v = rng.standard_normal(n) * free, rng.standard_normal(n) * free
        Mu, Mv = Minv(u), Minv(v)
        out.append(abs(u @ Mv - v @ Mu) / abs(u @ Mv))
        pos = min(pos, u @ Mu, v @ Mv)
    return out, pos
