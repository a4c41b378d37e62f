"""-pc_mg_precision single on the GPU: the option, the double hierarchy's bits, the float
operators against the double ones and against scipy's products, the V-cycle against the numpy
restatement that rounds at the same stores (tests/pcmg_single_ref.py), the PCG solve, the Newton loop,
the memory, the driver, and the same over the in-process transport under pc_mg_dist.

The helpers restate tests/test_gpu_pcmg.py's and tests/test_gpu_pcmg_dist.py's.  The bars: e' is the
distance between the numpy cycle in single and in double, computed in the test that uses it; the
asymmetry's scale is what tests/test_pcmg_single_cpu.py recorded for the reference (R.REF_ASYM); the
solve's bars are tests/test_gpu_pcmg.py's; the operators' bound is three float roundings, derived at
test_deeper_levels."""
import os
import re
import subprocess
import threading

import numpy as np
import pytest
import scipy.sparse as sp

import macroc_amd as M
import pcmg_single_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLASTIC = ["-da_grid_x", 12, "-da_grid_y", 10, "-da_grid_z", 12, "-dt", 0.01, "-ksp_rtol", "1e-12", "-mat_law", "plastic"]
DIST = {"A": ((17, 17, 17), (2, 1, 1)), "B": ((16, 16, 16), (2, 2, 2)), "C": ((24, 9, 13), (3, 1, 2))}
EPS = 2.0 ** -24  # a float rounding, relative


# ---------------------------------------------------------------- contexts
def assemble(m, steps=()):
    if steps:
        for ts in steps:
            m.time_step(ts)
    else:
        m.apply_bc_on_u(m.get_displacement(0))
        m.apply_bc_on_u(m.get_displacement(1))
    m.set_strains()
    m.homogenize()
    m.assembly_res()
    m.assembly_jac()
    return m


def grid_argv(g, procs=None, *more):
    a = ["-da_grid_x", g[0], "-da_grid_y", g[1], "-da_grid_z", g[2], "-bc_type", "0", "-ksp_rtol", "1e-8", "-ksp_monitor"]
    if procs:
        a += ["-da_processors_x", procs[0], "-da_processors_y", procs[1], "-da_processors_z", procs[2]]
    return a + list(more)


def csr_of(t, n):
    rp, ci, v = t
    return sp.csr_matrix((v, ci, rp), shape=(len(rp) - 1, n))


def fine_matrix(m):
    petsc, nat = m.owned_dofs()
    assert np.array_equal(petsc, nat)  # one rank: PETSc order is the natural order
    dmask = np.zeros(m.n, dtype=bool)
    dmask[m.dump_dirichlet()] = True
    return csr_of(m.dump_csr(), m.n), dmask


def dumps(m):
    """the operators of the levels >= 1 as the device holds them"""
    sizes = m.pc_mg_info()["nxyz"]
    return [csr_of(m.pc_mg_dump_csr(l), 3 * int(np.prod(sizes[l]))) for l in range(1, len(sizes))]


def same(a, b):
    """two sparse matrices: the same entries, bit for bit"""
    return a.shape == b.shape and (a != b).nnz == 0


def rel(a, b, keep=slice(None)):
    return np.linalg.norm((a - b)[keep]) / np.linalg.norm(b[keep])


class Case:
    pass


@pytest.fixture(scope="module", params=R.GRIDS, ids=lambda g: "x".join(map(str, g)))
def case(request):
    """one grid: a context that never heard of the option and one with it set to 1, both with pc_type 1"""
    k = Case()
    k.grid = request.param
    k.m = assemble(M.Macroc(grid_argv(k.grid)))
    k.m.set_option("pc_type", 1)
    k.ms = assemble(M.Macroc(grid_argv(k.grid)))
    k.ms.set_option("pc_mg_precision", 1)
    k.ms.set_option("pc_type", 1)
    k.A, k.dmask = fine_matrix(k.m)
    k.sizes, _, k.Ps = R.hierarchy(k.A, k.dmask, k.grid, False)  # the rule's P per level
    k.ops_d, k.ops_s = dumps(k.m), dumps(k.ms)
    k.info_d, k.info_s = k.m.pc_mg_info(), k.ms.pc_mg_info()
    yield k
    k.m.finish()
    k.ms.finish()


# ---------------------------------------------------------------- 1. the option
def test_option():
    with M.Macroc(grid_argv((9, 9, 9))) as m:
        assemble(m)
        assert m.pc_mg_precision() == 0
        for bad in (2, -1, 0.5):
            with pytest.raises(M.MacrocError, match=r"failed \(1\).*pc_mg_precision: 0 \(double.*1 \(single"):
                m.set_option("pc_mg_precision", bad)
        assert m.pc_mg_precision() == 0
        m.set_option("pc_type", 1)
        before = m.get_info()["device_bytes"]
        bytes_d = m.pc_mg_info()["bytes"]
        assert m.get_info()["device_bytes"] == before + bytes_d
        m.set_option("pc_mg_precision", 0)  # the value it has: nothing happens
        assert m.get_info()["device_bytes"] == before + bytes_d
        m.set_option("pc_mg_precision", 1)  # the hierarchy is freed ...
        assert m.pc_mg_precision() == 1 and m.get_info()["device_bytes"] == before
        bytes_s = m.pc_mg_info()["bytes"]  # ... and built again
        assert 0 < bytes_s < bytes_d and m.get_info()["device_bytes"] == before + bytes_s
        assert m.solve_Ax()[2] == 2
        m.set_option("pc_mg_precision", 0)
        assert m.get_info()["device_bytes"] == before
        assert m.pc_mg_info()["bytes"] == bytes_d
    with M.Macroc(grid_argv((9, 9, 9), None, "-pc_mg_precision", "single", "-pc_type", "mg")) as m:
        assert m.pc_mg_precision() == 1


# ---------------------------------------------------------------- 2. double keeps its bits
def test_double_keeps_its_bits(case):
    """never set, set to 0, and toggled 1 -> 0 over a built float hierarchy: one hierarchy, bit for bit"""
    r = np.random.default_rng(11).standard_normal(case.m.n)

    def everything(m):
        z, info = m.pc_apply(r), m.pc_mg_info()
        return z, dumps(m), info["lmax"], m.solve_Ax(), m.du()

    want = everything(case.m)
    for toggle in (False, True):
        with M.Macroc(grid_argv(case.grid)) as m:
            assemble(m)
            m.set_option("pc_type", 1)
            if toggle:
                m.set_option("pc_mg_precision", 1)
                assert m.pc_mg_info()["bytes"] == case.info_s["bytes"]
            m.set_option("pc_mg_precision", 0)
            got = everything(m)
            assert m.pc_mg_info()["bytes"] == case.info_d["bytes"]
        assert np.array_equal(got[0], want[0])
        assert len(got[1]) == len(want[1]) and all(same(a, b) for a, b in zip(got[1], want[1]))
        assert np.array_equal(got[2], want[2])
        assert got[3] == want[3] and np.array_equal(got[4], want[4])


# ---------------------------------------------------------------- 3. level 1
def check_level1(md, ms):
    sizes = md.pc_mg_info()["nxyz"]
    n1 = 3 * int(np.prod(sizes[1]))
    d, s = csr_of(md.pc_mg_dump_csr(1), n1), csr_of(ms.pc_mg_dump_csr(1), n1)
    assert np.array_equal(d.indptr, s.indptr) and np.array_equal(d.indices, s.indices)
    assert np.array_equal(s.data, R.f32(d.data))  # fl32 of the double operator, entry for entry
    assert not np.array_equal(s.data, d.data)  # and it is not the double one


def test_level1_aij(case):
    check_level1(case.m, case.ms)


def pair(argv, steps=()):
    out = []
    for single in (0, 1):
        m = assemble(M.Macroc(argv), steps)
        m.set_option("pc_mg_precision", single)
        m.set_option("pc_type", 1)
        out.append(m)
    return out


def test_level1_sbaij():
    md, ms = pair(grid_argv((24, 9, 13), None, "-dm_mat_type", "sbaij"))
    try:
        check_level1(md, ms)
    finally:
        md.finish()
        ms.finish()


def test_level1_plastic_with_exception_nodes():
    md, ms = pair(PLASTIC, steps=(0, 1))
    try:
        assert ms.nonlinear_stats()[0] > 0 and ms.get_info()["vi_exc_nodes"] > 0
        check_level1(md, ms)
    finally:
        md.finish()
        ms.finish()


# ---------------------------------------------------------------- 4. deeper levels
def test_deeper_levels(case):
    """A_{l+1} against P^T A_l P of the dumped float A_l, formed in double.  The device rounds the
    stored A_l P e (relative to sum |A_l| |P e|) and the restricted result (relative to its own size,
    at most |P|^T |A_l| |P|); one more rounding as the margin: 4 * 2^-24 covers (1 + eps)^3 - 1"""
    for l in range(len(case.ops_s)):
        v = case.ops_s[l].data
        assert np.array_equal(v, R.f32(v))  # float values
    for l in range(1, len(case.ops_s)):
        Al, P = case.ops_s[l - 1], case.Ps[l]
        want, _ = R.unit_on_empty((P.T @ Al @ P).tocsr())
        bound = (abs(P).T @ abs(Al) @ abs(P)).toarray()
        err = abs(case.ops_s[l] - want).toarray()
        worst = (err / np.where(bound > 0, bound, 1.0)).max()
        print(f"{case.grid} level {l + 1}: max |A - P^T A P| / (|P|^T |A| |P|) = {worst / EPS:.3f} x 2^-24")
        assert np.all(err <= 4 * EPS * bound)


# ---------------------------------------------------------------- 5. the cycle
def test_cycle(case):
    free = ~case.dmask
    r = np.random.default_rng(11).standard_normal(case.m.n)
    for k in (2, 3):
        case.m.set_option("pc_mg_smooth", k)
        case.ms.set_option("pc_mg_smooth", k)
        zd, zs = case.m.pc_apply(r), case.ms.pc_apply(r)
        nd = R.vcycle([case.A] + case.ops_d, case.Ps, case.info_d["lmax"], 0, r, k, False)
        ns = R.vcycle([case.A] + case.ops_s, case.Ps, case.info_s["lmax"], 0, r, k, True)
        e = rel(ns, nd, free)  # e': single against double, of the reference
        e_ref, e_dev, e_dbl = rel(zs, ns, free), rel(zs, zd, free), rel(zd, nd, free)
        print(f"{case.grid} V({k},{k}): e' = {e:.3e}; device single against numpy single {e_ref:.3e}, against the "
              f"device's double {e_dev:.3e}; device double against numpy double {e_dbl:.3e}")
        assert e > 0
        assert e_ref <= 10 * e and e_dev <= 10 * e
        assert not np.array_equal(zs, zd)  # the float path ran
        assert np.array_equal(case.ms.pc_apply(r), zs)  # the same bits again
    case.m.set_option("pc_mg_smooth", 2)
    case.ms.set_option("pc_mg_smooth", 2)


# ---------------------------------------------------------------- 6. symmetric positive
def test_operator_symmetric_positive(case):
    asym, pos = R.asymmetry(case.ms.pc_apply, ~case.dmask, case.m.n)  # the reference's four pairs
    print(f"{case.grid}: largest |u.Mv - v.Mu| / |u.Mv| of four pairs = {max(asym):.3e} "
          f"(the reference's largest: {R.REF_ASYM[case.grid]:.3e}); pairs: {asym}")
    assert pos > 0
    assert max(asym) <= 10 * R.REF_ASYM[case.grid]


# ---------------------------------------------------------------- 7. the solve
def test_solve(case):
    b = case.m.b()
    its_d, _, reason_d = case.m.solve_Ax()
    du_d = case.m.du()
    its, rnorm, reason = case.ms.solve_Ax()
    du, hist = case.ms.du(), case.ms.ksp_history()
    err, res = rel(du, du_d), np.linalg.norm(b - case.A @ du) / np.linalg.norm(b)
    print(f"{case.grid}: its double {its_d}, single {its}, |du_s - du_d|/|du_d| = {err:.3e}, |b - A du|/|b| = {res:.3e}")
    assert reason == 2 and reason_d == 2
    assert res <= 10 * 1e-8
    assert err <= 1e-6
    assert its <= its_d + 1
    assert len(hist) == its + 1 and hist[-1] == rnorm
    its2, rnorm2, _ = case.ms.solve_Ax()
    assert (its2, rnorm2) == (its, rnorm) and np.array_equal(case.ms.du(), du)


def test_solve_tight():
    """17^3 at -ksp_rtol 1e-12: float rounding makes M^-1 non-linear at the 1e-7 level, which may delay
    the PCG by a few iterations but not stall it"""
    md, ms = pair(grid_argv((17, 17, 17), None, "-ksp_rtol", "1e-12"))
    try:
        A, b = fine_matrix(md)[0], md.b()
        its_d, _, reason_d = md.solve_Ax()
        its, _, reason = ms.solve_Ax()
        res = np.linalg.norm(b - A @ ms.du()) / np.linalg.norm(b)
        print(f"rtol 1e-12: its double {its_d}, single {its}, |b - A du|/|b| = {res:.3e}")
        assert reason == 2 and reason_d == 2
        assert res <= 10 * 1e-12
        assert its <= its_d + max(2, its_d / 4)
    finally:
        md.finish()
        ms.finish()


# ---------------------------------------------------------------- 8. Newton
def test_newton_plastic_matches_jacobi():
    out = []
    for pc in (["-pc_type", "jacobi"], ["-pc_type", "mg", "-pc_mg_precision", "single"]):
        with M.Macroc(PLASTIC + pc) as m:
            m.time_step(0)
            r = m.time_step(1)
            out.append((r, m.u(), m.pc_mg_precision()))
    (rj, uj, _), (rm, um, single) = out
    print("jacobi:", rj, "\nmg, single:", rm)
    assert single == 1
    assert rj["newton_its"] == rm["newton_its"] >= 2
    np.testing.assert_allclose(rm["res"], rj["res"], rtol=1e-6)
    assert max(rm["ksp_its"]) < min(rj["ksp_its"])
    assert np.linalg.norm(um - uj) <= 1e-8 * np.linalg.norm(uj)


# ---------------------------------------------------------------- 9. memory
def test_memory():
    m = assemble(M.Macroc(grid_argv((17, 17, 17))))
    try:
        before = m.get_info()["device_bytes"]
        nbytes = []
        for single in (0, 1):
            m.set_option("pc_mg_precision", single)
            m.set_option("pc_type", 1)
            m.pc_apply(np.ones(m.n))
            nbytes.append(m.pc_mg_info()["bytes"])
            assert m.get_info()["device_bytes"] == before + nbytes[-1]
            m.set_option("pc_type", 0)
            assert m.get_info()["device_bytes"] == before
        print("hierarchy bytes: double", nbytes[0], " single", nbytes[1])
        assert nbytes[0] - nbytes[1] >= 4 * 243 * (9 ** 3 + 5 ** 3)  # the operators alone
    finally:
        m.finish()


# ---------------------------------------------------------------- 10. the driver
def test_driver_takes_the_flag(tmp_path):
    exe = os.path.join(ROOT, "macroc_amd", "driver", "macroc_amd")
    argv = [exe, "-da_grid_x", "17", "-da_grid_y", "17", "-da_grid_z", "17", "-ts", "2", "-bc_type", "0",
            "-ksp_rtol", "1e-8", "-pc_type", "mg"]
    its = []
    for word in ("double", "single"):
        out = subprocess.run(argv + ["-pc_mg_precision", word], cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "not used" not in out.stderr and "Elapsed time" in out.stdout
        its.append([int(v) for v in re.findall(r"Its = (\d+)", out.stdout)])
    assert its[0] and len(its[0]) == len(its[1])
    assert all(abs(a - b) <= 1 for a, b in zip(its[0], its[1])), its
    out = subprocess.run(argv + ["-pc_mg_precision", "half"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    text = out.stdout + out.stderr
    assert out.returncode != 0 and "double or single" in text and "half" in text


# ---------------------------------------------------------------- 11. pc_mg_dist, in process
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


def measure(m, rvec):
    """what the tests compare, of one rank of a group (or of a one-rank context with a communicator)"""
    o = {}
    assemble(m)
    o["nat"] = m.owned_dofs()[1]
    r = rvec[o["nat"]]
    o["bytes0"] = m.get_info()["device_bytes"]
    m.set_option("pc_mg_dist", 1)
    m.set_option("pc_mg_precision", 1)
    m.set_option("pc_type", 1)
    o["z"] = m.pc_apply(r)
    assert np.array_equal(m.pc_apply(r), o["z"])  # the same bits again
    o["info"] = m.pc_mg_info()
    o["bytes1"] = m.get_info()["device_bytes"]
    o["boxes"] = [m.pc_mg_box(l) for l in range(o["info"]["levels"])]
    o["ops"] = [m.pc_mg_dump_csr(l) for l in range(1, o["info"]["levels"])]
    o["solve"] = m.solve_Ax()
    o["du"], o["hist"] = m.du(), m.ksp_history()
    assert m.solve_Ax() == o["solve"] and np.array_equal(m.du(), o["du"])  # a second solve: the same bits
    m.set_option("pc_type", 0)
    o["bytes2"] = m.get_info()["device_bytes"]
    return o


class Ref:
    """the one-rank contexts on the grid: the float hierarchy the ranks are held against, and e' from
    the numpy cycles on the dumped double and float operators"""

    def __init__(self, grid):
        n = 3 * int(np.prod(grid))
        self.rvec = np.random.default_rng(11).standard_normal(n)
        md, ms = pair(grid_argv(grid))
        try:
            A, self.dmask = fine_matrix(md)
            self.sizes, _, Ps = R.hierarchy(A, self.dmask, grid, False)
            self.ops = dumps(ms)
            self.info = ms.pc_mg_info()
            self.z = ms.pc_apply(self.rvec)
            nd = R.vcycle([A] + dumps(md), Ps, md.pc_mg_info()["lmax"], 0, self.rvec, 2, False)
            ns = R.vcycle([A] + self.ops, Ps, self.info["lmax"], 0, self.rvec, 2, True)
            self.e = rel(ns, nd, ~self.dmask)
            self.solve, self.du = ms.solve_Ax(), ms.du()
        finally:
            md.finish()
            ms.finish()


def gathered(outs, key, n):
    v = np.zeros(n)
    for o in outs:
        v[o["nat"]] = o[key]
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
        loc = csr_of(o["ops"][l - 1], n).tocoo()
        A = A + sp.csr_matrix((loc.data, (rows[loc.row], loc.col)), shape=(n, n))
        rows_seen[rows] += 1
    assert np.all(rows_seen == 1)
    return A.tocsr()


@pytest.fixture(scope="module", params=list(DIST))
def dist(request):
    k = Case()
    k.name = request.param
    k.grid, k.procs = DIST[request.param]
    k.nr, k.n = int(np.prod(k.procs)), 3 * int(np.prod(k.grid))
    k.ref = Ref(k.grid)
    k.outs, errors = run_group(grid_argv(k.grid, k.procs), k.nr, lambda m: measure(m, k.ref.rvec))
    assert not errors, errors
    return k


def test_dist_operators_and_estimates(dist):
    ref, outs = dist.ref, dist.outs
    for l in range(1, len(ref.sizes)):
        assert same(assembled_by_box(outs, l, ref.sizes), ref.ops[l - 1]), l  # the one-rank dump, bit for bit
    # lmax: the same bits on every rank, so every rank takes the same branch.  A limit: against one rank
    # it is not the same bits, because the norm's partial sums go by rank (the same operator
    # up to the summation order of the dot products), already on the untouched double level 0.  Every
    # level is held to the double hierarchy's bar for this comparison, 1e-12 (tests/test_gpu_pcmg_dist.py)
    l0, l1 = outs[0]["info"]["lmax"], ref.info["lmax"]
    for o in outs:
        assert np.array_equal(o["info"]["lmax"], l0)
    print(f"{dist.name}: lmax {l0}, one rank {l1}, relative difference {abs(l0 - l1) / np.where(l1 > 0, l1, 1.0)}")
    assert l0[-1] == 0.0 and np.all(abs(l0 - l1) <= 1e-12 * abs(l1))


def test_dist_cycle(dist):
    z = gathered(dist.outs, "z", dist.n)
    err = rel(z, dist.ref.z, ~dist.ref.dmask)
    print(f"{dist.name}: |z - z_1| / |z_1| on the free dofs = {err:.3e}, e' = {dist.ref.e:.3e}")
    assert dist.ref.e > 0 and err <= 10 * dist.ref.e


def test_dist_solve(dist):
    ref, outs = dist.ref, dist.outs
    its, rnorm, reason = outs[0]["solve"]
    for o in outs:  # iterations, rnorm and history identical on every rank
        assert o["solve"] == outs[0]["solve"] and np.array_equal(o["hist"], outs[0]["hist"])
    err = rel(gathered(outs, "du", dist.n), ref.du)
    print(f"{dist.name}: one-rank its {ref.solve[0]}, {dist.nr}-rank its {its}, |du - du_1|/|du_1| = {err:.3e}")
    assert reason == 2 and ref.solve[2] == 2
    assert abs(its - ref.solve[0]) <= 1
    assert err <= 1e-6
    assert len(outs[0]["hist"]) == its + 1 and outs[0]["hist"][-1] == rnorm


def test_dist_device_bytes_count_the_hierarchy(dist):
    for o in dist.outs:
        n1 = int(np.prod(o["boxes"][1][1]))  # the rank's box of level 1
        assert o["info"]["bytes"] >= 4 * 243 * n1
        assert o["bytes1"] == o["bytes0"] + o["info"]["bytes"]
        assert o["bytes2"] == o["bytes0"]


def test_one_rank_keeps_its_bits():
    """pc_mg_dist on a context without a communicator changes nothing: the one-rank float hierarchy's bits"""
    grid = (17, 17, 17)
    ref = Ref(grid)
    with M.Macroc(grid_argv(grid)) as m:
        o = measure(m, ref.rvec)
    assert o["solve"] == ref.solve and np.array_equal(o["du"], ref.du)
    assert np.array_equal(o["z"], ref.z)
    assert np.array_equal(o["info"]["lmax"], ref.info["lmax"])


def test_one_rank_rccl_communicator():
    """a one-rank RCCL communicator: the distributed path (all-reduces through RCCL, no neighbour) in
    float.  With one rank no sum goes by rank, so it gives the one-rank hierarchy's bits"""
    grid = (17, 17, 17)
    ref = Ref(grid)
    with M.Macroc(grid_argv(grid), rank=0, nranks=1, comm_id=M.comm_unique_id()) as m:
        o = measure(m, ref.rvec)
        assert m.pc_mg_precision() == 1
    print(f"one-rank communicator: solve {o['solve']}, one rank {ref.solve}, lmax {o['info']['lmax']}, one rank "
          f"{ref.info['lmax']}, |z - z_1| / |z_1| = {rel(o['z'], ref.z):.3e}, |du - du_1| / |du_1| = {rel(o['du'], ref.du):.3e}")
    assert o["solve"][2] == 2 and o["solve"] == ref.solve
    assert np.array_equal(o["z"], ref.z) and np.array_equal(o["info"]["lmax"], ref.info["lmax"])
    assert np.array_equal(o["du"], ref.du)
    for l in range(1, len(ref.sizes)):
        assert same(csr_of(o["ops"][l - 1], 3 * int(np.prod(ref.sizes[l]))), ref.ops[l - 1])
