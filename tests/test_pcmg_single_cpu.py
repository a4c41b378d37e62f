"""-pc_mg_precision single without a GPU: the flag, the ABI, and the reference alone.

The reference (tests/pcmg_single_ref.py) builds, from the oracle's matrix, the hierarchy in double and
with its levels >= 1 stored in float, and runs the V-cycle and a PCG with both.  What it shows is what
the GPU tests (tests/test_gpu_pcmg_single.py) ask of the device: the two cycles differ (e' > 0, of
float size), the single one is symmetric positive to float rounding, and the PCG needs the double
hierarchy's iterations +- 1 at rtol 1e-8.  It also shows that 5 x 17 x 17, the grid whose float levels
have nx = 3 and 2, is a sound problem.  The numbers it prints are in DESIGN §17."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import macroc_amd as M
import pcmg_single_ref as R
from oracle import oracle as O


# ---------------------------------------------------------------- flags and ABI
def test_parse_args_takes_the_flag(capfd):
    for word in ("double", "single"):
        o = M.parse_args(["-da_grid_x", "17", "-pc_type", "mg", "-pc_mg_precision", word, "-ksp_rtol", "1e-8"])
        assert o.NX == 17 and o.ksp_rtol == 1e-8  # the flags around it are still read
    assert "not used" not in capfd.readouterr().err


@pytest.mark.parametrize("word", ["half", "1", None])
def test_a_wrong_word_fails_with_code_2(word):
    argv = ["-da_grid_x", "17", "-pc_mg_precision"] + ([word] if word else [])
    with pytest.raises(M.MacrocError, match=r"failed \(2\).*-pc_mg_precision: double or single, got " +
                       (word or r"\(none\)")):
        M.parse_args(argv)


def test_abi_revision_and_opts_layout_unchanged():
    assert M.lib().mcx_abi_version() == 3 == M.ABI_VERSION
    assert C.sizeof(M.Opts) == 264


def test_the_new_entry_refuses_a_null_context():
    L = M.lib()
    single = C.c_int(7)
    assert L.mcx_pc_mg_get_precision(None, C.byref(single)) == 1 and single.value == 7
    assert L.mcx_set_option(None, b"pc_mg_precision", 1.0) != 0
    assert "mcx_pc_mg_get_precision" in M.EXPORTS


# ---------------------------------------------------------------- the reference alone
def oracle_system(grid, rtol=1e-8):
    """the Newton system of time step 1 under -bc_type 0: (A, b, the Dirichlet mask), natural order"""
    P = O.Problem(*grid, bc_type=O.BC_BENDING, rtol=rtol)
    P.apply_bc_u(P.get_displacement(0))
    P.apply_bc_u(P.get_displacement(1))
    P.set_strains()
    P.homogenize()
    b = P.assembly_res()
    P.assembly_jac()
    rp, ci = P.csr()
    A = sp.csr_matrix((P.A_values(), ci, rp), shape=(P.ndofs, P.ndofs))
    dmask = np.zeros(P.ndofs, dtype=bool)
    dmask[P.dirichlet_set()] = True
    P.close()
    return A, b, dmask


@pytest.fixture(scope="module", params=R.GRIDS, ids=lambda g: "x".join(map(str, g)))
def ref(request):
    grid = request.param
    A, b, dmask = oracle_system(grid)
    out = {"grid": grid, "A": A, "b": b, "dmask": dmask}
    for single in (False, True):
        sizes, ops, Ps = R.hierarchy(A, dmask, grid, single)
        out[single] = (sizes, ops, Ps, R.estimates(ops, single))
    return out


def cycle_of(ref, single, k=2):
    _, ops, Ps, lmax = ref[single]
    return lambda r: R.vcycle(ops, Ps, lmax, 0, r, k, single)


def test_the_problem_is_sound(ref):
    """a symmetric matrix with a positive diagonal, a right-hand side, float levels where the issue
    puts them, and operators that are float values"""
    A, b = ref["A"], ref["b"]
    assert abs(A - A.T).max() <= 1e-12 * abs(A).max() and A.diagonal().min() > 0 and np.linalg.norm(b) > 0
    sizes, ops, _, lmax = ref[True]
    assert len(sizes) >= 3 and sizes == ref[False][0]
    if ref["grid"] == (5, 17, 17):
        assert sizes == [(5, 17, 17), (3, 9, 9), (2, 5, 5)]  # nx <= 3 on every float level
    for l in range(1, len(ops)):
        assert np.array_equal(ops[l].data, R.f32(ops[l].data))
    assert np.array_equal(ops[1].toarray(), R.f32(ref[False][1][1].toarray()))  # level 1: the double one, rounded
    assert np.all(lmax[:-1] > 1.0) and np.all(lmax[:-1] < 81.0) and lmax[-1] == 0.0


def test_single_against_double(ref):
    """e', the two iteration counts and the asymmetry of the reference"""
    A, b, free = ref["A"], ref["b"], ~ref["dmask"]
    n = A.shape[0]
    r = np.random.default_rng(11).standard_normal(n)
    for k in (2, 3):
        zd, zs = cycle_of(ref, False, k)(r), cycle_of(ref, True, k)(r)
        e = np.linalg.norm((zs - zd)[free]) / np.linalg.norm(zd[free])
        print(f"{ref['grid']} V({k},{k}): e' = |z_s - z_d| / |z_d| on the free dofs = {e:.3e}")
        assert e > 0.0  # float rounding (2^-24 = 6e-8) through the cycle's stores, times the levels' conditioning
        assert np.array_equal(cycle_of(ref, True, k)(r), zs)
    its_d, xd, _ = R.pcg(A, b, cycle_of(ref, False), 1e-8)
    its_s, xs, hist = R.pcg(A, b, cycle_of(ref, True), 1e-8)
    du = np.linalg.norm(xs - xd) / np.linalg.norm(xd)
    res = np.linalg.norm(b - A @ xs) / np.linalg.norm(b)
    print(f"{ref['grid']}: PCG its double {its_d}, single {its_s}, |du_s - du_d| / |du_d| = {du:.3e}, "
          f"|b - A du_s| / |b| = {res:.3e}")
    assert abs(its_s - its_d) <= 1 and hist[-1] <= 1e-8 * hist[0]
    assert du <= 1e-6 and res <= 1e-7
    asym_d, pos_d = R.asymmetry(cycle_of(ref, False), free, n)
    asym_s, pos_s = R.asymmetry(cycle_of(ref, True), free, n)
    print(f"{ref['grid']}: asymmetry double {max(asym_d):.3e}, single {max(asym_s):.3e} (pairs: {asym_s})")
    assert pos_d > 0 and pos_s > 0
    assert max(asym_d) <= 1e-12  # the bar of tests/test_gpu_pcmg.py
    # float rounding, far above the double cycle's; within the bar the GPU test gives the device
    assert max(asym_d) < max(asym_s) <= 10 * R.REF_ASYM[ref["grid"]], (max(asym_s), R.REF_ASYM[ref["grid"]])


def test_single_at_a_tight_tolerance():
    """17^3 at rtol 1e-12: the count the GPU test compares its own two counts with"""
    A, b, dmask = oracle_system((17, 17, 17), rtol=1e-12)
    its = {}
    for single in (False, True):
        sizes, ops, Ps = R.hierarchy(A, dmask, (17, 17, 17), single)
        lmax = R.estimates(ops, single)
        its[single], x, hist = R.pcg(A, b, lambda r: R.vcycle(ops, Ps, lmax, 0, r, 2, single), 1e-12)
        res = np.linalg.norm(b - A @ x) / np.linalg.norm(b)
        print(f"rtol 1e-12, single {single}: its {its[single]}, |b - A du| / |b| = {res:.3e}")
        assert hist[-1] <= 1e-12 * hist[0] and res <= 1e-11
    assert its[True] <= its[False] + max(2, its[False] / 4)
