"""The sparse cell reference (tests/micro_cell_sparse_ref.py) and the fixtures it wrote (tests/golden/cell_*.npz,
by tests/golden/make_micro_cells.py), checked without a GPU.

1. SparseCellRef against the dense TN.CellRef where both run: the same definition with other linear algebra,
   so sigma, C, C_hom and f_max agree to rounding (1e-12 of the largest entry; measured 4e-16 at n = 6, the
   margin is for the sparse assembly's other summation order), path and Newton count are equal, kappa agrees to
   the eigsh tolerance.
2. Every committed fixture is internally sound: the conditions under which the reference is a fair judge hold
   as recorded, C and C_hom are symmetric, C_hom lies between the Reuss and Voigt bounds, and the fixtures that
   are there for a partial yield front have one.
3. (slow) stage 1.0 of cell_s21_a regenerated and compared with the fixture.
"""
import functools
import glob
import os

import numpy as np
import pytest

import test_gpu_micro as TM
import test_gpu_micro_nl as TN
from micro_cell_sparse_ref import SparseCellRef

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
README_MATS = ((1.0e7, 0.25, 7.6e3, 1.0e8), (1.0e8, 0.3, 1.0e9, 1.0e7))
MATS = {"project": (TN.MAT1, TN.MAT2), "readme": README_MATS}
CELLS = [(0, 4), (0, 5), (0, 9), (1, 3), (1, 9)]
LOAD = (5, 4e-3)
FIXTURES = ("cell_s21_a", "cell_s26_a", "cell_s26_b", "cell_l21_a")
PARTIAL = ("cell_s21_a", "cell_s26_b")  # a yield front runs through the matrix in at least one stage
ROUND = 1e-12


@functools.lru_cache(maxsize=None)
def fixture(name):
    with np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max()


# ---------------------------------------------------------------- 1. sparse against dense
@pytest.mark.parametrize("mats", sorted(MATS))
@pytest.mark.parametrize("typ,n", CELLS)
def test_sparse_against_dense(typ, n, mats):
    dense, sparse = TN.CellRef(typ, n, *MATS[mats]), SparseCellRef(typ, n, *MATS[mats])
    assert np.array_equal(dense.ph, sparse.ph)
    assert rel(sparse.Chom, dense.Chom) <= ROUND
    kl = TM.reference(typ, n, MATS[mats][0][:2], MATS[mats][1][:2])[1]  # the linear law's own dense reference
    assert abs(sparse.kappa_lin - kl) <= 1e-6 * kl
    e0 = LOAD[1] * np.random.default_rng(LOAD[0]).uniform(-1, 1, 6)
    hd = hs = None
    for fac in TN.STAGES:
        d, s = dense.point(fac * e0, hd), sparse.point(fac * e0, hs)
        es, ec = rel(s["sig"], d["sig"]), rel(s["C"], d["C"])
        ef = abs(s["fmax"] - d["fmax"]) / d["strial"]  # f is a difference of two numbers of the trial stress's size
        ek = abs(s["kappa"] - d["kappa"]) / d["kappa"]
        print(f"cell ({typ},{n}) {mats} stage {fac}: sigma {es:.1e} C {ec:.1e} f {ef:.1e} kappa {d['kappa']:.6f} d {ek:.1e} "
              f"its {d['its']} / {s['its']} nplastic {s['nplastic']} of {sparse.matrix_points()}")
        assert d["path"] == s["path"] == 1 and d["its"] == s["its"]
        assert es <= ROUND and ec <= ROUND and ef <= ROUND and ek <= 1e-6
        assert abs(s["margin"] - d["margin"]) <= ROUND * d["strial"] / sparse.Sy.min()
        assert (s["nplastic"] > 0) == (d["fmax"] > 0) and 0 <= s["nplastic"] <= sparse.matrix_points()
        hd, hs = d["h"], s["h"]  # each goes on from its own history: a difference would show in the next stage


def test_flip_inverts_one_element():
    a, b = SparseCellRef(0, 5, *README_MATS), SparseCellRef(0, 5, *README_MATS, flip=[(3, 3, 0)])
    d = np.flatnonzero(a.ph != b.ph)
    assert d.tolist() == [3 + 4 * 3] and a.ph[d[0]] == 0 and b.ph[d[0]] == 1
    assert b.matrix_points() == a.matrix_points() - 8
    assert rel(b.Chom, a.Chom) > 1e-6  # every derived quantity follows the changed map


# ---------------------------------------------------------------- 2. the committed fixtures
def test_fixtures_are_all_there():
    have = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "cell_*.npz")))
    assert have == sorted(FIXTURES)


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_is_sound(name):
    fx = fixture(name)
    assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < 16384
    typ, n = int(fx["typ"]), int(fx["n"])
    assert (typ, n) == ({"s": 0, "l": 1}[name[5]], int(name[6:8]))
    assert tuple(fx["mat1"]) == README_MATS[0] and tuple(fx["mat2"]) == README_MATS[1]
    assert np.array_equal(fx["stages"], TN.STAGES) and float(fx["amp"]) in fx["amps_tried"]
    assert np.array_equal(fx["e0"], float(fx["amp"]) * np.random.default_rng(int(fx["seed"])).uniform(-1, 1, 6))
    # what TN.field gives all eight Gauss points of the 2x2x2 grid, but for the last bits of B u
    assert int(fx["seed"]) == 5
    ph = TN.phase_rule(typ, n)
    assert int(fx["phase1"]) == int(ph.sum()) and int(fx["matrix_points"]) == 8 * int((ph == 0).sum())
    for st in range(len(TN.STAGES)):
        r = {k: fx[k][st] for k in ("its", "margin", "mlin", "path", "kappa", "nplastic", "fmax")}
        TN.check_conditions(r)
        assert r["path"] == 1 and r["kappa"] >= 1.0 and 0 <= r["nplastic"] <= fx["matrix_points"]
        assert (r["fmax"] > 0) == (r["nplastic"] > 0)
        C = fx["C"][st]
        assert np.array_equal(C, C.T) and np.linalg.eigvalsh(C).min() > 0 and np.isfinite(fx["sig"][st]).all()
    assert fx["nplastic"][0] > 0 and fx["nplastic"][2] == 0  # the load yields; the unload to 0.5 is elastic
    Ch = fx["Chom"]
    assert np.array_equal(Ch, Ch.T)
    f1 = float(fx["phase1"]) / (n - 1) ** 3
    C1, C2 = TM.iso_C(*fx["mat1"][:2]), TM.iso_C(*fx["mat2"][:2])
    voigt = (1.0 - f1) * C1 + f1 * C2
    reuss = np.linalg.inv((1.0 - f1) * np.linalg.inv(C1) + f1 * np.linalg.inv(C2))
    for q in range(6):
        assert reuss[q, q] < Ch[q, q] < voigt[q, q], (q, reuss[q, q], Ch[q, q], voigt[q, q])
    # an elastic unload's tangent is C_hom again, to the rounding of another factorisation
    assert rel(fx["C"][2], Ch) <= ROUND * float(fx["kappa_lin"])
    assert abs(fx["kappa"][2] - fx["kappa_lin"]) <= 1e-6 * fx["kappa_lin"]


@pytest.mark.parametrize("name", PARTIAL)
def test_fixture_has_a_partial_front(name):
    fx = fixture(name)
    assert ((0 < fx["nplastic"]) & (fx["nplastic"] < fx["matrix_points"])).any(), fx["nplastic"]
    assert 0 < fx["nplastic"][0] < fx["matrix_points"]


# ---------------------------------------------------------------- 3. regeneration
@pytest.mark.slow
def test_regenerate_stage_one_of_s21_a():
    fx = fixture("cell_s21_a")
    cell = SparseCellRef(int(fx["typ"]), int(fx["n"]), tuple(fx["mat1"]), tuple(fx["mat2"]))
    r = cell.point(fx["stages"][0] * fx["e0"], None)
    assert rel(cell.Chom, fx["Chom"]) <= 1e-10 and abs(cell.kappa_lin - fx["kappa_lin"]) <= 1e-6 * fx["kappa_lin"]
    assert rel(r["sig"], fx["sig"][0]) <= 1e-10 and rel(r["C"], fx["C"][0]) <= 1e-10
    assert abs(r["fmax"] - fx["fmax"][0]) <= 1e-10 * r["strial"]
    assert abs(r["kappa"] - fx["kappa"][0]) <= 1e-6 * r["kappa"]
    for k in ("its", "path", "nplastic"):
        assert r[k] == fx[k][0], k
    assert abs(r["margin"] - fx["margin"][0]) <= 1e-10 * r["strial"] / cell.Sy.min()
    assert abs(r["mlin"] - fx["mlin"][0]) <= 1e-10 * r["strial"] / cell.Sy.min()
