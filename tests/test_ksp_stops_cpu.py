"""The stop-reason table (tests/ksp_stop_cases.py) proven on the CPU: every row is solved by the oracle
and by the numpy restatement of KSPSolve_CG; both give the table's (its, reason) and the same
iterate, and the margins hold that let tests/test_gpu_ksp_stops.py demand the exact iteration count
from a CG whose dot products are summed in another order."""
import numpy as np
import pytest

import ksp_stop_cases as K
from oracle import oracle as O

CASES = K.ALL_GRIDS_CASES


def check_case(case):
    P, out = K.oracle_case(case)
    c = K.restated(P)
    du = P.du()
    P.close()
    assert (out["its"], out["reason"]) == (c["its"], c["reason"]) == (case.its, case.reason)
    assert len(c["history"]) == K.norms_computed(case.its, case.reason)
    assert np.linalg.norm(c["x"] - du) <= 1e-11 * np.linalg.norm(du)
    assert K.same_rnorm(c["rnorm"], out["rnorm"])
    np.testing.assert_allclose(c["history"], out["history"], rtol=1e-9)
    if case.its == 0:
        assert not du.any() and not c["x"].any()
    else:
        assert np.linalg.norm(du) > 0
    if case.kind == "indef":
        i = case.its - 1
        assert i >= 1
        m = c["pap_margin"]
        assert len(m) == case.its and min(m[i - 1], m[i]) >= K.PAP_MARGIN, m
        assert c["pap"][i] * c["pap"][i - 1] < 0  # the sign change itself, not p.Ap == 0
        assert all(a * b > 0 for a, b in zip(c["pap"][:i - 1], c["pap"][1:i]))  # and the first one
        # the Jacobi diagonal stays usable (one sign on the free rows): z.r never changes sign, no INDEFINITE_PC
        assert all(v * c["zr"][0] > 0 for v in c["zr"])
    return c


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_table_row(case):
    c = check_case(case)
    if case.kind == "nan":
        want = {"nan": np.isnan, "inf": np.isnan, "big": np.isinf}[case.poison]
        assert want(c["rnorm"])


@pytest.mark.parametrize("grid", ["g8", "g20", "g70", "g12"])
def test_threshold_gaps(grid):
    """-ksp_divtol / -ksp_atol sit at the geometric mean of two history entries at least GAP apart,
    and no earlier entry crosses them."""
    h = K.base_history(grid, O.BC_BENDING, K.DTOL_NU)
    r = h / h[0]
    for k in K.DTOL_K[grid]:
        t = K.dtol_threshold(grid, k)
        assert r[k] / r[k - 1] >= K.GAP and r[k - 1] < t < r[k]
        assert np.all(r[:k] * np.sqrt(K.GAP) <= t * (1 + 1e-12))
    h = K.base_history(grid, O.BC_CIRCLE, 0.25)
    for k in K.ATOL_K[grid]:
        t = K.atol_threshold(grid, k)
        assert h[k - 1] / h[k] >= K.GAP and h[k] < t < h[k - 1]
        assert np.all(h[:k] >= t * np.sqrt(K.GAP) * (1 - 1e-12))


def test_dtol_history_rises():
    """The rising ratios h[k] / h[0] the DTOL rows are built on (three significant digits)."""
    want = {"g8": [4.22, 6.78, 10.3, 13.6, 17.9, 19.7, 21.5, 19.6],
            "g20": [5.42, 8.78, 13.5, 17.7, 21.6, 23.2, 24.3, 20.5],
            "g70": [7.28, 11.8, 18.0, 23.1, 25.5, 25.8, 25.7, 19.6]}
    for grid, w in want.items():
        h = K.base_history(grid, O.BC_BENDING, K.DTOL_NU)
        np.testing.assert_allclose(h[1:9] / h[0], w, rtol=6e-3)


@pytest.mark.parametrize("grid", ["g20", "g12"])
def test_decomposed_rows(grid):
    """The rows of the decomposed runs; 12x10x14's are derived by the rule of the literal ones."""
    cases = K.decomposed_cases(grid)
    assert [c.kind for c in cases] == ["indef", "indef", "dtol", "dtol", "atol", "nan"]
    assert (cases[0].its - cases[1].its) % 4 and cases[1].its > 4
    if grid == "g12":
        for case in cases:
            check_case(case)
