"""The re-assembly table (tests/reassembly_cases.py) proven on the CPU oracle: every state of every
sequence has the exception set the closed form gives, sits on the stated side of the 10 % / 30 % /
capacity thresholds with the stated margin, covers the stencil-class candidates it is said to cover,
and assembles to a finite matrix.  This is what keeps tests/test_gpu_matrix_reassembly.py from passing
vacuously."""
import functools

import numpy as np
import pytest

import reassembly_cases as R

STATES = {g: sorted({s.state for q in R.SEQUENCES.values() for s in q.steps}) for g in R.SEQ_GRIDS}
STATES["g130"] = sorted(set(STATES["g130"]) | {s.state for q in R.SEQUENCES_2R.values() for s in q.steps})
STATES["g17"] = sorted({s.state for s in R.MG_SEQUENCE.steps})
PAIRS = [(g, s) for g in R.GRIDS for s in STATES[g]]


@functools.lru_cache(maxsize=None)
def oracle_exc(grid, state):
    """(exception mask from the oracle's tangents, A_values all finite)"""
    cref = R.elastic_ctan(grid)
    P = R.move_oracle(grid, state)
    return R.exc_from_ctan(P.ctan(), cref, grid), bool(np.all(np.isfinite(P.A_values())))


@pytest.mark.parametrize("grid,state", PAIRS, ids=[f"{g}-{s}" for g, s in PAIRS])
def test_state_is_the_closed_form(grid, state):
    got, finite = oracle_exc(grid, state)
    want = R.closed_form_exc(grid, state)
    assert np.array_equal(got, want)
    assert int(want.sum()) == R.COUNTS[grid][state]
    assert finite
    u = R.bump_field(grid, state)
    assert np.count_nonzero(u) == 3 * len(R.bump_nodes(grid, state)) == 3 * len(set(R.bump_nodes(grid, state)))
    assert np.array_equal(u, R.bump_field(grid, state))  # a state met again: the same bits


SOLVED = [(g, s) for g in R.SEQ_GRIDS for s in STATES[g] if s in R.SOLVED and s != "empty"]


@pytest.mark.parametrize("grid,state", SOLVED, ids=[f"{g}-{s}" for g, s in SOLVED])
def test_solved_state_crosses_rtol_cleanly(grid, state):
    """The states whose solve the device test holds to the oracle's iteration count +- 1: the oracle
    converges, its history is SOLVE_GAP above the threshold two entries before the last, and the numpy
    restatement of the CG (another summation order) stops within one iteration of it."""
    import ksp_stop_cases as K

    P = R.move_oracle(grid, state)
    out = P.solve(history=True)
    h, its = out["history"], out["its"]
    assert out["reason"] == 2 and its > 100
    ttol = R.RTOL * h[0]
    assert h[its] <= ttol < h[its - 1] and h[its - 2] >= R.SOLVE_GAP * ttol, h[its - 2:its + 1] / ttol
    c = K.cg_petsc(K.matrix(P), P.b(), rtol=R.RTOL)
    assert c["reason"] == 2 and abs(c["its"] - its) <= 1, (c["its"], its)
    assert np.linalg.norm(c["x"] - P.du()) <= 50 * R.RTOL * np.linalg.norm(P.du())


def test_empty_state_has_no_residual():
    for grid in R.SEQ_GRIDS:
        P = R.move_oracle(grid, "empty")
        out = P.solve()
        assert not P.b().any() and out["its"] == 0 and out["reason"] > 0 and not P.du().any()


def side(frac, thr, margin):
    """-1 / +1: frac is below / above thr by the margin; 0: too close"""
    return -1 if frac <= thr * (1 - margin) else 1 if frac >= thr * (1 + margin) else 0


@pytest.mark.parametrize("grid", R.SEQ_GRIDS)
@pytest.mark.parametrize("name", list(R.SEQUENCES))
def test_sequence_thresholds(grid, name):
    """Every step's fraction against 10 % and the sequence's vi_exc_max, its count against the capacity
    the earlier steps left, and the storage the step states."""
    seq = R.SEQUENCES[name]
    NX, NY, NZ = R.GRIDS[grid]
    nown = NX * NY * NZ
    xld, declined, grew = 0, False, []
    for q, st in enumerate(seq.steps):
        nexc = R.COUNTS[grid][st.state]
        frac = nexc / nown
        if st.option and st.option[0] == "vi_exc_max":
            declined = False
        over = R.overflows(nexc, nown, seq.exc_max)
        if nexc:
            assert side(frac, R.ST_FRACTION, R.MARGIN[grid]) != 0, (st.state, frac)
            assert side(frac, seq.exc_max / 1000, R.MARGIN[grid]) == (1 if over else -1), (st.state, frac)
        want = "latched" if declined and not over else "fallback" if over else "vi"
        assert st.storage == want, (q, st, want)
        if over:
            declined = True
        if want == "vi":
            new = R.xld_after(xld, nexc, nown)
            if new != xld:
                grew.append(q)
            assert nexc <= new and new % 64 == 0
            xld = new
        if st.same_as is not None:
            assert seq.steps[st.same_as].state == st.state
    if seq.regrow:
        assert tuple(grew) == seq.regrow, grew
    if name == "regrow_shrink":  # `one` leaves 1,088 slots; plane_J5 does not fit them; the shrunk state keeps the larger capacity
        assert R.xld_after(0, 27, nown) == 1088 < R.COUNTS[grid]["plane_J5"] <= xld
    if name == "cross_10_percent":
        assert [R.st_auto(R.COUNTS[grid][s.state], nown) for s in seq.steps] == [True, False, True]
    if name.startswith("overflow"):
        assert [s.storage for s in seq.steps] == ["vi", "fallback", "latched", "vi"]
    if name == "appear_move_vanish":  # the moved cube shares no node with the old one
        assert not np.any(R.closed_form_exc(grid, "one") & R.closed_form_exc(grid, "moved"))


@pytest.mark.parametrize("grid", R.SEQ_GRIDS)
def test_candidates_covered(grid):
    """The candidate nodes restated from k_st_setup, and which of them each state's set holds."""
    n3 = R.GRIDS[grid]
    NX, NY, NZ = n3
    cands = R.class_candidates(n3)
    assert cands[0] == [(NX // 2, NY // 2, NZ // 2), (2, 2, 2), (NX - 3, NY - 3, NZ - 3), (2, NY - 3, NZ // 2),
                        (NX - 3, 2, NZ // 2)]
    assert cands[5] == [(NX // 2, NY // 2, 0), (2, 2, 0), (NX - 3, 2, 0), (2, NY - 3, 0), (NX - 3, NY - 3, 0)]
    assert cands[2] == [(NX - 1, NY // 2, NZ // 2), (NX - 1, 2, 2), (NX - 1, NY - 3, 2), (NX - 1, 2, NZ - 3),
                        (NX - 1, NY - 3, NZ - 3)]
    for c in range(7):
        assert len(set(cands[c])) == 5
        for (i, j, k) in cands[c]:  # on exactly the class's face
            on = [i == 0, i == NX - 1, j == 0, j == NY - 1, k == 0, k == NZ - 1]
            assert sum(on) == (1 if c else 0) and (c == 0 or on[c - 1])

    def covered(state, c):
        m = R.closed_form_exc(grid, state)
        return [bool(m[k, j, i]) for (i, j, k) in cands[c]]

    for state, c in R.CLASS_LOST.items():
        assert all(covered(state, c)), (state, c)
        for other in range(7):  # every other class keeps a candidate
            if other != c:
                assert not all(covered(state, other)), (state, other)
    assert covered("middle", 0) == [True, False, False, False, False]
    for state in ("one", "moved", "plane_J5", "plane_half", "corners"):  # the path stays on: the interior keeps a candidate
        assert not all(covered(state, 0)), state
    for c in range(7):  # `one` leaves every class a representative (on g130 it reaches the y-hi face's middle)
        assert not all(covered("one", c)) and sum(covered("one", c)) <= 1, c
    assert not any(covered("one", 0))
    # listed_model's premise: the candidates of the interior and of the two faces that get lost are not
    # next to a Dirichlet node; most of each of those faces is not listed before the class is lost
    on, nf, near = R.domain_masks(grid)
    for c in (0, 5, 2):
        assert not any(near[k, j, i] for (i, j, k) in cands[c]), c
    for state, c in R.CLASS_LOST.items():
        if c:
            face = on[c - 1] & (nf == 1)
            assert int((face & R.listed_model(grid, "one")).sum()) <= int(face.sum()) // 5
            assert np.all(R.listed_model(grid, state)[face])
    # corners: eight nodes each, all on two or three domain faces (edge / corner nodes)
    m = R.closed_form_exc(grid, "corners")
    kk, jj, ii = np.nonzero(m)
    nf = ((ii == 0) | (ii == NX - 1)).astype(int) + ((jj == 0) | (jj == NY - 1)) + ((kk == 0) | (kk == NZ - 1))
    assert len(ii) == 16 and np.all(nf <= 3) and np.count_nonzero(nf == 3) == 2


def test_two_rank_split():
    """(130, 9, 12) over (2, 1, 1): the oracle's decomposition puts the boundary between x = 64 and 65;
    every two-rank state's exception nodes split between the ranks as the table states, the zero and
    the over-the-limit ranks explicitly."""
    from oracle import oracle as O

    grid = "g130"
    NX, NY, NZ = R.GRIDS[grid]
    P2 = O.Problem(NX, NY, NZ, nranks=2, m=2, n=1, p=1)
    xs0, ys0, zs0, nx0, ny0, nz0 = P2.corners(0)[:6]
    xs1, _, _, nx1, _, _ = P2.corners(1)[:6]
    P2.close()
    assert (xs0, nx0, xs1, nx1) == (0, R.TWO_RANK_SPLIT_X, R.TWO_RANK_SPLIT_X, NX - R.TWO_RANK_SPLIT_X)
    nown = (nx0 * NY * NZ, nx1 * NY * NZ)
    for name, seq in R.SEQUENCES_2R.items():
        for st in seq.steps:
            got, finite = oracle_exc(grid, st.state)
            assert finite
            assert np.array_equal(got, R.closed_form_exc(grid, st.state))
            per = (int(got[:, :, :R.TWO_RANK_SPLIT_X].sum()), int(got[:, :, R.TWO_RANK_SPLIT_X:].sum()))
            assert per == R.TWO_RANK_COUNTS[st.state], (st.state, per)
            for r in (0, 1):
                if per[r]:
                    frac = per[r] / nown[r]
                    assert side(frac, R.ST_FRACTION, R.MARGIN[grid]) != 0
                    assert side(frac, seq.exc_max / 1000, R.MARGIN[grid]) != 0
    c = R.TWO_RANK_COUNTS
    assert c["straddle"][0] > 0 and c["straddle"][1] > 0 and c["right"][0] == 0 and c["left"][1] == 0
    # one_rank_overflows: rank 0 over the lowered limit, rank 1 far under it; at the default limit too
    assert R.overflows(c["slab_x55"][0], nown[0], R.TWO_RANK_EXC_MAX) and not R.overflows(c["slab_x55"][1], nown[1],
                                                                                        R.TWO_RANK_EXC_MAX)
    assert not R.overflows(c["one"][0], nown[0], R.TWO_RANK_EXC_MAX)
