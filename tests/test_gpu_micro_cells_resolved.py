"""Resolved micro cells (n = 21 and 26) against the sparse CPU reference ("Resolved cells against
the sparse reference").

The dense reference ends at n = 12 and solver 0 at n = 20; above that the suite knew only closed forms.  Here
the device-wide solvers are judged by independent numbers at the sizes they exist for: heterogeneous cells
whose third and fourth 8-wide tile per axis hold interior nodes and elements, so every tile-halo staging has
neighbours with non-trivial data on both sides.  The numbers are the fixtures tests/golden/cell_*.npz, written
once on a CPU by tests/golden/make_micro_cells.py from tests/micro_cell_sparse_ref.SparseCellRef, which
tests/test_micro_cell_sparse_cpu.py checks against the dense reference.  This file reads the fixtures only.

Every context takes the fixture's materials (the README's resolved-cell ones) and u = TN.field((2, 2, 2), 5,
amp, wobble=0): one strain e0 at all eight Gauss points, through 1.0 -> commit -> 1.5 -> commit -> 0.5.  The
bars are the project's, with kappa from the fixture:
    sigma, C, f_trial:  100 kappa micro_nl_rtol of the largest entry (f_trial of max|sigma|)
    C_hom:              100 kappa_lin micro_rtol max|C_hom|
Measured on an MI355X: DESIGN §18 has the table.
"""
import functools
import os
import time

import numpy as np
import pytest

import macroc_amd as M
import test_gpu_micro as TM
import test_gpu_micro_nl as TN
import test_gpu_micro_nl_grid as TG
import test_gpu_micro_nl_block as TB
import test_gpu_micro_nl_warm as TW

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NL_RTOL = TN.NL_RTOL
FIXTURES = ("cell_s21_a", "cell_s26_a", "cell_s26_b", "cell_l21_a")


@functools.lru_cache(maxsize=None)
def fixture(name):
    with np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def mat_flags(fx):
    return ("-micro_mat_1", "%r,%r,%r,%r" % tuple(float(v) for v in fx["mat1"]),
            "-micro_mat_2", "%r,%r,%r,%r" % tuple(float(v) for v in fx["mat2"]))


def run(name, repeat=1, **opts):
    """the fixture's load path under micro_nl_solver 1 with opts; every stage evaluated `repeat` times at the
    same u, then committed.  One TW.snap per evaluation, its wall time added."""
    fx = fixture(name)
    u1 = TN.field((2, 2, 2), int(fx["seed"]), float(fx["amp"]), wobble=0)
    out = []
    with TG.grid_ctx(TN.nl_argv(int(fx["typ"]), int(fx["n"]), extra=mat_flags(fx)), **opts) as m:
        for fac in fx["stages"]:
            for _ in range(repeat):
                m.synchronize()
                t0 = time.perf_counter()
                s = TW.snap(m, fac * u1)
                s["seconds"] = time.perf_counter() - t0
                assert np.abs(s["eps"] - fac * fx["e0"]).max() <= 1e-15  # the fixture's strain at all eight points
                out.append(s)
            m.update_vars()
    return out


@functools.lru_cache(maxsize=None)
def default_run(name):
    return run(name)


def check_stage(y, fx, st, what):
    """one evaluation against stage st of the fixture, all eight points; returns the worst error / bar"""
    kappa, sig, C = float(fx["kappa"][st]), fx["sig"][st], fx["C"][st]
    bar = 100 * kappa * NL_RTOL
    es = np.abs(y["sig"] - sig).max() / np.abs(sig).max()
    ec = np.abs(y["C"] - C).max() / np.abs(C).max()
    ef = abs(float(y["f"]) - float(fx["fmax"][st])) / np.abs(sig).max()
    print(f"{what} stage {st}: kappa {kappa:.1f} bar {bar:.2e} err / bar sigma {es / bar:.2e} C {ec / bar:.2e} f_trial "
          f"{ef / bar:.2e}; newton {y['newton_its'].tolist()} ref {int(fx['its'][st])} cg {y['cg_its'].tolist()} rnorm "
          f"{y['rnorm'].max():.1e} warm {y['warm'].tolist()} {y['seconds']:.2f} s")
    assert (y["path"] == fx["path"][st]).all()
    assert es <= bar and ec <= bar and ef <= bar, (what, st, es, ec, ef, bar)
    assert (y["rnorm"] <= NL_RTOL).all()
    for q in range(8):
        assert np.array_equal(y["C"][q], y["C"][q].T)
    return max(es, ec, ef) / bar


# ---------------------------------------------------------------- 1. the plastic cell, default options
@pytest.mark.parametrize("name", FIXTURES)
def test_plastic_cell_against_the_sparse_reference(name):
    fx, out = fixture(name), default_run(name)
    assert len(out) == len(fx["stages"]) == 3
    worst = max(check_stage(y, fx, st, name) for st, y in enumerate(out))
    print(f"{name}: worst error / bar {worst:.2e}")
    assert out[-1]["slots"] >= 8 and (out[0]["newton_its"] >= 1).all()


# ---------------------------------------------------------------- 2. the linear cell
@pytest.mark.parametrize("name", ["cell_s21_a", "cell_s26_a", "cell_l21_a"])
def test_chom_against_the_sparse_reference(name):
    """-mat_law micro -micro_solver grid: the six unit-strain solves at the resolved size"""
    fx = fixture(name)
    typ, n = int(fx["typ"]), int(fx["n"])
    argv = TM.micro_argv(typ, n, extra=("-micro_solver", "grid"), mat1=tuple(fx["mat1"][:2].tolist()),
                         mat2=tuple(fx["mat2"][:2].tolist()))
    with M.Macroc(argv) as m:
        Cg, its, rn = m.micro_ctan()
        ph = m.micro_phase()
    bar = 100 * float(fx["kappa_lin"]) * TM.RTOL
    err = np.abs(Cg - fx["Chom"]).max() / np.abs(fx["Chom"]).max()
    print(f"{name} C_hom: kappa_lin {float(fx['kappa_lin']):.1f} bar {bar:.2e} err / bar {err / bar:.2e} its {tuple(its)} "
          f"rnorm {max(rn):.1e}")
    assert err <= bar
    assert all(r <= TM.RTOL for r in rn) and min(its) >= 1
    assert np.array_equal(Cg, Cg.T)
    assert int(ph.sum()) == int(fx["phase1"])


# ---------------------------------------------------------------- 3. settings that must not change a bit
def test_block_and_fused_give_the_default_bits_at_n26():
    """four node tiles (8, 8, 8, 2) and four element tiles (8, 8, 8, 1) per axis under k_mnlb_* and the fused
    K_T p: the bits of the default run, which test 1 holds to the reference"""
    base = default_run("cell_s26_a")
    split, fused = run("cell_s26_a", micro_nl_tangent=1), run("cell_s26_a", micro_nl_tangent=1, micro_nl_apply=1)
    TB.same_bits(base, split)
    TB.same_bits(base, fused)
    for st, (x, y) in enumerate(zip(split, fused)):
        print(f"n 26 stage {st}: columns {y['cols'][0].tolist()} split {x['seconds']:.2f} s fused {y['seconds']:.2f} s "
              f"default {base[st]['seconds']:.2f} s")
        assert np.array_equal(x["cols"], y["cols"]) and (y["cols"] > 0).all()
        assert not base[st]["cols"].any()  # the sequential columns report no count of their own


def test_batches_of_three_give_the_default_bits_at_n21():
    """micro_mem_blocks 3: the eight points go in batches of 3, 3 and 2"""
    TB.same_bits(default_run("cell_s21_a"), run("cell_s21_a", micro_mem_blocks=3))


# ---------------------------------------------------------------- 4. the warm start
def test_warm_start_at_n21():
    """micro_nl_warm 1, every stage evaluated twice at the same u: the second evaluation starts every point
    from its record, stays within the bar of the same fixture stage and takes fewer CG iterations"""
    fx = fixture("cell_s21_a")
    out = run("cell_s21_a", repeat=2, micro_nl_warm=1)
    assert len(out) == 6
    for st in range(3):
        a, b = out[2 * st], out[2 * st + 1]
        check_stage(a, fx, st, "cell_s21_a warm, first evaluation,")
        check_stage(b, fx, st, "cell_s21_a warm, second evaluation,")
        assert a["path"].all() and (b["warm"] == 2).all()
        print(f"n 21 warm stage {st}: cg {a['cg_its'].sum()} -> {b['cg_its'].sum()} newton {a['newton_its'].max()} -> "
              f"{b['newton_its'].max()}")
        assert b["cg_its"].sum() < a["cg_its"].sum()
    assert (out[0]["warm"] == 1).all()  # a fresh context has no record
